"""Per-shape average duration of the one-row int4 launches from rocprofv3 --kernel-trace CSVs of `bench.py` runs (one directory per
build), told apart by their grids: 512-thread workgroups are the K = 4096 form (256 = o, 384 / 512 = qkv, 896 / 1024 = gate and up,
whose launches are identical), 1024-thread ones the K = 14336 form (down).

    python scripts/int4_shape_stats.py OUT.json label=DIR [label=DIR ...]
"""
import csv
import json
import os
import sys

SHAPES = {(512, 256): "o", (512, 384): "qkv", (512, 512): "qkv", (512, 896): "gate_up", (512, 1024): "gate_up", (1024, 256): "down"}


def trace_files(d):
    for root, _, files in os.walk(d):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                yield os.path.join(root, f)


def summarise(d):
    rows = {}
    for path in trace_files(d):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "int4_mm_kernel" not in r["Kernel_Name"]:
                    continue
                wg = int(r["Workgroup_Size_X"])
                key = SHAPES.get((wg, int(r["Grid_Size_X"]) // wg))
                if key is None or int(r["Grid_Size_Y"]) != 1:
                    continue
                rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), int(r["Grid_Size_X"]) // wg))
    out = {}
    for key, v in sorted(rows.items()):
        ns = sorted(t for t, _ in v)
        out[key] = {"launches": len(ns), "workgroups": sorted({g for _, g in v}), "avg_us": round(sum(ns) / len(ns) / 1e3, 3),
                    "median_us": round(ns[len(ns) // 2] / 1e3, 3), "p10_us": round(ns[len(ns) // 10] / 1e3, 3), "p90_us": round(ns[len(ns) * 9 // 10] / 1e3, 3)}
    return out


def main():
    res = {"source": "rocprofv3 --kernel-trace --stats -- python bench.py --steps 10 (one run per build, no counters); every int4_mm_kernel "
                     "dispatch of the process (eager first touch, capture warm-up and graph replays)", "builds": {}}
    for arg in sys.argv[2:]:
        label, d = arg.split("=", 1)
        res["builds"][label] = summarise(d)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
