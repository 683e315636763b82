"""Profiling aid: where one decode launch of the one-row int4 kernel spends its time, from the stamped build (ao_int4_set_tuning modes
983: today's grid, 984: the balanced grid).  One eager token of the five Llama-3-8B shapes at g = 128; per shape the workgroups per CU,
the span from the first entry to the last exit split into ramp / body / tail, and the body of CUs that hold 3 against CUs that hold 4
workgroups.  DESIGN.md 4.1 states the two limits the result is judged by.  The block rate is judged on the body of the busiest CUs (first
weight block landed on the CU -> its last wave 0 done): what "blocks per SIMD x block time" predicts.  The same ratio over the whole chip
(which adds the skew with which the CUs receive their workgroups) and over the whole launch (which adds ramp and tail) is written beside it.

    python tools/int4_decode_stamps.py OUT.json
"""
import ctypes
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from ao_amd import ops
from ao_amd._lib import lib as _load

SHAPES = (("qkv", 6144, 4096), ("o", 4096, 4096), ("gate", 14336, 4096), ("up", 14336, 4096), ("down", 4096, 14336))
BLOCK_NS = 190.0  # the laboratory's block time per SIMD at 8 waves (profiles/HISTORY.md 4.1)
STAMPED_K = 4096  # the stamped build is the 8-wave x 4-block form


def stamped_launch(lib, mode, x, q, sz, workgroups):
    trace = torch.zeros(workgroups * 8, dtype=torch.int64, device="cuda")
    lib.ao_int4_set_tuning(0, mode)
    try:
        ops.weight_int4pack_mm(x, q, 128, sz)  # the workspace exists, the code object is loaded
        torch.cuda.synchronize()
        lib.ao_int4_set_trace(ctypes.c_void_p(trace.data_ptr()))
        y = ops.weight_int4pack_mm(x, q, 128, sz)
        torch.cuda.synchronize()
    finally:
        lib.ao_int4_set_trace(ctypes.c_void_p(0))
        lib.ao_int4_set_tuning(0, 0)
    return trace.cpu().numpy().astype(np.int64).reshape(-1, 8), y


def analyse(t, tiles, cus):
    """t: [workgroups][8] = id, 100 MHz entry / exit, shader clock entry / first weight block / wave 0 done / exit, (half + 1) << 32 | tile."""
    cu = ((t[:, 0] >> 32) & 0xF) * 256 + ((t[:, 0] >> 8) & 0xFF)  # XCC | SE, SH, CU of HW_ID
    ids, per_cu = np.unique(cu, return_counts=True)
    mhz = 100.0 * (t[:, 6] - t[:, 3]).sum() / max(1, (t[:, 2] - t[:, 1]).sum())  # shader clock against the 100 MHz clock
    ns = lambda ticks: ticks * 1e3 / mhz  # noqa: E731
    t0 = t[:, 1].min()
    entry = (t[:, 1] - t0) * 10.0  # ns after the first entry
    first = entry + ns(t[:, 4] - t[:, 3])
    done = entry + ns(t[:, 5] - t[:, 3])
    exit_ = entry + ns(t[:, 6] - t[:, 3])
    last = int(np.argmax(exit_))
    half = (t[:, 7] >> 32) > 0
    full = -(-tiles // cus)
    hist = {int(c): int((per_cu == c).sum()) for c in np.unique(per_cu)}
    body_by_count, span_by_count = {}, {}
    for c in hist:
        on = np.isin(cu, ids[per_cu == c])
        body_by_count[c] = round(float((done[on] - first[on]).mean()) / 1e3, 3)
        span_by_count[c] = round(float(np.mean([done[cu == i].max() - first[cu == i].min() for i in ids[per_cu == c]])) / 1e3, 3)
    return {
        "workgroups": int(len(t)), "half_tile_workgroups": int(half.sum()), "cus_seen": int(len(ids)), "shader_mhz": round(float(mhz), 1),
        "workgroups_per_cu": hist,
        "cus_above_full_minus_one": round(float((per_cu > full - 1).mean()), 4),
        "span_us": round(float(exit_.max()) / 1e3, 3),
        # the last workgroup to leave: launch -> its first weight block, -> its wave 0 done with its blocks, -> exit
        "last_exit": {"ramp_us": round(float(first[last]) / 1e3, 3), "body_us": round(float(done[last] - first[last]) / 1e3, 3),
                      "tail_us": round(float(exit_[last] - done[last]) / 1e3, 3), "half": bool(half[last])},
        # over all workgroups: first weight block anywhere -> last wave-0 done anywhere
        "ramp_us": round(float(first.min()) / 1e3, 3), "body_us": round(float(done.max() - first.min()) / 1e3, 3),
        "tail_us": round(float(exit_.max() - done.max()) / 1e3, 3),
        "mean_workgroup": {"entry_us": round(float(entry.mean()) / 1e3, 3), "first_data_us": round(float((first - entry).mean()) / 1e3, 3),
                           "blocks_us": round(float((done - first).mean()) / 1e3, 3), "exit_us": round(float((exit_ - done).mean()) / 1e3, 3)},
        "workgroup_body_us_by_cu_load": body_by_count, "cu_body_span_us_by_cu_load": span_by_count,
    }


def main():
    out_path = sys.argv[1]
    lib = _load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "cus": cus, "block_ns": BLOCK_NS, "shapes": {}}
    weights = {}
    for name, n, k in SHAPES:
        w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16) * 0.02
        weights[name] = tuple(ops.int4_quantize_tinygemm(w, 128)) + (torch.randn(1, k, device="cuda", dtype=torch.bfloat16),)
        del w
    for name, n, k in SHAPES:  # one token: the five launches in layer order
        q, sz, x = weights[name]
        tiles = n // 16
        entry = {"tiles": tiles, "tiles_per_cu": round(tiles / cus, 3)}
        if k != STAMPED_K:
            entry["note"] = "16 waves x 7 blocks: no stamped build of this form (the grid is even: one tile per CU)"
            res["shapes"][name] = entry
            continue
        t, y0 = stamped_launch(lib, 983, x, q, sz, tiles)
        entry["grid"] = analyse(t, tiles, cus)
        # blocks of the busiest SIMD: ceil(tiles / CUs) workgroups of 8 waves x 4 blocks on 4 SIMDs
        blocks = -(-tiles // cus) * 8
        entry["blocks_busiest_simd"] = blocks
        entry["predicted_body_us"] = round(blocks * BLOCK_NS / 1e3, 3)
        busiest = max(entry["grid"]["cu_body_span_us_by_cu_load"])
        entry["busiest_cu_body_us"] = entry["grid"]["cu_body_span_us_by_cu_load"][busiest]
        entry["busiest_cu_body_vs_predicted"] = round(entry["busiest_cu_body_us"] / entry["predicted_body_us"], 3)
        entry["body_vs_predicted"] = round(entry["grid"]["body_us"] / entry["predicted_body_us"], 3)
        entry["span_vs_predicted"] = round(entry["grid"]["span_us"] / entry["predicted_body_us"], 3)
        r = lib.ao_int4_balanced_halves(tiles, cus, 0)
        if r > 0:
            t, y1 = stamped_launch(lib, 984, x, q, sz, tiles + r)
            entry["balanced"] = analyse(t, tiles, cus)
            entry["balanced"]["bit_identical"] = bool(torch.equal(y0.view(torch.int16), y1.view(torch.int16)))
        res["shapes"][name] = entry
    three = [res["shapes"][s] for s in ("qkv", "gate", "up")]
    res["placement_even"] = bool(all(e["grid"]["cus_above_full_minus_one"] < 0.1 for e in three))
    res["block_rate_unexplained"] = bool(any(abs(e["busiest_cu_body_vs_predicted"] - 1) > 0.2 for e in three))
    res["body_unexplained"] = bool(any(abs(e["body_vs_predicted"] - 1) > 0.2 for e in three))
    res["span_unexplained"] = bool(any(abs(e["span_vs_predicted"] - 1) > 0.2 for e in three))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
