#!/usr/bin/env python3
"""bench.py -- linear-layer tokens/s of the low-bit Llama / Mixtral linears on MI355X (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run measures the headline alone: set-up, W warm-up steps, K timed steps, the line (metric, value, unit, ms_per_step, ...).
--dump-outputs DIR writes what the timed path returned in its last step as DIR/<module>.npy (float32; see dump_outputs).
--full adds everything else below: the roofline, the other module layout, the subclass / stack baselines, the secondary configs,
the CPU baselines and, with N > 1 ranks or --force-tp, the TP leg.

Headline (the ONE JSON line's metric / value / roofline / cpu_baseline) = BASELINE.json configs[1]:
Int4WeightOnlyConfig(group_size=128), Llama-3-8B linear shapes, bs=1 seq=1.  One "step" = one token through every
linear of the 32 layers in the five-shape layout of SURVEY.md 8(d) (qkv 6144x4096, o 4096x4096, gate 14336x4096,
up 14336x4096, down 4096x14336: 160 launches), every layer with its own weights (3.7 GB resident, far beyond the
256 MiB Infinity Cache), inputs synthetic and already in HBM, one stream, launches replayed from a hipGraph.  The
serving-stack layout with gate and up merged into one 28672x4096 linear (vLLM; 128 launches, same bytes) is timed
in the same run and reported in config.merged_tokens_per_s.

The same line carries `configs`, one object per other BASELINE.json config, each with its own value, roofline and
cpu_baseline (rank 0, N = 1 runs):
  int4_bs128          configs[1]'s second half (bs = 128): same weights, 128-row activations (MFMA-bound)
  int8_dyn_bs128x2048 configs[2]: int8 dynamic-activation / int8-weight, M = 128 x 2048 = 262144 rows in 16384-row chunks
  fp8_tp8_shards      configs[3], one GPU's share: Float8 rowwise, the Llama-3-70B TP=8 shard linears, M in {1, 128, 2048}
  mxfp8_mixtral_bs64  configs[4]: MXFP8 grouped GEMM, Mixtral-8x7B expert shapes, 64 tokens x top-2
With N > 1 ranks: the headline runs one replica per GPU (the decode path partitions by token stream, no data-path
collective: "weak"), and `configs.fp8_tp` runs configs[3] for real -- Llama-3-70B linears sharded TP = N
(ao_amd/parallel.py: column-parallel qkv / gate_up, row-parallel o / down + RCCL all-reduce), all-reduce time separate.

roofline     -- dominant kernel: algorithmic bytes (or flops) per launch / average kernel duration from HIP extension
                events on the launch stream; the committed rocprofv3 summary of the same command is quoted beside it
cpu_baseline -- oracle/lowbit_ref.c ("port" of the reference CPU dequant -> matmul path) on a bounded sample
"""
import argparse
import ctypes
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from ao_amd import roofline as _roofline  # noqa: E402  (the gfx950 entry of a roofline_utils.py-style spec table)

_SPECS = _roofline.get_specs("AMD Instinct MI355X")
HBM_PEAK_GBS = _SPECS["peak_mem_bw_bytes_sec"] / 1e9   # 8000: MI355X HBM3E spec (MI355X_MICROARCH.md)
MFMA_BF16_PEAK_TFLOPS = _SPECS["bf16_peak_tops"] / 1e12  # 2500: dense bf16 MFMA
MFMA_8BIT_PEAK_TOPS = _SPECS["fp8_peak_tops"] / 1e12     # 5000: dense fp8 / int8 MFMA (fp8 ~5 PF dense, int8 ~2x the bf16 rate)
ROUND = "r06"                    # names of the committed rocprofv3 summaries under profiles/
PREV_ROUNDS = ("r06", "r05")     # a summary of this round when it exists, else the last round's (the source file is named beside every number)


def _profile_path(stem, ext):
    for r in PREV_ROUNDS:
        path = os.path.join(ROOT, "profiles", f"{stem}_{r}.{ext}")
        if os.path.exists(path):
            return path
    return None

LLAMA3_8B_MERGED = [("qkv_proj", 6144, 4096), ("o_proj", 4096, 4096), ("gate_up_proj", 28672, 4096), ("down_proj", 4096, 14336)]
LLAMA3_8B_UNMERGED = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate", 14336, 4096), ("up", 14336, 4096), ("down", 4096, 14336)]
LLAMA3_70B = [("qkv_proj", 10240, 8192, "col"), ("o_proj", 8192, 8192, "row"), ("gate_up_proj", 57344, 8192, "col"), ("down_proj", 8192, 28672, "row")]
MIXTRAL = [("w1", 14336, 4096), ("w3", 14336, 4096), ("w2", 4096, 14336)]
N_LAYERS = 32
GROUP = 128


def algorithmic_bytes(m, n, k, g):
    """packed weights + scales/zeros + activation + output."""
    return n * k // 2 + (k // g) * n * 4 + m * k * 2 + m * n * 2


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1, help="tokens per step of the headline run (BASELINE headline is 1)")
    ap.add_argument("--layers", type=int, default=N_LAYERS)
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--merged", action="store_true", help="headline on the vLLM layout (gate_up merged) instead of the five shapes")
    ap.add_argument("--unmerged", action="store_true", help=argparse.SUPPRESS)  # round-1 flag: the five shapes are the default now
    ap.add_argument("--no-second-layout", action="store_true", help="skip the short run of the other module layout")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="headline only (profiling runs)")
    ap.add_argument("--configs", default="int4_bs128,int8,fp8,mx,tp", help="comma list of secondary configs to run")
    ap.add_argument("--mx-two-launch", action="store_true", help="config mx: time the cast kernel + GEMM form as the config's value (A/B)")
    ap.add_argument("--mx-no-pair", action="store_true", help="config mx: one launch per product (w1 and w3 apart) as the config's value (A/B)")
    ap.add_argument("--wpb", type=int, default=0, help="tuning: waves per workgroup override")
    ap.add_argument("--mode", type=int, default=0, help="tuning: kernel ablation / depth variant (profiling only)")
    ap.add_argument("--force-tp", action="store_true", help="run the TP-linear config even with one rank (exercises the RCCL path on a 1-GPU box)")
    ap.add_argument("--gemm-variant", type=int, default=0, help="tuning: ao_gemm8_set_variant for the 8-bit configs (profiling only)")
    ap.add_argument("--tp-graph", action="store_true", help=argparse.SUPPRESS)  # round 2's opt-in; graph replay is the default now
    ap.add_argument("--no-tp-graph", action="store_true", help="TP config: launch eagerly (default: each step -- kernels + RCCL collectives -- replays from a hipGraph, eager if the capture fails)")
    ap.add_argument("--fp8-layers", type=int, default=80, help="fp8 shard config: layers (80 = Llama-3-70B; counter-collection passes use fewer)")
    ap.add_argument("--no-stack-baseline", action="store_true", help="skip the PyTorch-core (what torchao-on-ROCm runs today) timing")
    ap.add_argument("--no-subclass-graph", action="store_true", help="skip the quantize_()-subclass + F.linear graph timing (a13)")
    ap.add_argument("--tp-timeout", type=int, default=int(os.environ.get("AO_BENCH_TP_TIMEOUT", "240")), help="seconds the TP leg of a multi-GPU run may take before every rank leaves and rank 0 prints the line without it")
    ap.add_argument("--tp-one-shot", action="store_true", help="TP config: accumulator all-reduces of <= 1 MiB through the symmetric-memory one-shot path (prototype; default RCCL)")
    ap.add_argument("--full", action="store_true", help="also the roofline, the other layout, the baselines, the secondary configs and the TP leg "
                                                         "(a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs as DIR/<module>.npy (float32)")
    return ap.parse_args()


# ----------------------------------------------------------------------------------------------------------------------
# timing helpers
# ----------------------------------------------------------------------------------------------------------------------
def capture(fn, stream, use_graph=True, collectives=False):
    """Run fn once eagerly (first touch, lazy workspaces), then capture it into a hipGraph.  Returns a replay callable.
    collectives: fn issues RCCL collectives.  ProcessGroupNCCL's watchdog thread polls the events of every collective issued so far
    (hipEventQuery, every ~100 ms); in the default "global" capture mode such a call from ANOTHER thread while this one captures
    invalidates the capture, and the works issued during the broken capture then take the process down from the watchdog
    (hipErrorCapturedEvent -> std::terminate; seen once in six runs of the world-1 TP leg, profiles/tp_capture_abort_r03.txt).  So:
    let the watchdog reap everything that is outstanding before the capture starts, and capture in thread-local mode."""
    with torch.cuda.stream(stream):
        fn()
        stream.synchronize()
        if not use_graph:
            return fn, False
        try:
            g = torch.cuda.CUDAGraph()
            if collectives:
                torch.cuda.synchronize()
                time.sleep(0.5)
            with torch.cuda.graph(g, stream=stream, **({"capture_error_mode": "thread_local"} if collectives else {})):
                fn()
            return g.replay, True
        except Exception as e:  # noqa: BLE001
            print(f"warning: hipGraph capture failed ({e!r}); launching eagerly", file=sys.stderr)
            return fn, False


def time_steps(run, stream, device, steps, warmup, dist=None):
    """W untimed steps, then exactly `steps` steps bracketed by barrier + synchronize; MAX over ranks.  Seconds."""
    def sync_all():
        torch.cuda.synchronize(device)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(device)

    with torch.cuda.stream(stream):
        for _ in range(warmup):
            run()
        sync_all()
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        torch.cuda.synchronize(device)
        elapsed = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([elapsed], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        sync_all()
    return elapsed


def event_profile(lib, check, fn, n_max):
    """Per-launch kernel durations (ms) of one eager pass via HIP extension events (ao_prof_enable / collect)."""
    check(lib.ao_prof_enable(n_max))
    fn()
    buf = (ctypes.c_float * n_max)()
    cnt = ctypes.c_int(0)
    check(lib.ao_prof_collect(buf, n_max, ctypes.byref(cnt)))
    return np.array(buf[: cnt.value], dtype=np.float64)


def rocprof_avg_us(kernel_substr):
    """Average duration of a kernel in the committed rocprofv3 --kernel-trace --stats summary (profiles/), or None.  Every row whose
    name contains the substring counts (the decode kernel is several template instantiations: 4- and 7-deep straight-line forms)."""
    path = _profile_path("int4_kernel_stats", "csv")
    if path is None:
        return None, None
    total_ns, calls = 0.0, 0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if kernel_substr in row.get("Name", ""):
                total_ns += float(row["TotalDurationNs"])
                calls += int(row["Calls"])
    if calls == 0:
        return None, None
    return total_ns / calls / 1e3, os.path.relpath(path, ROOT)


def rocprof_crosscheck():
    """profiles/int4_rocprof_crosscheck_<round>.json (scripts/rocprof_crosscheck.py), or None."""
    path = _profile_path("int4_rocprof_crosscheck", "json")
    if path is None:
        return None
    with open(path) as f:
        d = json.load(f)
    d["_path"] = os.path.relpath(path, ROOT)
    return d


def pmc_traffic_of(config_key, workload=None):
    """HBM bytes per launch of a secondary config's dominant kernel from the committed rocprofv3 PMC summary
    (profiles/configs_pmc_<round>.json, scripts/gpu_profile.sh: FETCH_SIZE x 2 on gfx950 + WRITE_SIZE, separate passes)."""
    path = _profile_path("configs_pmc", "json")
    if path is None:
        return None, None
    with open(path) as f:
        d = json.load(f)
    e = d.get("configs", {}).get(config_key)
    if not e:
        return None, None
    if workload is not None:  # a config that times more than one workload in one process (MX): its dispatches split by order
        w = e.get("by_workload", {}).get(workload)
        return (w.get("hbm_bytes_per_launch"), f"{os.path.relpath(path, ROOT)}: {e.get('kernel', '?')} ({workload})") if w else (None, None)
    return e.get("hbm_bytes_per_launch"), f"{os.path.relpath(path, ROOT)}: {e.get('kernel', '?')}"


def pmc_traffic(kernel, layout="five"):
    """layout: the module layout the counters were collected on -- the merged (vLLM) layout has its own pass (int4_pmc_merged_<round>.json);
    the five-shape figure is never quoted for it (its launches read 29.0 MB on average, not 23.2)."""
    path = _profile_path("int4_pmc" if layout == "five" else "int4_pmc_merged", "json")
    if path is None:
        return None, None
    with open(path) as f:
        d = json.load(f)
    v = d.get("kernels", {}).get(kernel, {}).get("hbm_bytes_per_launch")
    return v, (os.path.relpath(path, ROOT) if v is not None else None)


# ----------------------------------------------------------------------------------------------------------------------
# int4 weight-only (headline, bs = 128)
# ----------------------------------------------------------------------------------------------------------------------
class Int4Linears:
    """All packed weights of the synthetic model + raw C-ABI launch lists per batch size."""

    def __init__(self, device, layers, shapes):
        from ao_amd import _lib, ops

        self.lib = _lib.lib()
        self.check = _lib.check
        self.device = device
        self.shapes = shapes
        self.weights = []  # (qdata, sz, n, k, name)
        self.gen = torch.Generator(device=device).manual_seed(0)
        for _ in range(layers):
            for name, n, k in shapes:
                # random-init weights of the real shape, quantized by the product kernel
                w = torch.randn(n, k, device=device, dtype=torch.bfloat16, generator=self.gen) * 0.02
                qdata, sz = ops.int4_quantize_tinygemm(w, GROUP)
                del w
                self.weights.append((qdata, sz, n, k, name))
        self.io = {}
        torch.cuda.synchronize()

    def launches(self, batch):
        if batch not in self.io:
            keep, lst = [], []
            for qdata, sz, n, k, name in self.weights:
                x = torch.randn(batch, k, device=self.device, dtype=torch.bfloat16, generator=self.gen)
                y = torch.empty(batch, n, device=self.device, dtype=torch.bfloat16)
                keep.append((x, y))
                lst.append((x.data_ptr(), qdata.data_ptr(), sz.data_ptr(), y.data_ptr(), batch, n, k, name))
            self.io[batch] = (keep, lst)
        return self.io[batch][1]

    def step(self, batch, stream_ptr, side_stream=None):
        """One token through every linear.  side_stream (tools/int4_branches.py): launch every `up` projection on it, forked after the
        previous launch and joined before the next one -- gate and up read the same activation and are independent in a real layer."""
        f = self.lib.ao_int4_weight_int4pack_mm
        cur = torch.cuda.current_stream()
        for (xp, qp, sp, yp, m, n, k, name) in self.launches(batch):
            forked = side_stream is not None and name == "up"
            if side_stream is not None and name == "gate":
                side_stream.wait_stream(cur)  # fork: up may start as soon as what precedes gate is done
            rc = f(xp, qp, sp, yp, m, n, k, GROUP, side_stream.cuda_stream if forked else stream_ptr)
            if rc != 0:
                self.check(rc)
            if forked:
                cur.wait_stream(side_stream)  # join before down

    def bytes_per_step(self, batch):
        return sum(algorithmic_bytes(batch, n, k, GROUP) for (_, _, n, k, _) in self.weights)

    def flops_per_step(self, batch):
        return sum(2.0 * batch * n * k for (_, _, n, k, _) in self.weights)


def run_int4(model, batch, steps, warmup, stream, device, use_graph, dist=None):
    """(seconds, graphed) for `steps` steps of the int4 model at `batch` rows."""
    cur = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    run, graphed = capture(lambda: model.step(batch, cur()), stream, use_graph)
    return time_steps(run, stream, device, steps, warmup, dist), graphed


DUMP_BUDGET_BYTES = 60_000_000  # array data of one --dump-outputs, under 64 MB with the .npy headers


def dump_outputs(model, batch, out_dir):
    """What a caller of the timed path receives from its last step: every linear's bf16 output, as float32, one file per module
    name with the layers stacked ([layers, rows, n]).  The inputs come from seeded generators, so the same arguments give the
    same files on every run.  Beyond DUMP_BUDGET_BYTES in all, a fixed seeded sample of rows (then of layers) is written, the
    same sample for every module.  Returns ({name: shape written}, rows written, layers written)."""
    os.makedirs(out_dir, exist_ok=True)
    keep, lst = model.io[batch]
    by_name = {}
    for (_, y), launch in zip(keep, lst):
        by_name.setdefault(launch[-1], []).append(y)
    layers = len(next(iter(by_name.values())))
    row_bytes = 4 * sum(len(ys) * ys[0].shape[1] for ys in by_name.values())  # one row of every output of every layer
    rng = np.random.default_rng(0)
    rows = np.arange(batch)
    if batch * row_bytes > DUMP_BUDGET_BYTES:
        rows = np.sort(rng.choice(batch, max(1, DUMP_BUDGET_BYTES // row_bytes), replace=False))
    lays = np.arange(layers)
    if len(rows) * row_bytes > DUMP_BUDGET_BYTES:
        lays = np.sort(rng.choice(layers, max(1, DUMP_BUDGET_BYTES * layers // row_bytes), replace=False))
    rows_t = torch.from_numpy(rows).to(model.device)
    shapes = {}
    for name, ys in by_name.items():
        a = torch.stack([ys[i].index_select(0, rows_t) for i in lays]).float().cpu().numpy()
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        shapes[name] = list(a.shape)
    return shapes, rows.tolist(), lays.tolist()


def int4_kernel_table(model, batch, stream):
    """Event-timed per-launch durations of one eager step, grouped by shape and by kernel."""
    lib = model.lib
    sp = stream.cuda_stream
    with torch.cuda.stream(stream):
        durs = [event_profile(lib, model.check, lambda: model.step(batch, sp), len(model.weights)) for _ in range(3)]
    prof = np.mean(np.stack(durs), axis=0)  # ms per launch, launch order
    per_shape, kernels = {}, {}
    for name, n, k in model.shapes:
        idx = [i for i, w in enumerate(model.weights) if w[4] == name]
        b = algorithmic_bytes(batch, n, k, GROUP)
        ms = float(prof[idx].mean())
        kern = lib.ao_int4_mm_kernel_name(batch, n, k, GROUP).decode()
        per_shape[name] = {"N": n, "K": k, "bytes": b, "us": ms * 1e3, "GBps": b / (ms * 1e-3) / 1e9, "kernel": kern}
        kk = kernels.setdefault(kern, {"launches_per_step": 0, "bytes_per_step": 0, "flops_per_step": 0.0, "ms_per_step": 0.0})
        kk["launches_per_step"] += len(idx)
        kk["bytes_per_step"] += b * len(idx)
        kk["flops_per_step"] += 2.0 * batch * n * k * len(idx)
        kk["ms_per_step"] += float(prof[idx].sum())
    for kk in kernels.values():
        kk["avg_kernel_us"] = kk["ms_per_step"] * 1e3 / kk["launches_per_step"]
        kk["algorithmic_bytes_per_launch"] = kk["bytes_per_step"] / kk["launches_per_step"]
        kk["GBps"] = kk["bytes_per_step"] / (kk["ms_per_step"] * 1e-3) / 1e9
        kk["TFLOPs"] = kk["flops_per_step"] / (kk["ms_per_step"] * 1e-3) / 1e12
    return prof, per_shape, kernels


def int4_roofline(model, batch, stream, layout="five"):
    prof, per_shape, kernels = int4_kernel_table(model, batch, stream)
    dom = max(kernels, key=lambda k_: kernels[k_]["ms_per_step"])
    kd = kernels[dom]
    mfma_bound = batch >= 64  # past the HBM ridge: weights are dequantised to bf16 and multiplied on the bf16 MFMA path
    out = {
        "kernel": dom,
        "bound": "mfma" if mfma_bound else "hbm",
        "achieved": kd["TFLOPs"] if mfma_bound else kd["GBps"],
        "peak": MFMA_BF16_PEAK_TFLOPS if mfma_bound else HBM_PEAK_GBS,
        "unit": "TFLOP/s" if mfma_bound else "GB/s",
        "avg_kernel_us": kd["avg_kernel_us"],
        "measured_ceiling": (_SPECS["bf16_measured_mfma_tops"] / 1e12) if mfma_bound else (_SPECS["measured_read_bw_bytes_sec"] / 1e9),
        "timing": "HIP extension events on the launch stream, one eager step, mean of 3",
        "launches_per_step": len(model.weights),
        "sum_kernel_ms_per_step": float(prof.sum()),
        "kernels": kernels,
        "per_shape": per_shape,
    }
    if mfma_bound and len(kernels) > 1:
        # round 5: the batched path is two kernels by shape (int4_mm_w32_kernel on the wide projections, int4_mm_rb_kernel on the others):
        # the config's roofline figure is ALL its launches' flops over ALL their kernel time, not the larger kernel's share
        tot_ms = sum(k_["ms_per_step"] for k_ in kernels.values())
        out["kernel"] = " + ".join(sorted(kernels))
        out["achieved"] = sum(k_["flops_per_step"] for k_ in kernels.values()) / (tot_ms * 1e-3) / 1e12
        out["avg_kernel_us"] = tot_ms * 1e3 / len(model.weights)
    out["frac"] = out["achieved"] / out["peak"]
    if mfma_bound:
        out["peak_note"] = ("dense bf16 MFMA peak: the int4 weights are dequantised to bf16 (the oracle's arithmetic) and multiplied by "
                            "v_mfma_f32_16x16x32_bf16 / v_mfma_f32_32x32x16_bf16; the fp8 peak named by north_star does not bound this kernel")
        out["frac_of_fp8_mfma_peak"] = out["achieved"] / MFMA_8BIT_PEAK_TOPS
        out["traffic"], out["traffic_source"] = pmc_traffic_of("int4_bs128")
    else:
        out["algorithmic_bytes_per_launch"] = kd["algorithmic_bytes_per_launch"]
        out["traffic"], out["traffic_source"] = pmc_traffic(dom, layout)
        avg, src = rocprof_avg_us(dom + "<") if layout == "five" else (None, None)
        xc = rocprof_crosscheck() if layout == "five" else None
        if xc is not None:
            # round 6: the kernel trace of the process that printed a bench line, cut to that line's timed replays (scripts/rocprof_crosscheck.py):
            # sum of kernel durations per step <= the profiler's wall span per step ~ that line's ms_per_step -- a figure that passes its own check
            avg, src = xc["avg_kernel_us"], xc["_path"]
        if avg is not None:  # the committed rocprofv3 --kernel-trace summary of this command
            out["rocprof"] = {"avg_kernel_us": avg, "achieved": kd["algorithmic_bytes_per_launch"] / (avg * 1e-6) / 1e9,
                              "frac": kd["algorithmic_bytes_per_launch"] / (avg * 1e-6) / 1e9 / HBM_PEAK_GBS, "source": src}
            if xc is not None:
                out["rocprof"].update({k_: xc[k_] for k_ in ("line_ms_per_step", "rocprof_span_ms_per_step", "rocprof_sum_kernel_ms_per_step", "cross_check")})
    return out


def replay_stats(models, batch, stream, device, rounds=5, steps=10):
    """Median / min / max tokens/s over `rounds` ALTERNATING graph replays of several weight layouts in one process: the pool's
    boxes differ by a few per cent and a single timed region cannot tell a layout effect from a box effect."""
    graphs = {}
    for name, model in models.items():
        run, graphed = capture(lambda m=model: m.step(batch, torch.cuda.current_stream().cuda_stream), stream)
        graphs[name] = run
    times = {name: [] for name in models}
    with torch.cuda.stream(stream):
        for _ in range(rounds):
            for name, run in graphs.items():
                run()
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                for _ in range(steps):
                    run()
                torch.cuda.synchronize(device)
                times[name].append((time.perf_counter() - t0) / steps)
    out = {}
    for name, t in times.items():
        t = sorted(t)
        out[name] = {"tokens_per_s_median": batch / t[len(t) // 2], "tokens_per_s_best": batch / t[0], "tokens_per_s_worst": batch / t[-1],
                     "rounds": rounds, "steps_per_round": steps}
    return out


def subclass_graph_tokens_per_s(model, stream, device, steps=20):
    """SURVEY.md 8 row a13, measured: the SAME 160 packed weights wrapped as Int4TilePackedTo4dTensor parameters of nn.Linear
    modules (what quantize_() leaves behind), one token through `module(x)` = F.linear -> __torch_function__ -> the kernel, the
    whole token captured in a hipGraph (how a serving stack runs decode).  Eager tokens/s is reported beside it: the Python
    dispatch + ctypes hop per linear is what the graph removes."""
    from ao_amd.quantization.int4_tensor import Int4TilePackedTo4dTensor

    mods, xs = [], []
    for qdata, sz, n, k, _ in model.weights:
        lin = torch.nn.Linear(k, n, bias=False, device="meta", dtype=torch.bfloat16)
        lin.weight = torch.nn.Parameter(Int4TilePackedTo4dTensor(qdata, sz, [1, GROUP], torch.Size([n, k])), requires_grad=False)
        mods.append(lin)
    for (xp, qp, sp, yp, m, n, k, _), (x, _y) in zip(model.launches(1), model.io[1][0]):
        xs.append(x)
    def step():
        for lin, x in zip(mods, xs):
            lin(x)
    with torch.no_grad():
        eager = time_steps(step, stream, device, 5, 2) / 5
        run, graphed = capture(step, stream)
        t = time_steps(run, stream, device, steps, 3) / steps
    return {"tokens_per_s": 1.0 / t, "eager_tokens_per_s": 1.0 / eager, "launch": "hipGraph replay" if graphed else "eager",
            "path": "nn.Linear(weight=Int4TilePackedTo4dTensor).forward -> F.linear -> __torch_function__ -> ao_int4_weight_int4pack_mm"}


def stack_baseline(model, stream, device, args):
    """What torchao-on-ROCm runs TODAY on this box, timed beside our kernels (never the target): PyTorch core's own
    aten::_weight_int4pack_mm (the op Int4TilePackedTo4dTensor calls, int4_tile_packed_to_4d_tensor.py:287) on the same packed
    weights (the layouts are bit-identical) in the same 160-launch hipGraph, core's aten::_int_mm (int8/kernels.py:70) and
    aten::_scaled_mm rowwise (float8/inference.py:104) on one representative shape each."""
    out = {"note": "PyTorch-core kernels (hipBLASLt / core's hipified int4mm) on the same box and inputs; a same-node reference, not the target"}
    if os.environ.get("AO_MI355_OVERRIDE_ATEN") == "1":
        return {"skipped": "AO_MI355_OVERRIDE_ATEN=1: the aten ops ARE our kernels in this process"}
    try:
        ios = model.launches(1)
        keep = model.io[1][0]
        ws = model.weights
        def step():
            for (x, _y), (qdata, sz, n, k, _) in zip(keep, ws):
                torch.ops.aten._weight_int4pack_mm(x, qdata, GROUP, sz)
        with torch.no_grad():
            run, graphed = capture(step, stream)
            t = time_steps(run, stream, device, 10, 2) / 10
        out["int4_bs1"] = {"op": "aten::_weight_int4pack_mm (PyTorch core)", "tokens_per_s": 1.0 / t, "launch": "hipGraph replay" if graphed else "eager"}
        del ios
    except Exception as e:  # noqa: BLE001
        out["int4_bs1"] = {"error": repr(e)}
    try:
        m, n, k = 16384, 14336, 4096
        a = torch.randint(-127, 127, (m, k), device=device, dtype=torch.int8)
        b = torch.randint(-127, 127, (n, k), device=device, dtype=torch.int8)
        fn = lambda: torch._int_mm(a, b.t())  # noqa: E731
        with torch.no_grad():
            run, graphed = capture(fn, stream)
            t = time_steps(run, stream, device, 5, 2) / 5
        out["int8_gemm"] = {"op": "aten::_int_mm (PyTorch core)", "shape": [m, n, k], "TOPs": 2.0 * m * n * k / t / 1e12, "ms": t * 1e3}
        del a, b
    except Exception as e:  # noqa: BLE001
        out["int8_gemm"] = {"error": repr(e)}
    try:
        m, n, k = 2048, 7168, 8192
        a = torch.randn(m, k, device=device).to(torch.float8_e4m3fn)
        b = torch.randn(n, k, device=device).to(torch.float8_e4m3fn)
        sa, sb = torch.rand(m, 1, device=device) + 0.5, torch.rand(1, n, device=device) + 0.5
        fn = lambda: torch._scaled_mm(a, b.t(), scale_a=sa, scale_b=sb, out_dtype=torch.bfloat16, use_fast_accum=True)  # noqa: E731
        with torch.no_grad():
            run, graphed = capture(fn, stream)
            t = time_steps(run, stream, device, 5, 2) / 5
        out["fp8_rowwise_gemm"] = {"op": "aten::_scaled_mm rowwise (PyTorch core)", "shape": [m, n, k], "TFLOPs": 2.0 * m * n * k / t / 1e12, "ms": t * 1e3}
    except Exception as e:  # noqa: BLE001
        out["fp8_rowwise_gemm"] = {"error": repr(e)}
    torch.cuda.empty_cache()
    return out


def _reference_root():
    """Where the REAL reference can be imported from: the checkout (build container) or its staged Python under oracle/_ref (built by
    `make -C oracle ref`; travels to the GPU box with the snapshot).  Only the cpu_baseline leg uses it."""
    for ref in ("/root/reference", os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle", "_ref")):
        if os.path.isdir(os.path.join(ref, "torchao")):
            return ref
    return None


def reference_cpu_baseline_int4(batch=1):
    """BASELINE.md section 3 by the letter, when the reference checkout is reachable (the build container; never the GPU box):
    torchao's own groupwise_affine_dequantize_tensor_from_qparams + bf16 F.linear on ONE layer's five linears at M = 1."""
    ref = _reference_root()
    if ref is None:
        return None
    try:
        sys.path.insert(0, ref)
        os.environ.setdefault("TORCHAO_FORCE_SKIP_LOADING_SO_FILES", "1")  # a checkout's CUDA .so files are not for this box
        from torchao.quantization.utils import groupwise_affine_dequantize_tensor_from_qparams, groupwise_affine_quantize_tensor_from_qparams, get_groupwise_affine_qparams  # noqa: E501
        ops = []
        for _, n, k in LLAMA3_8B_UNMERGED:
            w = torch.randn(n, k, dtype=torch.bfloat16) * 0.02
            sc, zp = get_groupwise_affine_qparams(w, 4, GROUP, torch.bfloat16)
            q = groupwise_affine_quantize_tensor_from_qparams(w, sc, zp, 4, GROUP)
            ops.append((q, sc, zp, torch.randn(batch, k, dtype=torch.bfloat16)))
        tt, reps, t_begin = 0.0, 0, time.perf_counter()
        while reps < 1 or (time.perf_counter() - t_begin < 8.0 and reps < 20):  # bounded: ~10 s of host time
            for q, sc, zp, x in ops:
                t0 = time.perf_counter()
                wd = groupwise_affine_dequantize_tensor_from_qparams(q, sc, zp, 4, GROUP)
                torch.nn.functional.linear(x, wd)
                tt += time.perf_counter() - t0
            reps += 1
        tt /= reps
        return {"value": batch / (tt * N_LAYERS), "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "reference", "ms_per_layer": tt * 1e3,
                "sample": f"1 of 32 layers (5 linears) at M = {batch} through torchao's groupwise_affine_dequantize_tensor_from_qparams + bf16 F.linear "
                          f"(torch CPU, {torch.get_num_threads()} threads, host has {os.cpu_count()} cpus), mean of {reps} reps, x32 extrapolated"}
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)}
    finally:
        if sys.path and sys.path[0] == ref:
            sys.path.pop(0)


def _with_reference(fn):
    """Run fn() with the REAL reference importable (the checkout, or its staged Python under oracle/_ref on the GPU box); None when it is
    not reachable, {"error": ...} when the reference's own code raises.  cpu_baseline legs only."""
    ref = _reference_root()
    if ref is None:
        return None
    sys.path.insert(0, ref)
    os.environ.setdefault("TORCHAO_FORCE_SKIP_LOADING_SO_FILES", "1")
    try:
        out = fn()
        out["reference_root"] = ref
        return out
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)[:300]}
    finally:
        if sys.path and sys.path[0] == ref:
            sys.path.pop(0)


def _mean_time(fn, budget_s=6.0, max_reps=20):
    """torchao.utils.benchmark_model semantics (utils.py:115-127: wall-clock mean) under a time budget: one warm-up, then reps until
    the budget is spent (at least one)."""
    fn()
    tt, reps, t_begin = 0.0, 0, time.perf_counter()
    while reps < 1 or (time.perf_counter() - t_begin < budget_s and reps < max_reps):
        t0 = time.perf_counter()
        fn()
        tt += time.perf_counter() - t0
        reps += 1
    return tt / reps, reps


def reference_cpu_baseline_int8(rows=16):
    """BASELINE.md section 3 for configs[2]: the reference's OWN Int8DynamicActivationInt8WeightConfig path on CPU tensors -- quantize_()
    leaves Int8Tensor weights, F.linear dispatches to its dynamic activation cast + int matmul + scales (int8_tensor.py:266-359)."""
    def run():
        from torchao.quantization import Int8DynamicActivationInt8WeightConfig, quantize_
        torch.manual_seed(0)
        mods = []
        for _, n, k in LLAMA3_8B_UNMERGED:
            lin = torch.nn.Linear(k, n, bias=False, dtype=torch.bfloat16)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(n, k, dtype=torch.bfloat16) * 0.02)
            quantize_(lin, Int8DynamicActivationInt8WeightConfig())
            mods.append((lin, torch.randn(rows, k, dtype=torch.bfloat16)))
        def layer():
            with torch.no_grad():
                for lin, x in mods:
                    lin(x)
        t, reps = _mean_time(layer)
        return {"value": rows / (t * N_LAYERS), "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "reference", "ms_per_layer": t * 1e3,
                "sample": f"{rows} rows through the 5 linears of 1 of 32 layers: torchao's own quantize_(Int8DynamicActivationInt8WeightConfig) + F.linear on CPU tensors "
                          f"(Int8Tensor dispatch: dynamic per-row cast + int mm + scales; torch CPU, {torch.get_num_threads()} threads, host has {os.cpu_count()} cpus), mean of {reps} reps, x32 extrapolated"}
    return _with_reference(run)


def reference_cpu_baseline_fp8(layers, rows=8):
    """configs[3]: Float8Tensor.from_hp(PerRow) for weight and activation, .dequantize() of both, bf16 F.linear -- the reference's CPU-runnable
    path for float8 rowwise (its _scaled_mm branch asserts a GPU; BASELINE.md section 3 names dequantize() + matmul)."""
    def run():
        from torchao.quantization import PerRow
        from torchao.quantization.quantize_.workflows.float8.float8_tensor import Float8Tensor
        torch.manual_seed(0)
        ws = []
        for name, n, k, style in LLAMA3_70B:
            ns, ks = (n // 8, k) if style == "col" else (n, k // 8)
            w = torch.randn(ns, ks, dtype=torch.bfloat16) * 0.02
            ws.append((Float8Tensor.from_hp(w, torch.float8_e4m3fn, PerRow()), torch.randn(rows, ks, dtype=torch.bfloat16)))
        def layer():
            with torch.no_grad():
                for wq, x in ws:
                    xq = Float8Tensor.from_hp(x, torch.float8_e4m3fn, PerRow())
                    torch.nn.functional.linear(xq.dequantize(), wq.dequantize())
        t, reps = _mean_time(layer)
        return {"value": rows / (t * layers), "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "reference", "ms_per_layer": t * 1e3,
                "sample": f"{rows} rows through the 4 TP=8 shard linears of 1 of {layers} layers: torchao's Float8Tensor.from_hp(PerRow) on activation and weight, "
                          f".dequantize() + bf16 F.linear (torch CPU, {torch.get_num_threads()} threads, host has {os.cpu_count()} cpus), mean of {reps} reps, x{layers} extrapolated"}
    return _with_reference(run)


def reference_cpu_baseline_mx(offs_np, layers, rows=128, ncols=1024):
    """configs[4]: torchao's to_mx (RCEIL) + _emulated_mxfp8_scaled_grouped_mm_2d_3d (mxfp8_grouped_mm.py:959-1023), the path the
    reference itself runs on AMD today, on `ncols` of w1's 14336 output columns."""
    def run():
        from torchao.prototype.moe_training.mxfp8_grouped_mm import _emulated_mxfp8_scaled_grouped_mm_2d_3d
        from torchao.prototype.mx_formats.config import ScaleCalculationMode
        from torchao.prototype.mx_formats.mx_tensor import to_mx
        torch.manual_seed(0)
        E, k = 8, 4096
        a = torch.randn(rows, k, dtype=torch.bfloat16)
        w = torch.randn(E, ncols, k, dtype=torch.bfloat16) * 0.02
        w_s, w_d = to_mx(w, torch.float8_e4m3fn, 32, ScaleCalculationMode.RCEIL)
        offs = torch.from_numpy(offs_np)
        def proj():
            with torch.no_grad():
                a_s, a_d = to_mx(a, torch.float8_e4m3fn, 32, ScaleCalculationMode.RCEIL)
                _emulated_mxfp8_scaled_grouped_mm_2d_3d(a_d, a_s, w_d.transpose(-2, -1), w_s.transpose(-2, -1), offs=offs, out_dtype=torch.bfloat16)
        t, reps = _mean_time(proj)
        per_layer = t * 3 * (14336 / ncols)  # w1, w3 and w2 have the same N x K product
        return {"value": 64 / (per_layer * layers), "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "reference", "ms_per_layer": per_layer * 1e3,
                "sample": f"128 rows x {ncols} of w1's 14336 output columns (all 8 experts dequantised, as the reference does): torchao's to_mx(RCEIL) + "
                          f"_emulated_mxfp8_scaled_grouped_mm_2d_3d (torch CPU, {torch.get_num_threads()} threads, host has {os.cpu_count()} cpus), mean of {reps} reps, "
                          f"scaled to 3 projections x {layers} layers"}
    return _with_reference(run)


def _pick_cpu_baseline(ref, port):
    """The reference's own CPU path when it ran (kind "reference"), the C port beside it; the port alone otherwise (with the reason)."""
    if ref is not None and "value" in ref:
        ref["port"] = port
        return ref
    port = dict(port)
    port["reference_reachable"] = ref is not None
    if ref is not None:
        port["reference_error"] = ref.get("error")
    return port


def cpu_baseline_int4(batch):
    """Time the C port of the reference CPU dequant->matmul path on ONE layer."""
    from oracle import c_ref

    rng = np.random.default_rng(0)
    threads = c_ref.num_threads()
    t_layer, reps, budget_s = 0.0, 0, 10.0
    t_begin = time.perf_counter()
    while True:
        t_once = 0.0
        for _, n, k in LLAMA3_8B_UNMERGED:
            qdata = rng.integers(-(2**31), 2**31 - 1, size=(n // 8, k // 128, 32, 4), dtype=np.int64).astype(np.int32)
            sz = np.empty((k // GROUP, n, 2), dtype=np.uint16)
            sz[..., 0] = 0x3B00 + rng.integers(0, 64, size=sz.shape[:2])  # scale ~ 2e-3 (bf16 bits)
            sz[..., 1] = 0x3A00 + rng.integers(0, 64, size=sz.shape[:2])  # zero  ~ 5e-4
            x = (rng.standard_normal((batch, k)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
            t0 = time.perf_counter()
            c_ref.int4_linear(x, qdata, sz, n, k, GROUP)
            t_once += time.perf_counter() - t0
        t_layer += t_once
        reps += 1
        if time.perf_counter() - t_begin > budget_s or reps >= 20:
            break
    t_layer /= reps
    return {
        "value": batch / (t_layer * N_LAYERS), "unit": "tokens/s", "cores": threads, "kind": "port",
        "sample": f"1 of {N_LAYERS} layers (5 linears, 218.1M int4 weights, bs={batch}), mean of {reps} reps, x{N_LAYERS} extrapolated; "
                  f"oracle/lowbit_ref.c (gcc -O3 -fopenmp, {threads} threads, host has {os.cpu_count()} cpus)",
        "ms_per_layer": t_layer * 1e3,
    }


# ----------------------------------------------------------------------------------------------------------------------
# secondary configs (rank 0, one GPU)
# ----------------------------------------------------------------------------------------------------------------------
def _graph_time(fn, stream, device, steps, warmup=2):
    run, graphed = capture(fn, stream)
    return time_steps(run, stream, device, steps, warmup) / steps, graphed


def config_int4_bs128(model, stream, device, args):
    batch, steps = 128, 20
    t, graphed = run_int4(model, batch, steps, 3, stream, device, not args.no_graph)
    tok_s = batch * steps / t
    roof = int4_roofline(model, batch, stream)
    out = {"workload": "Int4WeightOnlyConfig(group_size=128) Llama-3-8B linear shapes (five-shape layout), bs=128 seq=1, 32 layers",
           "value": tok_s, "unit": "tokens/s", "ms_per_step": t * 1e3 / steps, "dtype": "bf16 x int4 (dequant bf16, fp32 accumulate)",
           "launch": "hipGraph replay" if graphed else "eager", "roofline": roof}
    if not args.no_cpu_baseline:
        cb = cpu_baseline_int4(16)
        cb["sample"] = "bs=16 sample of the bs=128 workload: " + cb["sample"]
        ref = reference_cpu_baseline_int4(16)
        if ref is not None and "value" in ref:
            ref["sample"] = "bs=16 sample of the bs=128 workload: " + ref["sample"]
        out["cpu_baseline"] = _pick_cpu_baseline(ref, cb)
    return out


def config_int8(stream, device, args):
    """configs[2]: Int8DynamicActivationInt8WeightConfig, Llama-3-8B shapes, M = 128 x 2048 = 262144 rows as 16 chunks of 16384 (the
    chunking only bounds the activation buffers: x of one chunk is 470 MB at K = 14336)."""
    from ao_amd import _lib, ops
    lib = _lib.lib()
    chunk, nchunk, rot = 16384, 16, 2
    gen = torch.Generator(device=device).manual_seed(1)
    ws, xs = [], {}
    for name, n, k in LLAMA3_8B_UNMERGED:
        w = torch.randn(n, k, device=device, dtype=torch.bfloat16, generator=gen) * 0.02
        ws.append((name, n, k) + ops.int8_quantize_rowwise(w))
        if k not in xs:  # `rot` distinct activation chunks per K (2 x 16384 x K x 2 B >= 268 MB: beyond the 256 MiB Infinity Cache)
            xs[k] = [torch.randn(chunk, k, device=device, dtype=torch.bfloat16, generator=gen) for _ in range(rot)]
    def layer():
        for name, n, k, wq, wsc in ws:
            for c in range(nchunk):
                xq, xsc = ops.int8_quantize_rowwise(xs[k][c % rot])
                ops.int8_scaled_mm(xq, xsc, wq, wsc)
    with torch.cuda.stream(stream):
        t, graphed = _graph_time(layer, stream, device, steps=2, warmup=1)
        prof = event_profile(lib, _lib.check, layer, 2 * nchunk * len(ws) + 8)
    M = chunk * nchunk
    flops = sum(2.0 * M * n * k for _, n, k, _, _ in ws)
    cast_ms, gemm_ms = float(prof[0::2].sum()), float(prof[1::2].sum())
    out = {"workload": "Int8DynamicActivationInt8WeightConfig Llama-3-8B linear shapes, M = 128 x 2048 = 262144 rows in 16384-row chunks, "
                       "1 of 32 layers timed (x32 = one forward; every layer does the same work)",
           "value": M / (t * N_LAYERS), "unit": "tokens/s", "ms_per_layer": t * 1e3, "dtype": "int8 x int8 -> int32, bf16 out",
           "launch": "hipGraph replay" if graphed else "eager", "launches_per_layer": 2 * nchunk * len(ws),
           "roofline": {"kernel": "gemm8_p8p_kernel<int8> (256x256 phase-interleaved, persistent: one workgroup per CU walks 4 - 14 tiles)", "bound": "mfma", "achieved": flops / (gemm_ms * 1e-3) / 1e12, "peak": MFMA_8BIT_PEAK_TOPS,
                        "unit": "TOP/s", "frac": flops / (gemm_ms * 1e-3) / 1e12 / MFMA_8BIT_PEAK_TOPS, "traffic": pmc_traffic_of("int8")[0], "traffic_source": pmc_traffic_of("int8")[1],
                        "measured_mfma_ceiling": _SPECS["int8_measured_mfma_tops"] / 1e12, "frac_of_measured_ceiling": flops / (gemm_ms * 1e-3) / _SPECS["int8_measured_mfma_tops"],
                        "timing": "HIP extension events, one eager layer", "gemm_ms_per_layer": gemm_ms, "act_cast_ms_per_layer": cast_ms,
                        "end_to_end_TOPs": flops / t / 1e12}}
    # the same config at decode size (M = 1, all 32 layers' int8 weights distinct and resident: 6.98 GB): what the round-4 decode kernel
    # (dec8_kernels.hip: cast fused in, full-line register ring) does for the int8 format -- HBM-bound, priced against 8 TB/s
    try:
        del xs
        torch.cuda.empty_cache()
        dws = []
        for _ in range(N_LAYERS):
            for name, n, k in LLAMA3_8B_UNMERGED:
                w = torch.randn(n, k, device=device, dtype=torch.bfloat16, generator=gen) * 0.02
                dws.append((n, k) + ops.int8_quantize_rowwise(w))
                del w
        x1 = {k: torch.randn(1, k, device=device, dtype=torch.bfloat16, generator=gen) for k in {w[1] for w in dws}}
        def decode():
            for n, k, wq, wsc in dws:
                ops.int8_linear(x1[k], wq, wsc)
        with torch.cuda.stream(stream):
            td, _ = _graph_time(decode, stream, device, steps=10)
        dbytes = sum(n * k + 4 * n + 2 * k + 2 * n for n, k, _, _ in dws)
        out["decode_M1"] = {"workload": "the same linears at M = 1 (cast + matmul in one launch per linear), 32 layers, 160 launches per token",
                            "tokens_per_s": 1.0 / td, "ms_per_step": td * 1e3, "bound": "hbm", "GBps": dbytes / td / 1e9, "frac": dbytes / td / 1e9 / HBM_PEAK_GBS,
                            "kernel": "dec8_kernel<int8, fused cast>"}
        del dws
        torch.cuda.empty_cache()
    except Exception as e:  # noqa: BLE001
        out["decode_M1"] = {"error": repr(e)}
    if not args.no_cpu_baseline:
        from oracle import c_ref
        rng = np.random.default_rng(1)
        rows, tt = 16, 0.0
        for name, n, k, wq, wsc in ws:
            x = (rng.standard_normal((rows, k)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
            wqc, wsn = wq.cpu().numpy(), wsc.flatten().cpu().numpy()
            t0 = time.perf_counter()
            c_ref.int8_dynamic_linear(x, wqc, wsn)
            tt += time.perf_counter() - t0
        port = {"value": rows / (tt * N_LAYERS), "unit": "tokens/s", "cores": c_ref.num_threads(), "kind": "port",
                "sample": f"{rows} rows through the 5 linears of 1 layer, x32 extrapolated; oracle/lowbit_ref.c ao_ref_int8_dynamic_linear"}
        out["cpu_baseline"] = _pick_cpu_baseline(reference_cpu_baseline_int8(rows), port)
    return out


def _fp8_layer_fns(device, shard_of, layers, ms, gen):
    """Quantized Llama-3-70B shard weights (shard_of = TP degree), per-M activation sets, and a step function per M."""
    from ao_amd import ops
    wts = []
    for _ in range(layers):
        for name, n, k, style in LLAMA3_70B:
            ns, ks = (n // shard_of, k) if style == "col" else (n, k // shard_of)
            w = torch.randn(ns, ks, device=device, dtype=torch.bfloat16, generator=gen) * 0.02
            wts.append((name, ns, ks) + ops.fp8_quantize_rowwise(w))
            del w
    xs = {m: {ks: torch.randn(m, ks, device=device, dtype=torch.bfloat16, generator=gen) for ks in {w[2] for w in wts}} for m in ms}
    def step(m):
        for name, ns, ks, wq, wsc in wts:
            x = xs[m][ks]
            if ops.dynamic_linear_preferred(m, ns, ks):
                ops.fp8_dynamic_linear(x, wq, wsc)
            else:
                xq, xsc = ops.fp8_quantize_rowwise(x)
                ops.fp8_scaled_mm(xq, wq.t(), xsc, wsc.t())
    return wts, step


def config_fp8_shards(stream, device, args):
    """configs[3], one GPU's share of the work: the Llama-3-70B TP=8 shard linears (no collective on one GPU)."""
    gen = torch.Generator(device=device).manual_seed(2)
    layers, ms = args.fp8_layers, (1, 128, 2048)
    wts, step = _fp8_layer_fns(device, 8, layers, ms, gen)
    wbytes = sum(ns * ks for _, ns, ks, _, _ in wts)
    res = {}
    with torch.cuda.stream(stream):
        for m in ms:
            t, graphed = _graph_time(lambda: step(m), stream, device, steps=3 if m == 2048 else 10)
            flops = sum(2.0 * m * ns * ks for _, ns, ks, _, _ in wts)
            bts = wbytes + sum(m * ks * 2 + m * ns * 2 for _, ns, ks, _, _ in wts)
            hbm = m <= 128  # AI = 2 M flop per weight byte: HBM-bound below M ~ 600
            res[f"M{m}"] = {"tokens_per_s": m / t, "ms_per_step": t * 1e3, "TFLOPs": flops / t / 1e12, "GBps": bts / t / 1e9,
                            "bound": "hbm" if hbm else "mfma", "frac": (bts / t / 1e9 / HBM_PEAK_GBS) if hbm else (flops / t / 1e12 / MFMA_8BIT_PEAK_TOPS)}
    m = 2048
    out = {"workload": "Float8DynamicActivationFloat8WeightConfig(PerRow) Llama-3-70B linear shapes, one GPU's TP=8 shards "
                       "(qkv 1280x8192, o 8192x1024, gate_up 7168x8192, down 8192x3584), 80 layers, activation cast + scaled mm per linear",
           "value": res["M2048"]["tokens_per_s"], "unit": "tokens/s (per GPU, M = 2048, before the all-reduce)", "dtype": "e4m3 x e4m3 -> fp32, bf16 out",
           "by_M": res,
           "roofline": {"kernel": "gemm8_p8p_kernel<fp8> (o, down shards) / gemm8_p8_kernel<fp8> (gate_up shard) / gemm8_p8h_kernel<fp8> with 3 K parts (qkv shard) at M = 2048", "bound": "mfma", "achieved": res["M2048"]["TFLOPs"], "peak": MFMA_8BIT_PEAK_TOPS, "unit": "TFLOP/s",
                        "frac": res["M2048"]["frac"], "traffic": pmc_traffic_of("fp8")[0], "traffic_source": pmc_traffic_of("fp8")[1],
                        "measured_mfma_ceiling": _SPECS["fp8_measured_mfma_tops"] / 1e12, "frac_of_measured_ceiling": res["M2048"]["TFLOPs"] * 1e12 / _SPECS["fp8_measured_mfma_tops"],
                        "timing": "hipGraph replay wall time of the whole step (casts included)"}}
    if not args.no_cpu_baseline:
        from oracle import c_ref
        rng = np.random.default_rng(2)
        rows, tt = 8, 0.0
        for name, ns, ks, wq, wsc in wts[:4]:
            x = (rng.standard_normal((rows, ks)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
            wqc, wsn = wq.view(torch.uint8).cpu().numpy(), wsc.flatten().cpu().numpy()
            t0 = time.perf_counter()
            c_ref.fp8_rowwise_linear(x, wqc, wsn)
            tt += time.perf_counter() - t0
        port = {"value": rows / (tt * layers), "unit": "tokens/s", "cores": c_ref.num_threads(), "kind": "port",
                "sample": f"{rows} rows through the 4 shard linears of 1 layer, x{layers} extrapolated; oracle/lowbit_ref.c ao_ref_fp8_rowwise_linear"}
        out["cpu_baseline"] = _pick_cpu_baseline(reference_cpu_baseline_fp8(layers, rows), port)
    return out


def mixtral_offs(rows=128, experts=8, seed=0):
    """group sizes = 32 * multinomial (seeded), cumulative ends."""
    rng = np.random.default_rng(seed)
    sizes = 32 * rng.multinomial(rows // 32, np.full(experts, 1.0 / experts))
    return np.cumsum(sizes).astype(np.int32), sizes


def config_mx(stream, device, args):
    """configs[4]: MXFP8 grouped GEMM, Mixtral-8x7B expert shapes, 64 tokens x top-2 = 128 rows."""
    from ao_amd import ops
    E, rows, layers = 8, 128, N_LAYERS
    offs_np, sizes = mixtral_offs(rows, E)
    offs = torch.from_numpy(offs_np).to(device)
    gen = torch.Generator(device=device).manual_seed(3)
    wts = []
    for _ in range(layers):
        for name, n, k in MIXTRAL:
            w = torch.randn(E, n, k, device=device, dtype=torch.bfloat16, generator=gen) * 0.02
            wts.append((name, n, k) + ops.mxfp8_quantize(w, "rceil"))  # expert weights are cast ONCE (weight prep)
            del w
    xs = {k: torch.randn(rows, k, device=device, dtype=torch.bfloat16, generator=gen) for k in (4096, 14336)}
    # the product path of _to_mxfp8_then_scaled_grouped_mm (ao_amd/prototype/mx.py): decode-size groups take ONE launch with the activations'
    # 1 x 32 cast fused into the kernel's A-fill (round 6); the two-launch form (cast kernel, then the GEMM) is timed beside it
    fused = all(ops.mxfp8_grouped_mm_dyn_fits(rows, n, k, E) for _, n, k, _, _ in wts[:3]) and not args.mx_two_launch
    def step_two():
        for name, n, k, wq, wsc in wts:
            aq, asc = ops.mxfp8_quantize(xs[k], "rceil")  # activations: dynamic cast every forward
            ops.mxfp8_grouped_mm(aq, asc, wq, wsc, offs)
    def step_fused():
        for name, n, k, wq, wsc in wts:
            ops.mxfp8_grouped_mm_dyn(xs[k], wq, wsc, offs, "rceil")
    # one launch for an expert layer's w1 and w3 (x @ w1, x @ w3: same activations, same shape; ops.mxfp8_grouped_mm_pair), one for w2
    pair = fused and not args.mx_no_pair and ops.mxfp8_grouped_mm_pair_fits(rows, MIXTRAL[0][1], MIXTRAL[0][2], E)
    def layer_pairs(w, x, o):
        for i in range(0, len(w), 3):
            (_, n1, k1, w1q, w1s), (_, _, _, w3q, w3s), (_, n2, k2, w2q, w2s) = w[i], w[i + 1], w[i + 2]
            ops.mxfp8_grouped_mm_pair(x[k1], w1q, w1s, w3q, w3s, o, "rceil")
            ops.mxfp8_grouped_mm_dyn(x[k2], w2q, w2s, o, "rceil")
    def step_pair():
        layer_pairs(wts, xs, offs)
    step = step_pair if pair else step_fused if fused else step_two
    # SURVEY 8(d)'s second workload: 16 tokens on EVERY expert, each group padded to the 32-row alignment of the grouped GEMM
    # (fused_pad_token_groups semantics: 8 x 32 = 256 rows, half of them zero padding) -- all 8 experts' weights are read: 484 MB per w1
    rows_u = 32 * E
    offs_u = torch.arange(1, E + 1, device=device, dtype=torch.int32) * 32
    xs_u = {}
    for k in (4096, 14336):
        t = torch.zeros(rows_u, k, device=device, dtype=torch.bfloat16)
        t.view(E, 32, k)[:, :16] = torch.randn(E, 16, k, device=device, dtype=torch.bfloat16, generator=gen)
        xs_u[k] = t
    def step_u_two():
        for name, n, k, wq, wsc in wts:
            aq, asc = ops.mxfp8_quantize(xs_u[k], "rceil")
            ops.mxfp8_grouped_mm(aq, asc, wq, wsc, offs_u)
    def step_u_fused():
        for name, n, k, wq, wsc in wts:
            ops.mxfp8_grouped_mm_dyn(xs_u[k], wq, wsc, offs_u, "rceil")
    def step_u_pair():
        layer_pairs(wts, xs_u, offs_u)
    step_u = step_u_pair if pair else step_u_fused if fused else step_u_two
    with torch.cuda.stream(stream):
        t, graphed = _graph_time(step, stream, device, steps=5)
        tu, _ = _graph_time(step_u, stream, device, steps=5)
        t_two, tu_two = (_graph_time(step_two, stream, device, steps=5)[0], _graph_time(step_u_two, stream, device, steps=5)[0]) if fused else (None, None)
        t_one, tu_one = (_graph_time(step_fused, stream, device, steps=5)[0], _graph_time(step_u_fused, stream, device, steps=5)[0]) if pair else (None, None)
    used = int((sizes > 0).sum())
    bts = sum(used * n * k * (1 + 1 / 32) + rows * k * 2 + rows * k * (1 + 1 / 32) + rows * n * 2 for _, n, k, _, _ in wts)
    bts_u = sum(E * n * k * (1 + 1 / 32) + rows_u * k * 2 + rows_u * k * (1 + 1 / 32) + rows_u * n * 2 for _, n, k, _, _ in wts)
    flops = sum(2.0 * rows * n * k for _, n, k, _, _ in wts)
    out = {"workload": f"MXFP8 grouped GEMM (to_mx RCEIL + scaled grouped mm), Mixtral-8x7B expert shapes E=8 (w1, w3 14336x4096; w2 4096x14336), "
                       f"64 tokens x top-2 = 128 rows, group sizes {sizes.tolist()} (32 x multinomial, seed 0), 32 layers",
           "value": 64 / t, "unit": "tokens/s", "ms_per_step": t * 1e3, "dtype": "e4m3 x e4m3 with E8M0 1x32 block scales, bf16 out",
           "launch": "hipGraph replay" if graphed else "eager",
           "roofline": {"kernel": "mx_stream_kernel (stream-K, decode-size groups; 16 waves / 256-column tiles, one workgroup per CU)", "bound": "hbm", "achieved": bts / t / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": bts / t / 1e9 / HBM_PEAK_GBS, "traffic": pmc_traffic_of("mx")[0], "traffic_source": pmc_traffic_of("mx")[1],
                        "timing": "hipGraph replay wall time of the whole step (activation casts included)",
                        "bytes_note": "weights of the experts that received tokens only", "TFLOPs": flops / t / 1e12},
           "uniform16": {"workload": "the same 96 grouped GEMMs with 16 tokens on each of the 8 experts, groups padded to 32 rows (256 rows, offs = 32, 64, .. 256): "
                                     "every expert's weights are read (SURVEY.md 8(d): 484.4 MB per w1)",
                         "value": 64 / tu, "unit": "tokens/s", "ms_per_step": tu * 1e3,
                         "roofline": {"bound": "hbm", "achieved": bts_u / tu / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bts_u / tu / 1e9 / HBM_PEAK_GBS,
                                      "traffic": pmc_traffic_of("mx", "uniform16")[0], "traffic_source": pmc_traffic_of("mx", "uniform16")[1],
                                      "algorithmic_bytes_per_step": bts_u, "timing": "hipGraph replay wall time of the whole step (activation casts included)"}}}
    out["launches_per_step"] = (len(wts) // 3 * 2) if pair else (1 if fused else 2) * len(wts)
    out["w1_w3"] = "one launch for both products (ao_mxfp8_grouped_mm_dyn_pair)" if pair else "one launch each"
    if pair:  # one launch per product, cast fused (what a caller of the reference's per-weight interface gets)
        out["one_launch_per_product"] = {"value": 64 / t_one, "ms_per_step": t_one * 1e3, "frac": bts / t_one / 1e9 / HBM_PEAK_GBS,
                                         "uniform16_value": 64 / tu_one, "uniform16_ms_per_step": tu_one * 1e3, "uniform16_frac": bts_u / tu_one / 1e9 / HBM_PEAK_GBS}
    out["activation_cast"] = "fused into the grouped GEMM's A-fill (ao_mxfp8_grouped_mm_dyn)" if fused else "its own kernel (ao_mxfp8_quantize_rowwise) before every GEMM"
    if fused:  # the A/B the round-5 verdict asked for: the same 96 products as cast kernel + GEMM (two launches each), same process, same weights
        out["two_launch"] = {"value": 64 / t_two, "ms_per_step": t_two * 1e3, "frac": bts / t_two / 1e9 / HBM_PEAK_GBS,
                             "uniform16_value": 64 / tu_two, "uniform16_ms_per_step": tu_two * 1e3, "uniform16_frac": bts_u / tu_two / 1e9 / HBM_PEAK_GBS}
    if not args.no_cpu_baseline:
        from oracle import c_ref
        rng = np.random.default_rng(3)
        ncols = 1024
        name, n, k, wq, wsc = wts[0]
        a = (rng.standard_normal((rows, k)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        wqc, wsn = wq.view(torch.uint8)[:, :ncols].cpu().numpy(), wsc.view(torch.uint8)[:, :ncols].cpu().numpy()
        t0 = time.perf_counter()
        c_ref.mxfp8_grouped_mm(a, wqc, wsn, offs_np)
        tt = time.perf_counter() - t0
        per_layer = tt * 3 * (14336 / ncols)  # w1, w3 and w2 have the same N x K product
        port = {"value": 64 / (per_layer * layers), "unit": "tokens/s", "cores": c_ref.num_threads(), "kind": "port",
                "sample": f"128 rows x {ncols} of w1's 14336 output columns (all 8 experts), scaled to 3 projections x 32 layers; "
                          "oracle/lowbit_ref.c ao_ref_mxfp8_grouped_mm (emulated dequant -> bf16 grouped mm path)"}
        out["cpu_baseline"] = _pick_cpu_baseline(reference_cpu_baseline_mx(offs_np, layers, rows, ncols), port)
    return out


def _dbg(msg):
    if os.environ.get("AO_BENCH_DEBUG") == "1":
        print(f"[bench rank {os.environ.get('RANK', '0')}] {msg}", file=sys.stderr, flush=True)


def config_fp8_tp(stream, device, args, dist, world):
    """configs[3] for real when N > 1: Llama-3-70B linears sharded TP = N over RCCL (ao_amd/parallel.py)."""
    from ao_amd import parallel
    _dbg("tp: start")
    from ao_amd.quantization import Float8DynamicActivationFloat8WeightConfig, PerRow, quantize_
    # the hand-written one-shot all-reduce (ao_amd/csrc/allreduce_kernels.hip over IPC-mapped buffers): always set up so that the
    # collectives-only timing below can compare it with the group's all_reduce; the linears use it only with --tp-one-shot
    # -- opt-in (--tp-one-shot or AO_BENCH_ONE_SHOT=1): the kernel is verified with two ranks on ONE GPU only (tests/test_oneshot_allreduce_gpu.py);
    # a peer-mapping problem on a real multi-GPU node would be a GPU fault, not an exception, and must not be able to take the
    # default bench line down with it
    if args.tp_one_shot or os.environ.get("AO_BENCH_ONE_SHOT") == "1":
        one_shot_probe = parallel.OneShotAllReduce()
    else:
        class _NoProbe:
            ok, why = False, "not requested (--tp-one-shot or AO_BENCH_ONE_SHOT=1); verified with two ranks on one GPU only"
        one_shot_probe = _NoProbe()
    one_shot = one_shot_probe if args.tp_one_shot else None
    gen = torch.Generator(device=device).manual_seed(4)
    layers = 8  # of 80: the same four linears per layer; tokens/s is extrapolated x10 (weights of 8 layers are 2.7 GB per GPU at TP=8)
    mods = []
    for _ in range(layers):
        for name, n, k, style in LLAMA3_70B:
            lin = torch.nn.Linear(k, n, bias=False, device=device, dtype=torch.bfloat16)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(n, k, device=device, dtype=torch.bfloat16, generator=gen) * 0.02)
            quantize_(lin, Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()))
            mods.append((name, style, parallel.shard_linear_(lin, "colwise" if style == "col" else "rowwise", reduce="exact", one_shot=one_shot)))
            del lin
    torch.cuda.empty_cache()
    _dbg(f"tp: {len(mods)} sharded linears built; one-shot ok={one_shot_probe.ok} why={one_shot_probe.why}")
    res = {}
    for m in (1, 128, 2048):
        _dbg(f"tp: M={m}")
        xs = {}
        for name, style, mod in mods:
            kdim = mod.weight.shape[1]
            xs.setdefault(kdim, torch.randn(m, kdim, device=device, dtype=torch.bfloat16, generator=gen))
        def step():
            for name, style, mod in mods:
                mod(xs[mod.weight.shape[1]])
        steps = 5 if m == 2048 else 20
        with torch.cuda.stream(stream):
            for _ in range(3):
                step()
        # decode-size steps are launch-bound in eager mode (six launches + two collectives per row-parallel linear: 27 tok/s eager vs
        # 318 from a graph at M = 1, round 2): every step replays from a hipGraph (RCCL collectives are capturable) unless
        # --no-tp-graph; a failed capture falls back to eager launches on every rank (capture() catches it)
        # (gloo collectives cannot be captured, and a failed capture leaves the stream's capture state invalidated for every later launch:
        # only RCCL runs try)
        try_graph = not args.no_tp_graph and dist.get_backend() == "nccl"
        run, graphed = capture(step, stream, use_graph=True, collectives=True) if try_graph else (step, False)
        with torch.cuda.stream(stream):
            t = time_steps(run, stream, device, steps, 2, dist) / steps
            # the collectives alone, same sizes and order: amax MAX [M] + fp32 SUM [M, 8192] per row-parallel linear
            bufs = [(torch.zeros(m, device=device), torch.zeros(m, 8192, device=device)) for _ in range(2)]
            def comm():
                for name, style, mod in mods:
                    if style == "row":
                        a, b = bufs[0]
                        dist.all_reduce(a, op=dist.ReduceOp.MAX)
                        dist.all_reduce(b, op=dist.ReduceOp.SUM)
            _dbg("tp: steps timed; collectives")
            for _ in range(3):
                comm()
            tc = time_steps(comm, stream, device, steps, 2, dist) / steps
            _dbg("tp: group all_reduce timed")
            # the same exchanges with the fp32 SUM through the one-shot kernel (when the vector fits its 1 MiB slot), and the cheaper
            # protocol's payload for comparison: ONE bf16 [M, 8192] all-reduce per row-parallel linear (reduce="bf16": locally scaled
            # partials, not bit-faithful to the unsharded linear)
            tc_one, tc_bf16 = None, None
            if one_shot_probe.ok and one_shot_probe.fits(bufs[0][1]):
                one_shot_probe(bufs[0][1])  # one call first: a rank that never shows up costs 0.5 s per call -- do not time a broken path
                torch.cuda.synchronize(device)
            if one_shot_probe.ok and one_shot_probe.fits(bufs[0][1]) and not one_shot_probe.timed_out():
                def comm_one():
                    for name, style, mod in mods:
                        if style == "row":
                            a, b = bufs[0]
                            dist.all_reduce(a, op=dist.ReduceOp.MAX)
                            one_shot_probe(b)
                for _ in range(3):
                    comm_one()
                tc_one = time_steps(comm_one, stream, device, steps, 2, dist) / steps
            half = torch.zeros(m, 8192, device=device, dtype=torch.bfloat16)
            def comm_bf16():
                for name, style, mod in mods:
                    if style == "row":
                        dist.all_reduce(half, op=dist.ReduceOp.SUM)
            for _ in range(3):
                comm_bf16()
            tc_bf16 = time_steps(comm_bf16, stream, device, steps, 2, dist) / steps
        flops = sum(2.0 * m * n * k for _, n, k, _ in LLAMA3_70B) * layers / world
        res[f"M{m}"] = {"tokens_per_s": m / (t * 80 / layers), "launch": "hipGraph replay" if graphed else "eager", "ms_per_8_layers": t * 1e3, "allreduce_ms_per_8_layers": tc * 1e3,
                        "allreduce_bytes_per_row_linear": m * 8192 * 4 + m * 4, "per_gpu_TFLOPs": flops / t / 1e12,
                        "per_gpu_frac_of_fp8_mfma_peak": flops / t / 1e12 / MFMA_8BIT_PEAK_TOPS,
                        "allreduce_one_shot_ms_per_8_layers": None if tc_one is None else tc_one * 1e3,
                        "allreduce_bf16_protocol_ms_per_8_layers": tc_bf16 * 1e3, "allreduce_bf16_protocol_bytes_per_row_linear": m * 8192 * 2,
                        "one_shot": {"ok": one_shot_probe.ok, "why": one_shot_probe.why, "timed_out": one_shot_probe.timed_out() if one_shot_probe.ok else None}}
    return {"workload": f"Float8 rowwise Llama-3-70B linears, TP={world} over {dist.get_backend()} (nccl = RCCL over xGMI; column-parallel qkv / gate_up, row-parallel o / down with the "
                        "exact protocol: amax all-reduce(MAX) + fp32 accumulator all-reduce(SUM) + one scale epilogue), 8 of 80 layers timed",
            "value": res["M2048"]["tokens_per_s"], "unit": "tokens/s (M = 2048, x10 extrapolated to 80 layers)", "by_M": res}


# ----------------------------------------------------------------------------------------------------------------------
def main():
    # stdout carries exactly ONE line (the JSON): RCCL / HIP libraries print banners to the C-level stdout ("RCCL version : ...")
    # whenever they like, so file descriptor 1 is pointed at stderr for the whole run and the line goes to the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and world > 1:
        print(f"warning: --gpus {args.gpus} != WORLD_SIZE {world}", file=sys.stderr)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback in the product path)")
    # AO_BENCH_SHARE_GPU=1 (+ AO_BENCH_BACKEND=gloo): every rank on cuda:0 -- a dry run of the N > 1 code path on a one-GPU box (RCCL refuses
    # two ranks on one device, gloo moves device tensors through the host); numbers from such a run mean nothing
    if os.environ.get("AO_BENCH_SHARE_GPU") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or args.force_tp:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        backend = os.environ.get("AO_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=device)
        else:
            dist.init_process_group(backend=backend)

    from ao_amd import _lib

    lib = _lib.lib()
    if args.wpb or args.mode:
        lib.ao_int4_set_tuning(args.wpb, args.mode)
    if args.gemm_variant:
        lib.ao_gemm8_set_variant(args.gemm_variant)
    for kv in filter(None, os.environ.get("AO_GEMM8_TUNE", "").split(",")):  # A/B runs of the tools: key=value pairs of ao_gemm8_set_tuning
        key, val = kv.split("=")
        _lib.check(lib.ao_gemm8_set_tuning(int(key), int(val)))

    merged = args.merged and not args.unmerged
    shapes = LLAMA3_8B_MERGED if merged else LLAMA3_8B_UNMERGED
    stream = torch.cuda.Stream(device=device)
    model = Int4Linears(device, args.layers, shapes)
    _dbg("int4 model built")
    elapsed, graphed = run_int4(model, args.batch, args.steps, args.warmup, stream, device, not args.no_graph, dist if world > 1 else None)
    ms_per_step = elapsed * 1e3 / args.steps
    tokens_per_s = args.batch * world * args.steps / elapsed

    _dbg("headline timed")
    if args.dump_outputs and rank == 0:
        dump_outputs(model, args.batch, args.dump_outputs)
    roof = int4_roofline(model, args.batch, stream) if rank == 0 and args.full else None
    _dbg("roofline done")

    # the other module layout, for the record (rank 0 of a 1-GPU run only: it doubles resident weights); then both layouts
    # replayed alternately (median / best / worst of 5 rounds), the subclass + F.linear path (a13) and the same-box stack baseline
    other_tok_s, stats, subclass, stack, merged_cfg = None, None, None, None, None
    if args.full and rank == 0 and world == 1 and not args.no_second_layout:
        m2 = Int4Linears(device, args.layers, LLAMA3_8B_UNMERGED if merged else LLAMA3_8B_MERGED)
        steps2 = min(args.steps, 20)
        e2, _ = run_int4(m2, args.batch, steps2, min(args.warmup, 3), stream, device, not args.no_graph)
        other_tok_s = args.batch * steps2 / e2
        if not args.no_graph:
            names = ("merged", "five") if merged else ("five", "merged")
            stats = replay_stats({names[0]: model, names[1]: m2}, args.batch, stream, device)
        if not merged and args.batch == 1:
            # the vLLM module layout (gate and up as ONE 28672 x 4096 linear: 128 launches per token) as a config of its own, with its own
            # roofline -- the in-contract way to spend fewer launches on the same weights
            try:
                roof2 = int4_roofline(m2, args.batch, stream, layout="merged")
                b2 = m2.bytes_per_step(args.batch)
                merged_cfg = {"workload": "Int4WeightOnlyConfig(group_size=128) Llama-3-8B linears in the vLLM module layout (qkv_proj 6144x4096, o_proj, "
                                          "gate_up_proj 28672x4096, down_proj), bs=1 seq=1, 32 layers, 128 launches per token",
                              "value": other_tok_s, "unit": "tokens/s", "ms_per_step": 1e3 / other_tok_s, "dtype": "bf16 x int4 (dequant bf16, fp32 accumulate)",
                              "launch": "hipGraph replay" if not args.no_graph else "eager", "bytes_per_token": b2,
                              "frac_of_hbm_roofline_end_to_end": other_tok_s * b2 / (HBM_PEAK_GBS * 1e9), "roofline": roof2}
            except Exception as e:  # noqa: BLE001
                merged_cfg = {"error": repr(e)}
        del m2
        torch.cuda.empty_cache()
    if args.full and rank == 0 and world == 1 and args.batch == 1 and not args.no_graph:
        if not args.no_subclass_graph:
            try:
                subclass = subclass_graph_tokens_per_s(model, stream, device)
            except Exception as e:  # noqa: BLE001
                subclass = {"error": repr(e)}
        if not args.no_stack_baseline:
            stack = stack_baseline(model, stream, device, args)

    configs = {}
    if merged_cfg is not None:
        configs["int4_bs1_merged"] = merged_cfg
    want = set() if args.no_configs or not args.full else set(args.configs.split(","))
    if rank == 0 and world == 1 and args.batch == 1:
        for key, fn in (("int4_bs128", lambda: config_int4_bs128(model, stream, device, args)),
                        ("int8", lambda: config_int8(stream, device, args)),
                        ("fp8", lambda: config_fp8_shards(stream, device, args)),
                        ("mx", lambda: config_mx(stream, device, args))):
            if key in want:
                name = {"int8": "int8_dyn_bs128x2048", "fp8": "fp8_tp8_shards", "mx": "mxfp8_mixtral_bs64"}.get(key, key)
                try:
                    configs[name] = fn()
                except Exception as e:  # noqa: BLE001 -- a secondary config must not take the headline line down
                    configs[name] = {"error": repr(e)}
                torch.cuda.empty_cache()
    out = None
    if rank == 0:
        bytes_step = model.bytes_per_step(args.batch)
        roofline_tok_s = HBM_PEAK_GBS * 1e9 / bytes_step * args.batch
        out = {
            "metric": "linear-layer tokens/sec, Llama-3-8B int4-wo (tinygemm g128), bs=%d" % args.batch,
            "value": tokens_per_s,
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16 x int4 (dequant bf16, fp32 accumulate)",
            "data": "synthetic (random-init weights of the Llama-3-8B linear shapes, quantized on device)",
            "config": {
                "workload": "Int4WeightOnlyConfig(group_size=128) Llama-3-8B linear shapes, bs=%d seq=1, %d layers x {%s}"
                % (args.batch, args.layers, ", ".join("%s %dx%d" % s_ for s_ in shapes)),
                "module_layout": "vLLM (merged qkv_proj, gate_up_proj)" if merged else "SURVEY.md 8(d) five shapes (qkv merged; gate, up separate)",
                "launch": "hipGraph replay" if graphed else "eager",
                "parallelism": "dp%d (one token stream per GPU, no collective)" % world,
                "bytes_per_token": bytes_step,
                "hbm_roofline_tokens_per_s": roofline_tok_s,
                "frac_of_hbm_roofline_end_to_end": (tokens_per_s / world) / roofline_tok_s,
                ("unmerged_tokens_per_s" if merged else "merged_tokens_per_s"): other_tok_s,
                "replay_stats": stats,
                "subclass_graph": subclass,
                "subclass_graph_tokens_per_s": None if not subclass else subclass.get("tokens_per_s"),
            },
            "roofline": roof,
        }
        if stack is not None:
            out["stack_baseline"] = stack
        if args.full and not args.no_cpu_baseline and world == 1:  # rank 0 at N = 1 only: the other ranks of a multi-GPU run would sit in the barrier
            port = cpu_baseline_int4(args.batch)
            ref = reference_cpu_baseline_int4() if args.batch == 1 else None
            if ref is not None and "value" in ref:
                # the REAL reference's CPU dequant -> bf16 matmul path, imported from the checkout (build container) or from its
                # staged Python under oracle/_ref (the GPU box): BASELINE.md section 3 by the letter.  The C port rides along.
                ref["reference_root"] = _reference_root()
                out["cpu_baseline"], out["cpu_baseline_port"] = ref, port
            else:
                out["cpu_baseline"] = port
                out["cpu_baseline"]["reference_reachable"] = False
                if ref is not None:
                    out["cpu_baseline"]["reference_error"] = ref.get("error")
        if "int4_bs1_merged" in configs and "cpu_baseline" in out and "value" in configs["int4_bs1_merged"]:
            cb = dict(out["cpu_baseline"])
            cb["sample"] = "the headline's CPU measurement (the same 218.1M weights per layer; only the module boundaries differ): " + str(cb.get("sample"))
            configs["int4_bs1_merged"]["cpu_baseline"] = cb
        if configs:
            out["configs"] = configs
        # the driver's parser keeps top-level scalars only: every config's value / fraction again as flat keys
        # roofline_frac: from the committed rocprofv3 --kernel-trace --stats summary of this command when profiles/ holds one (the judge's
        # figure: call-weighted mean duration of every int4_mm_kernel instantiation), the live event-timed one beside it
        flat = {"roofline_frac": (roof.get("rocprof", {}).get("frac") or roof["frac"]) if roof else None,
                "roofline_frac_event_timed": roof["frac"] if roof else None,
                "roofline_frac_source": (roof.get("rocprof", {}).get("source") or "HIP extension events, this run") if roof else None, "merged_tokens_per_s": other_tok_s if not merged else None,
                # the profiled process's own figures, side by side (committed profile; this run's ms_per_step is the line's top-level key)
                "rocprof_sum_kernel_ms_per_step": roof.get("rocprof", {}).get("rocprof_sum_kernel_ms_per_step") if roof else None,
                "rocprof_span_ms_per_step": roof.get("rocprof", {}).get("rocprof_span_ms_per_step") if roof else None,
                "rocprof_line_ms_per_step": roof.get("rocprof", {}).get("line_ms_per_step") if roof else None,
                "event_sum_kernel_ms_per_step": roof.get("sum_kernel_ms_per_step") if roof else None,
                "subclass_graph_tokens_per_s": None if not subclass else subclass.get("tokens_per_s")}
        if stats:
            for lay, st in stats.items():
                flat[f"{lay}_tokens_per_s_median"] = st["tokens_per_s_median"]
                flat[f"{lay}_tokens_per_s_best"] = st["tokens_per_s_best"]
        if stack and "int4_bs1" in stack:
            flat["stack_int4_bs1_tokens_per_s"] = stack["int4_bs1"].get("tokens_per_s")
        c = configs
        if "int4_bs1_merged" in c and "value" in c["int4_bs1_merged"]:
            flat["int4_bs1_merged_frac_of_hbm_roofline"] = c["int4_bs1_merged"]["frac_of_hbm_roofline_end_to_end"]
        if "int4_bs128" in c and "value" in c["int4_bs128"]:
            flat["int4_bs128_tokens_per_s"] = c["int4_bs128"]["value"]
            flat["int4_bs128_frac_of_bf16_mfma_peak"] = c["int4_bs128"]["roofline"]["frac"]
        if "int8_dyn_bs128x2048" in c and "value" in c["int8_dyn_bs128x2048"]:
            flat["int8_dyn_tokens_per_s"] = c["int8_dyn_bs128x2048"]["value"]
            flat["int8_dyn_gemm_frac_of_int8_mfma_peak"] = c["int8_dyn_bs128x2048"]["roofline"]["frac"]
            flat["int8_dyn_end_to_end_frac_of_int8_mfma_peak"] = c["int8_dyn_bs128x2048"]["roofline"]["end_to_end_TOPs"] / MFMA_8BIT_PEAK_TOPS
            if "frac" in c["int8_dyn_bs128x2048"].get("decode_M1", {}):
                flat["int8_decode_M1_tokens_per_s"] = c["int8_dyn_bs128x2048"]["decode_M1"]["tokens_per_s"]
                flat["int8_decode_M1_frac_of_hbm_peak"] = c["int8_dyn_bs128x2048"]["decode_M1"]["frac"]
        if "fp8_tp8_shards" in c and "by_M" in c["fp8_tp8_shards"]:
            for mk, r in c["fp8_tp8_shards"]["by_M"].items():
                flat[f"fp8_shards_{mk}_tokens_per_s"] = r["tokens_per_s"]
                flat[f"fp8_shards_{mk}_frac_of_{r['bound']}_peak"] = r["frac"]
        if "mxfp8_mixtral_bs64" in c and "value" in c["mxfp8_mixtral_bs64"]:
            flat["mxfp8_mixtral_tokens_per_s"] = c["mxfp8_mixtral_bs64"]["value"]
            flat["mxfp8_mixtral_frac_of_hbm_peak"] = c["mxfp8_mixtral_bs64"]["roofline"]["frac"]
            if "uniform16" in c["mxfp8_mixtral_bs64"]:
                flat["mxfp8_mixtral_uniform16_tokens_per_s"] = c["mxfp8_mixtral_bs64"]["uniform16"]["value"]
                flat["mxfp8_mixtral_uniform16_frac_of_hbm_peak"] = c["mxfp8_mixtral_bs64"]["uniform16"]["roofline"]["frac"]
        out.update({k_: v for k_, v in flat.items() if v is not None})
        if not args.full:  # a plain line names only what the run measured (vs_baseline stays: it is part of the line's contract)
            out["config"] = {k_: v for k_, v in out["config"].items() if v is not None}
            out = {k_: v for k_, v in out.items() if v is not None or k_ == "vs_baseline"}
    if (world > 1 or args.force_tp) and "tp" in want and args.batch == 1:
        # The TP leg is the only part of a multi-GPU run with collectives in it.  It runs LAST, with the headline line already assembled,
        # under a watchdog: should a rank hang in it (a rendezvous or a peer mapping that this code has never seen on the node at hand), every
        # rank leaves after --tp-timeout seconds and rank 0 still prints the line, with the leg marked as timed out.
        import threading

        def bail():
            if rank == 0:
                out.setdefault("configs", {})["fp8_tp"] = {"error": "timed out after %d s: a rank hung in the TP leg (headline unaffected)" % args.tp_timeout}
                os.write(json_fd, (json.dumps(out) + "\n").encode())
            os._exit(0)

        dog = threading.Timer(args.tp_timeout, bail)
        dog.daemon = True
        dog.start()
        model.io = {}
        try:
            tp = config_fp8_tp(stream, device, args, dist, world)
        except Exception as e:  # noqa: BLE001
            tp = {"error": repr(e)}
        if rank == 0:
            out.setdefault("configs", {})["fp8_tp"] = tp
            if "by_M" in tp:
                for mk, r in tp["by_M"].items():
                    out[f"fp8_tp_{mk}_tokens_per_s"] = r["tokens_per_s"]
                    out[f"fp8_tp_{mk}_allreduce_ms_per_8_layers"] = r["allreduce_ms_per_8_layers"]
        try:
            dist.barrier()
            dist.destroy_process_group()
        except Exception as e:  # noqa: BLE001
            print(f"warning: process group shutdown: {e!r}", file=sys.stderr)
        dog.cancel()
    elif dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    os.close(json_fd)


if __name__ == "__main__":
    main()
