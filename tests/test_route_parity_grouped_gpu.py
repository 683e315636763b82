"""Every grouped GEMM route (tests/route_cases.py GROUPED_CASES) and the forced-only grouped forms against a float64
reference, through the C ABI, on guarded and poisoned output buffers (tests/_parity.py).

Operands as in test_route_parity_gpu.py: every finite e4m3 code, fp32 row / column scales 2^U(-10, 4) (rowwise fp8), E8M0 block scales
127 + U{-12..12} per (row, 32-block), and for the fused-cast entries bf16 activations with (row, block) magnitudes 2^U(-8, 8) and one
all-zero block, cast by the oracle (oracle/mx_ref.to_mx) under the case's scaling mode.  The group sizes are the case's pattern
(route_cases.group_sizes): the rows past offs[-1] must keep the sentinel.  The pair forms draw w1 and w3 independently and check each
output against its own reference.  Every case launches twice into differently poisoned buffers and must give the same bits; on the
stream-K form another grouped stream-K shape and the smallest dense split-K case run in between.
"""
import numpy as np
import pytest
import torch

import _parity
import route_cases as rc
from ao_amd import _lib
from test_route_parity_gpu import _SPLIT, K_FLOOR_E4M3_MX, Draw, Run, _e4m3, _ptr, mx_cast, mx_dequant

# The floor on K of the bound (tests/_parity.py) and the equal fractions, measured on every grouped case with the operands below: the
# worst element needs max(K, floor) >= 786 on rowwise fp8 (at K = 128; 139 at 2048), so 896; >= 1286 on MX (at K = 128; 632 at 2048,
# 42 at 14336), the scaled MFMA's floor of the dense MX cases (test_route_parity_gpu.K_FLOOR_E4M3_MX).  Equal 0.964 at least on both.
K_FLOOR_GROUPED = {"fp8": 896, "mx": K_FLOOR_E4M3_MX}
EQUAL_GROUPED_FP8 = 0.96
EQUAL_GROUPED_MX = 0.96
_MODES = {"floor": 0, "rceil": 1}  # AO_MX_SCALE_*


def _shifted(t, aligned, nbytes=4):
    """t itself, or a copy of it `nbytes` past a 16-byte-aligned base."""
    if aligned:
        return t
    es = t.element_size()
    buf = torch.empty(t.numel() + 16 // es + nbytes // es, dtype=t.dtype, device=t.device)
    off = (-buf.data_ptr() // es) % (16 // es) + nbytes // es
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == nbytes
    return out


class GRun:
    """Operands of a grouped case, its launch into one (two for the pair forms) guarded buffer(s), and the references."""

    def __init__(self, case, seed, dev, sizes=None):
        self.case, self.dev = case, dev
        _, entry, M, N, K, E, aligned, offs, mode = case
        d = Draw(seed, dev)
        self.sizes = sizes if sizes is not None else rc.group_sizes(E, M, offs)
        self.offs = torch.tensor(np.cumsum(self.sizes), dtype=torch.int32, device=dev)
        self.written = int(sum(self.sizes))
        self.pair = entry in rc.PAIRS
        if entry == "fp8":
            self.a, self.sa = d.fp8(M, K), d.scales(M)
            self.b, self.sb = [d.fp8(E, N, K)], [d.scales(E * N).view(E, N)]
            A = _e4m3(self.a)
            deq = lambda e, i: _e4m3(self.b[i][e])  # noqa: E731
            sa64 = self.sa.double()[:, None]
        else:
            if entry in rc.FUSED:
                self.x = d.mx_act(M, K)
                self.a, self.sa = mx_cast(self.x, "e4m3", mode)
            else:
                self.a, self.sa = d.fp8(M, K), d.e8m0(M, K // 32)
            nb = 2 if self.pair else 1
            self.b, self.sb = zip(*[(d.fp8(E, N, K), d.e8m0(E, N, K // 32)) for _ in range(nb)])
            A = mx_dequant(self.a, self.sa, "e4m3")
            deq = lambda e, i: mx_dequant(self.b[i][e], self.sb[i][e], "e4m3")  # noqa: E731
            sa64 = None
        self.refs = []
        for i in range(len(self.b)):
            ref = torch.zeros(M, N, dtype=torch.float64, device=dev)
            S = torch.zeros_like(ref)
            lo = 0
            for e, n in enumerate(self.sizes):
                if n:
                    W = deq(e, i)
                    ref[lo:lo + n] = A[lo:lo + n] @ W.T
                    S[lo:lo + n] = A[lo:lo + n].abs() @ W.abs().T
                    if sa64 is not None:
                        sc = sa64[lo:lo + n] * self.sb[i][e].double()[None, :]
                        ref[lo:lo + n] *= sc
                        S[lo:lo + n] *= sc
                lo += n
            kw = dict(ref64=ref, S=S, K=K, written_rows=self.written)
            if entry == "fp8":
                kw.update(equal=EQUAL_GROUPED_FP8, k_floor=K_FLOOR_GROUPED["fp8"])
            else:
                kw.update(equal=EQUAL_GROUPED_MX, k_floor=K_FLOOR_GROUPED["mx"])
            self.refs.append(kw)
        # what the route's aligned flag covers, moved off 16 bytes by 4: the scales (aligned cases: the tensors as allocated)
        self.sa_arg = _shifted(self.sa, aligned)
        self.sb_arg = [_shifted(t, aligned) for t in self.sb]

    def buffers(self):
        return [_parity.Guarded(self.case.M, self.case.N, torch.bfloat16, self.dev) for _ in self.refs]

    def launch(self, bufs, sync=True):
        lib = _lib.lib()
        _, entry, M, N, K, E, _, _, mode = self.case
        s = torch.cuda.current_stream().cuda_stream
        y = [b.out.data_ptr() for b in bufs]
        b, sb, offs = [t.data_ptr() for t in self.b], [t.data_ptr() for t in self.sb_arg], self.offs.data_ptr()
        if entry == "fp8":
            rc_ = lib.ao_fp8_grouped_mm(_ptr(self.a), _ptr(self.sa_arg), b[0], sb[0], offs, y[0], M, N, K, E, s)
        elif entry == "mx":
            rc_ = lib.ao_mxfp8_grouped_mm(_ptr(self.a), _ptr(self.sa_arg), b[0], sb[0], offs, y[0], M, N, K, E, s)
        elif entry == "mx_dyn":
            rc_ = lib.ao_mxfp8_grouped_mm_dyn(_ptr(self.x), b[0], sb[0], offs, y[0], M, N, K, E, _MODES[mode], s)
        elif entry == "mx_dyn_pair":
            rc_ = lib.ao_mxfp8_grouped_mm_dyn_pair(_ptr(self.x), b[0], sb[0], b[1], sb[1], offs, y[0], y[1], M, N, K, E, _MODES[mode], s)
        else:
            rc_ = lib.ao_mxfp8_grouped_mm_pair(_ptr(self.a), _ptr(self.sa_arg), b[0], sb[0], b[1], sb[1], offs, y[0], y[1], M, N, K, E, s)
        _lib.check(rc_)
        if sync:
            torch.cuda.synchronize()

    def check(self, bufs, route=None):
        for i, (buf, kw) in enumerate(zip(bufs, self.refs)):
            msgs = _parity.problems(buf, route=route, **kw)
            assert not msgs, ("output %d: " % (2 * i + 1) if self.pair else "") + "; ".join(msgs)


def _relaunch_same_bits(run, bufs, route, between=()):
    """A second launch into buffers poisoned with the other sentinel, after the launches in `between`, gives the same bits."""
    first = [b.bits().clone() for b in bufs]
    for launch in between:
        launch()
    for b in bufs:
        b.poison(_parity.SENTINEL2)
    run.launch(bufs)
    for i, (b, f) in enumerate(zip(bufs, first)):
        assert not b.guard_problems(), b.guard_problems()
        # the rows the kernel must not write hold the sentinel of each launch: compare the written rows
        same = b.bits()[:run.written] == f[:run.written]
        if not bool(same.all()):
            r, c = (int(v) for v in torch.nonzero(~same)[0])
            raise AssertionError("output %d: second launch differs in %d elements, first at row %d, column %d%s"
                                 % (i, int((~same).sum()), r, c, _parity.locate(r, c, route)))
        assert not bool((b.bits()[run.written:] != b.sentinel).any()), "second launch wrote rows past offs[-1]"


# between two launches of a stream-K case: another grouped stream-K shape, and the smallest dense split-K case
_STREAM = [c for c, s in sorted(rc.GROUPED_CASES, key=lambda cs: rc.grouped_cost(cs[0])) if "/mx_stream/" in s]


def _other_users(case, dev):
    other = next(c for c in _STREAM if c[2:6] != case[2:6])
    dense = _SPLIT["gemm8"]

    def grouped():
        orun = GRun(other, 5, dev)
        orun.launch(orun.buffers())

    def split():
        drun = Run(dense, 7, dev)
        drun.launch(_parity.Guarded(dense.M, dense.N, drun.out_dtype, dev))

    return (grouped, split)


@pytest.fixture(scope="module")
def product_dispatch():
    """The launches take the product dispatch: no override may be set when the module starts, and none is left when it ends."""
    lib = _lib.lib()
    assert not lib.ao_gemm8_overridden(), "an earlier test left an ao_gemm8_* override set"
    try:
        yield lib
    finally:
        torch.cuda.synchronize()
        assert not lib.ao_gemm8_overridden()


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(rc.GROUPED_CASES)),
                         ids=["%s:%d,%d,%d,E%d:%s%s%s" % (s, c.M, c.N, c.K, c.E, c.offs, ":" + c.mode if c.mode else "",
                                                          "" if c.aligned else ":unal") for c, s in rc.GROUPED_CASES])
def test_grouped_route_parity(product_dispatch, index):
    case, sig = rc.GROUPED_CASES[index]
    lib = product_dispatch
    route = rc.grouped_route_of(lib, case)
    assert route is not None and route["sig"] == sig, (case, sig, route and route["sig"])
    dev = torch.device("cuda", 0)
    run = GRun(case, 2000 + index, dev)
    bufs = run.buffers()
    run.launch(bufs)
    run.check(bufs, route)
    between = _other_users(case, dev) if route["raw"]["kernel"] == "mx_stream" else ()
    _relaunch_same_bits(run, bufs, route, between)
    assert rc.grouped_route_of(lib, case)["sig"] == sig


# ---- forms no product route takes on the grid: one override test each ----

def _forced(lib, variant, run, bufs):
    lib.ao_gemm8_set_variant(variant)
    try:
        run.launch(bufs)
    finally:
        lib.ao_gemm8_set_variant(0)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,N,K", [
    ([0, 1, 7, 0, 3, 0, 5, 0], 208, 2048),      # mx_grouped_kernel, 1 m-tile (twice the average group <= 16 rows)
    ([0, 1, 40, 0, 30, 0, 18, 0], 1040, 2048),  # 2 m-tiles
    ([0, 1, 100, 0, 60, 0, 40, 0], 208, 4096),  # 4 m-tiles; a group of more than one 64-row pass
    ([0, 1, 9, 0, 3, 0, 5, 0], 208, 512),       # stream8_kernel<S8_MX>, 2 m-tiles (K % 2048 != 0)
    ([0, 1, 70, 0, 33, 0, 17, 0], 48, 384),     # 4 m-tiles
    ([0, 1, 0, 0], 48, 384),                    # 1 m-tile
])
def test_grouped_mx_variant_111_forms(product_dispatch, sizes, N, K):
    """Variant 111: the A-stationary mx_grouped_kernel (K % 2048 == 0) and the per-tile stream8_kernel<S8_MX> -- the product takes them
    only when rb8 cannot (2^32 bytes of codes in one operand, more than 65535 slabs).  One row past offs[-1]."""
    lib = product_dispatch
    M, E = sum(sizes) + 1, len(sizes)
    case = rc.GCase("grouped", "mx", M, N, K, E, True, "spread", "")
    dev = torch.device("cuda", 0)
    run = GRun(case, 111 + N + K, dev, sizes)
    bufs = run.buffers()
    _forced(lib, 111, run, bufs)
    run.check(bufs)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,N,K", [
    ([0, 1, 20, 0, 33, 0, 9, 0], 1040, 512),   # per-4-step scales
    ([0, 1, 20, 0, 33, 0, 9, 0], 208, 384),    # per-step scales
    ([0, 1, 90, 0, 3, 0, 9, 0], 208, 2048),    # a group of two 64-row slabs
])
def test_grouped_mx_variant_113_one_workgroup_per_tile(product_dispatch, sizes, N, K):
    """Variant 113: decode-size groups of ao_mxfp8_grouped_mm on one workgroup per (slab, tile) instead of the stream-K shares (the
    fused-cast and pair forms have no such form)."""
    lib = product_dispatch
    M, E = sum(sizes) + 1, len(sizes)
    case = rc.GCase("grouped", "mx", M, N, K, E, True, "spread", "")
    dev = torch.device("cuda", 0)
    run = GRun(case, 113 + N + K, dev, sizes)
    bufs = run.buffers()
    _forced(lib, 113, run, bufs)
    run.check(bufs)


# ---- every (instance, m-tile specialisation) of rb8_grouped_kernel (profiles/rb8_split_instances_tests.txt) ----
# (entry, waves, slab rows, k steps per scale fetch): key 3 forces the slab height; variant 113 keeps 64-row MX groups off the stream-K
# form; K = 1024 (a multiple of 512, more than six steps) takes the per-4-step scales, K = 896 (seven steps) the per-step ones; 8 waves
# need 400 (slab, tile) pairs, so M_total provides 134 slabs per group (the rows past offs[-1] keep the sentinel).
_RB8_GROUPED_FORMS = [("mx", 4, 64, 1), ("mx", 4, 64, 4), ("mx", 4, 128, 1), ("mx", 4, 128, 4), ("mx", 8, 128, 1), ("mx", 8, 128, 4),
                      ("fp8", 4, 64, 1), ("fp8", 4, 128, 1), ("fp8", 8, 128, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,waves,rows,qs,g", [(e, w, r, q, g) for e, w, r, q in _RB8_GROUPED_FORMS for g in (1, 17, 33, 65) if g < r])
def test_rb8_grouped_instances(product_dispatch, entry, waves, rows, qs, g):
    """Three experts with {0, g, 1} rows: the second group's slab has 1, 2, 3 or 5 m-tiles (the loop specialised on 1, 2, 4 or 8), the
    third one row.  N = 80: with 4 waves the second tile has one live n-tile, with 8 waves the single tile has three idle waves."""
    lib = product_dispatch
    N, K, E = 80, 1024 if qs == 4 else 896, 3
    M = g + 2 if waves == 4 else 133 * 128 + 1
    case = rc.GCase("grouped", entry, M, N, K, E, True, "spread", "")
    dev = torch.device("cuda", 0)
    run = GRun(case, 9000 + 10 * rows + g, dev, [0, g, 1])
    bufs = run.buffers()
    lib.ao_gemm8_set_variant(113)
    lib.ao_gemm8_set_tuning(3, rows)
    try:
        run.launch(bufs)
    finally:
        lib.ao_gemm8_set_variant(0)
        lib.ao_gemm8_set_tuning(3, 0)
    # ao_grouped8_route reports the product route only.  It is the forced form where grouped8_route needs no override for it: the 8-wave
    # cases (M_total > 48 E: 128-row slabs; 402 (slab, tile) pairs) and rowwise fp8 at 64 rows (decode-size groups, no stream-K form).
    # The other forms follow from key 3 and variant 113 by the same rules and cannot be read back.
    if waves == 8 or (entry == "fp8" and rows == 64):
        r = rc.route_grouped(lib, entry, M, N, K, E)
        assert (r["kernel"], r["slab_rows"], r["waves"], r["mt"], r["qs"]) == ("rb8", rows, waves, rows // 16, qs), r
    run.check(bufs)
