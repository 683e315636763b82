"""Every GEMM route the product takes (tests/route_cases.py CASES) against a float64 reference, through the C ABI, on guarded and
poisoned output buffers (tests/_parity.py).

Operands are drawn directly, not quantised from normals: int8 codes uniform over [-128, 127], every finite e4m3fn code, random int4
nibbles; row / column scales 2^U(-10, 4), int4 scales and zeros 2^U(-6, 2) per (group, column), bias randn x 2^U(-4, 4) per column,
bf16 activations (int4, dynamic entries) with row magnitudes 2^U(-8, 8).  A scale, group or bias read from the wrong index is off by a
large factor.  The reference is a float64 product in torch on the device; the int8 epilogue and the activation casts are the oracle's.
MX dense linears: every finite e4m3 code or all 16 e2m1 nibbles, E8M0 scales 127 + U{-12..12} per (row, 32-block), so a scale read
from the neighbouring block or the wrong half of the e4m3 lane map is off by up to 2^24; the fused cast's activations have magnitudes
2^U(-8, 8) per (row, block) and one all-zero block, cast by the oracle (oracle/mx_ref.to_mx, tests/mx_linear_ref.to_mx4) under both
scaling modes.  Every case launches twice into differently poisoned buffers (split-K routes with another split-K launch in between) and
must give the same bits; its route must still be the recorded one.
"""
import numpy as np
import pytest
import torch

import _parity
import route_cases as rc
from ao_amd import _lib
import mx_linear_ref
from oracle import fp8_ref, int4_ref, int8_ref, mx_ref

# Outputs equal to the oracle's rounding, at least (tests/_parity.py; bf16 x int4: its default 0.97).  Measured on every route of
# these families with the operands below: fp8 GEMMs 0.958 - 0.97, fp8 x int4 0.94 - 0.96, each element within the bound.
EQUAL_FP8 = 0.95
EQUAL_FP8_INT4 = 0.93
# MX dense (scaled MFMA): the floor on K of the bound (tests/_parity.py) and the equal fraction per format, measured on every MX case
# with the operands below (E8M0 scales spread over 2^+-12 per block).  e2m1: every element within ulp + 0.13 x 2^-23 S, equal 0.9997
# at least.  e4m3: one scaled MFMA sums e4m3 products spanning 2^36 less exactly than a float64 sum rounded once -- by a share of S
# that does not grow with K: the worst element needs max(K, floor) >= 1110 on the route cases (607 at K = 32, 1110 at 1024, 904 at
# 4160), 1153 on the forced stream form at K = 160 and 1286 on the grouped MX cases (K = 128) -- the same instruction, one floor:
# 1408.  Equal 0.963 at least.
K_FLOOR_E4M3_MX = 1408
K_FLOOR_MX = {"e2m1": 0, "e4m3": K_FLOOR_E4M3_MX}
EQUAL_MX = {"e2m1": 0.99, "e4m3": 0.96}
MX_MODES = {"floor": mx_ref.FLOOR, "rceil": mx_ref.RCEIL}

_TILE_INDEX = None


def _tile_index():
    """Flat (n, k) index, inside one 16 x 128 tile, of every nibble slot of the tile's 64 x 4 words (oracle int4_ref._tile_coords)."""
    global _TILE_INDEX
    if _TILE_INDEX is None:
        n_idx, k_idx = int4_ref._tile_coords(1, 1)
        _TILE_INDEX = torch.from_numpy((n_idx[0, 0] * 128 + k_idx[0, 0]).astype(np.int64))
    return _TILE_INDEX


def pack_int4(q):
    """oracle int4_ref.convert_weight_to_int4pack(nibble_pack(q)) in torch: q int [N, K] in 0..15 -> int32 [N/8, K/128, 32, 4]."""
    N, K = q.shape
    t = q.reshape(N // 16, 16, K // 128, 128).permute(0, 2, 1, 3).reshape(N // 16, K // 128, 2048)
    vals = t[:, :, _tile_index().to(q.device).view(-1)].view(N // 16, K // 128, 64, 4, 8).to(torch.int64)
    words = (vals << (4 * torch.arange(8, device=q.device))).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return words.reshape(N // 8, K // 128, 32, 4)


def dequant_tinygemm(q, sz, G):
    """oracle int4_ref.dequantize_tinygemm in torch: bf16( bf16( bf16(q - 8) * s ) + z ), bf16 [N, K]."""
    N, K = q.shape
    s = sz[..., 0].float().T[:, :, None]
    z = sz[..., 1].float().T[:, :, None]
    w = ((q - 8).float().view(N, K // G, G) * s).bfloat16().float() + z
    return w.bfloat16().view(N, K)


# ---- operands ----

class Draw:
    def __init__(self, seed, dev):
        self.g = torch.Generator(device=dev).manual_seed(seed)
        self.dev = dev

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.g, device=self.dev, dtype=torch.float64)

    def pow2(self, lo, hi, *shape):
        return torch.exp2(self.rand(*shape) * (hi - lo) + lo)

    def int8(self, *shape):
        return torch.randint(-128, 128, shape, generator=self.g, device=self.dev, dtype=torch.int8)

    def fp8(self, *shape):
        """Every finite e4m3fn code (0x7F / 0xFF are NaN), subnormals and +-448 included."""
        i = torch.randint(0, 254, shape, generator=self.g, device=self.dev)
        return (i + (i >= 0x7F).to(i.dtype)).to(torch.uint8)

    def nibbles(self, *shape):
        return torch.randint(0, 16, shape, generator=self.g, device=self.dev)

    def scales(self, n):
        return self.pow2(-10, 4, n).float()

    def bias(self, n):
        return (torch.randn(n, generator=self.g, device=self.dev, dtype=torch.float64) * self.pow2(-4, 4, n)).bfloat16()

    def act(self, M, K):
        """bf16 activations whose row magnitudes span 2^-8 .. 2^8."""
        x = torch.randn(M, K, generator=self.g, device=self.dev, dtype=torch.float64) * self.pow2(-8, 8, M, 1)
        return x.bfloat16()

    def e8m0(self, *shape):
        """E8M0 block scales 127 + U{-12..12}, independent per element."""
        return (127 + torch.randint(-12, 13, shape, generator=self.g, device=self.dev)).to(torch.uint8)

    def e2m1(self, *shape):
        """Packed e2m1 codes [..., K / 2] of all 16 nibbles (element 2i in the low nibble of byte i)."""
        q = self.nibbles(*shape)
        return (q[..., 0::2] | (q[..., 1::2] << 4)).to(torch.uint8)

    def mx_act(self, M, K):
        """bf16 activations whose (row, 32-block) magnitudes span 2^-8 .. 2^8, one block all zero."""
        x = torch.randn(M, K, generator=self.g, device=self.dev, dtype=torch.float64)
        x = x * self.pow2(-8, 8, M, K // 32).repeat_interleave(32, 1)
        x[M // 2, 32 * ((K // 32) // 2):32 * ((K // 32) // 2 + 1)] = 0
        return x.bfloat16()

    def int4_sz(self, K, N, G, zeros=True):
        s = self.pow2(-6, 2, K // G, N)
        z = self.pow2(-6, 2, K // G, N) * (torch.randint(0, 2, (K // G, N), generator=self.g, device=self.dev) * 2 - 1) if zeros else 0 * s
        return torch.stack([s, z], -1).bfloat16().contiguous()


def _offset(t, aligned):
    """t itself, or a copy of it at a one-element offset (4 bytes for fp32 scales, 2 for bf16 bias, 1 for E8M0 scales)."""
    if aligned or t is None:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


def _e4m3(codes):
    return torch.from_numpy(fp8_ref.E4M3.astype(np.float64)).to(codes.device)[codes.long()]


def _ptr(t):
    return None if t is None else t.data_ptr()


def mx_dequant(codes, scale, fmt):
    """float64 elements 2^(scale - 127) of e4m3 codes [..., K] or packed e2m1 [..., K / 2] (exact)."""
    if fmt == "e2m1":
        table = torch.from_numpy(mx_linear_ref.E2M1_VALUES.astype(np.float64)).to(codes.device)
        q = torch.stack([codes & 15, codes >> 4], -1).flatten(-2)
        v = table[q.long()]
    else:
        v = _e4m3(codes)
    return v * torch.exp2(scale.double() - 127).repeat_interleave(32, -1)


def mx_cast(x, fmt, mode):
    """The oracle's 1 x 32 cast of bf16 x (to_mx / to_mx4) -> (codes, E8M0 scales) on x's device."""
    if fmt == "e2m1":
        q, s = mx_linear_ref.to_mx4(x.view(torch.int16).cpu().numpy().view(np.uint16), MX_MODES[mode])
    else:
        q, s = mx_ref.to_mx(x.float().cpu().numpy(), MX_MODES[mode])
    return torch.from_numpy(np.ascontiguousarray(q)).to(x.device), torch.from_numpy(np.ascontiguousarray(s)).to(x.device)


# ---- one case: operands, launch, reference ----

class Run:
    """Operands of a case, a launch into a guarded buffer, and the reference the output must meet."""

    def __init__(self, case, seed, dev, mode=None):
        self.case, self.dev, self.mode = case, dev, mode
        fam, entry, M, N, K, G, bias, aligned = case
        d = Draw(seed, dev)
        self.bias = d.bias(N) if bias else None
        self.ref = {}
        if fam == "gemm8":
            self._gemm8(d, entry, M, N, K)
        elif fam == "int4":
            self._int4(d, M, N, K, G)
        elif fam == "mx":
            self._mx(d, entry, M, N, K)
        else:
            self._fp8_int4(d, entry, M, N, K, G)
        self.sa = _offset(getattr(self, "sa", None), aligned)
        self.sb = _offset(getattr(self, "sb", None), aligned)
        self.bias_arg = _offset(self.bias, aligned)

    def _bias64(self):
        return 0 if self.bias is None else self.bias.double()[None, :]

    def _gemm8(self, d, entry, M, N, K):
        self.out_dtype = torch.int32 if entry == "int_mm" else torch.float32 if entry == "fp8_mm_f32" else torch.bfloat16
        if entry in ("int8_dyn", "fp8_dyn"):
            self.x = d.act(M, K)
            xs = self.x.float().cpu().numpy()
            q, s = (int8_ref if entry == "int8_dyn" else fp8_ref).quantize_rowwise(xs)
            self.a = torch.from_numpy(q.view(np.uint8) if entry == "fp8_dyn" else q).to(self.dev)
            self.sa = torch.from_numpy(s).to(self.dev)
        else:
            self.a = d.int8(M, K) if entry in ("int8_scaled", "int_mm") else d.fp8(M, K)
            self.sa = d.scales(M) if entry in rc.SCALED else None
        int8 = entry in ("int8_scaled", "int_mm", "int8_dyn")
        self.b = d.int8(N, K) if int8 else d.fp8(N, K)
        self.sb = d.scales(N) if entry not in ("int_mm", "fp8_mm_f32") else None
        A, B = (self.a.double(), self.b.double()) if int8 else (_e4m3(self.a), _e4m3(self.b))
        acc = A @ B.T
        if entry == "int_mm":
            self.ref["ref_bits"] = acc.to(torch.int32)
        elif int8:  # the oracle's epilogue on the exact accumulator (int8_ref.scaled_mm)
            y = (acc.float() * self.sa[:, None]).bfloat16().float() * self.sb[None, :]
            if self.bias is not None:
                y = y + self.bias.float()[None, :]
            self.ref["ref_bits"] = y.bfloat16()
        else:
            S = A.abs() @ B.abs().T
            if entry != "fp8_mm_f32":
                sc = self.sa.double()[:, None] * self.sb.double()[None, :]
                acc, S = acc * sc + self._bias64(), S * sc + abs(self._bias64())
            self.ref.update(ref64=acc, S=S, K=K, equal=EQUAL_FP8)

    def _int4(self, d, M, N, K, G):
        self.out_dtype = torch.bfloat16
        self.x = d.act(M, K)
        q = d.nibbles(N, K)
        self.qdata = pack_int4(q)
        self.sz = d.int4_sz(K, N, G)
        w = dequant_tinygemm(q, self.sz, G).double()
        X = self.x.double()
        self.ref.update(ref64=X @ w.T, S=X.abs() @ w.abs().T, K=K)

    def _fp8_int4(self, d, entry, M, N, K, G):
        self.out_dtype = torch.bfloat16
        if entry.startswith("dyn"):
            self.x = d.act(M, K)
            q8, s8 = fp8_ref.quantize_rowwise(self.x.float().cpu().numpy())
            self.a, self.sa = torch.from_numpy(q8).to(self.dev), torch.from_numpy(s8).to(self.dev)
        else:
            self.a, self.sa = d.fp8(M, K), d.scales(M)
        q = d.nibbles(N, K)
        self.qdata = pack_int4(q)
        self.sz = d.int4_sz(K, N, G, zeros=entry.endswith("asym"))
        s = self.sz[..., 0].double().T.repeat_interleave(G, 1)
        z = self.sz[..., 1].double().T.repeat_interleave(G, 1)
        w, wabs = s * (q - 8).double() + z, (s * (q - 8).double()).abs() + z.abs()
        X = _e4m3(self.a)
        xs = self.sa.double()[:, None]
        self.ref.update(ref64=xs * (X @ w.T) + self._bias64(), S=xs * (X.abs() @ wabs.T) + abs(self._bias64()), K=K, equal=EQUAL_FP8_INT4)

    def _mx(self, d, entry, M, N, K):
        """Codes and scales drawn directly (codes entry) or the oracle's cast of drawn activations (fused entry, self.mode)."""
        fmt, form = entry.split("_")
        self.fmt, self.out_dtype = fmt, torch.bfloat16
        codes = d.fp8 if fmt == "e4m3" else (lambda r, k: d.e2m1(r, k))
        self.b, self.sb = codes(N, K), d.e8m0(N, K // 32)
        if form == "codes":
            self.a, self.sa = codes(M, K), d.e8m0(M, K // 32)
        else:
            self.x = d.mx_act(M, K)
            self.a, self.sa = mx_cast(self.x, fmt, self.mode)
        A, B = mx_dequant(self.a, self.sa, fmt), mx_dequant(self.b, self.sb, fmt)
        self.ref.update(ref64=A @ B.T + self._bias64(), S=A.abs() @ B.abs().T + abs(self._bias64()), K=K, equal=EQUAL_MX[fmt],
                        k_floor=K_FLOOR_MX[fmt])

    def launch(self, buf, sync=True):
        lib = _lib.lib()
        fam, entry, M, N, K, G = self.case[:6]
        s = torch.cuda.current_stream().cuda_stream
        y = buf.out.data_ptr()
        if fam == "gemm8":
            call = {
                "int8_scaled": lambda: lib.ao_int8_scaled_mm(_ptr(self.a), _ptr(self.sa), _ptr(self.b), _ptr(self.sb), _ptr(self.bias_arg), y, M, N, K, s),
                "fp8_scaled": lambda: lib.ao_fp8_scaled_mm(_ptr(self.a), _ptr(self.b), _ptr(self.sa), _ptr(self.sb), _ptr(self.bias_arg), y, M, N, K, s),
                "int_mm": lambda: lib.ao_int8_int_mm(_ptr(self.a), _ptr(self.b), y, M, N, K, s),
                "fp8_mm_f32": lambda: lib.ao_fp8_mm_f32(_ptr(self.a), _ptr(self.b), y, M, N, K, s),
                "int8_dyn": lambda: lib.ao_int8_dynamic_linear(_ptr(self.x), _ptr(self.b), _ptr(self.sb), _ptr(self.bias_arg), y, M, N, K, s),
                "fp8_dyn": lambda: lib.ao_fp8_dynamic_linear(_ptr(self.x), _ptr(self.b), _ptr(self.sb), _ptr(self.bias_arg), y, M, N, K, s),
            }[entry]
            rc_ = call()
        elif fam == "mx":
            fmt = rc.MX_FMT[self.fmt]
            if entry.endswith("fused"):
                rc_ = lib.ao_mx_dynamic_linear(fmt, _ptr(self.x), _ptr(self.b), _ptr(self.sb), _ptr(self.bias_arg), y, M, N, K, MX_MODES[self.mode], s)
            else:
                rc_ = lib.ao_mx_linear(fmt, _ptr(self.a), _ptr(self.sa), _ptr(self.b), _ptr(self.sb), _ptr(self.bias_arg), y, M, N, K, s)
        elif fam == "int4":
            rc_ = lib.ao_int4_weight_int4pack_mm(_ptr(self.x), _ptr(self.qdata), _ptr(self.sz), y, M, N, K, G, s)
        elif entry.startswith("dyn"):
            rc_ = lib.ao_fp8_int4_dynamic_linear(_ptr(self.x), _ptr(self.qdata), _ptr(self.sz), _ptr(self.bias_arg), y, M, N, K, G, s)
        else:
            rc_ = lib.ao_fp8_int4_linear(_ptr(self.a), _ptr(self.sa), _ptr(self.qdata), _ptr(self.sz), _ptr(self.bias_arg), y, M, N, K, G, s)
        _lib.check(rc_)
        if sync:
            torch.cuda.synchronize()


# the smallest split-K case of each family: launched between the two launches of a split-K case
_SPLIT = {}
for _c, _s in sorted(rc.CASES, key=lambda cs: rc.cost(cs[0])):
    if _s.endswith("/kparts"):
        _SPLIT.setdefault(_c.family, _c)


@pytest.fixture(scope="module")
def product_dispatch():
    """The launches take the product dispatch: no override may be set when the module starts, and none is left when it ends."""
    lib = _lib.lib()
    assert not lib.ao_gemm8_overridden() and not lib.ao_int4_overridden(), "an earlier test left an ao_gemm8_* / ao_int4_set_tuning override set"
    try:
        yield lib
    finally:
        torch.cuda.synchronize()
        assert not lib.ao_gemm8_overridden() and not lib.ao_int4_overridden()


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(rc.CASES)), ids=["%s:%d,%d,%d%s%s" % (s, c.M, c.N, c.K, "+b" if c.bias else "", "" if c.aligned else ":unal")
                                                              for c, s in rc.CASES])
def test_route_parity(product_dispatch, index):
    case, sig = rc.CASES[index]
    lib = product_dispatch
    route = rc.route_of(lib, case)
    assert route is not None and route["sig"] == sig, (case, sig, route and route["sig"])
    dev = torch.device("cuda", 0)
    for mode in (MX_MODES if case.family == "mx" and case.entry.endswith("fused") else (None,)):
        run = Run(case, 1000 + index, dev, mode)
        buf = _parity.Guarded(case.M, case.N, run.out_dtype, dev)
        run.launch(buf)
        _parity.check(buf, route=route, **run.ref)
        first = buf.bits().clone()

        if route["parts"] > 1:  # no ticket or workspace state may carry over from another split-K launch
            other = _SPLIT[case.family] if _SPLIT[case.family] != case else None
            if other is not None:
                orun = Run(other, 7, dev)
                orun.launch(_parity.Guarded(other.M, other.N, orun.out_dtype, dev))
        buf.poison(_parity.SENTINEL2)
        run.launch(buf)
        assert not buf.guard_problems(), buf.guard_problems()
        same = buf.bits() == first
        if not bool(same.all()):
            i, j = (int(v) for v in torch.nonzero(~same)[0])
            raise AssertionError("second launch differs in %d elements, first at row %d, column %d%s"
                                 % (int((~same).sum()), i, j, _parity.locate(i, j, route)))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ("int8_dyn", "fp8_dyn"))
@pytest.mark.parametrize("M", (1, 5, 16))
@pytest.mark.parametrize("bias", (False, True))
def test_dyn8_override_form(product_dispatch, entry, M, bias):
    """dyn8_kernel, the fused decode form no product route takes (ao_gemm8_set_variant(299): never dec8_kernel), against the same
    reference: its int8 epilogue adds the bias to the rounded product like the others."""
    lib = product_dispatch
    case = rc.Case("gemm8", entry, M, 208, 1152, 0, bias, True)
    dev = torch.device("cuda", 0)
    run = Run(case, 77 + M, dev)
    buf = _parity.Guarded(case.M, case.N, run.out_dtype, dev)
    lib.ao_gemm8_set_variant(299)
    try:
        run.launch(buf)
    finally:
        lib.ao_gemm8_set_variant(0)
    _parity.check(buf, **run.ref)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ("fp8_scaled", "int8_scaled"))
@pytest.mark.parametrize("parts", (1, 2))
def test_rb8_1x8_override_form(product_dispatch, entry, parts):
    """The 1 x 8 wave arrangement of the 8-wave x 128-row rowwise form (ao_gemm8_set_variant(103); the product stands 2 x 4), forced with
    128-row slabs (key 3) and 128-column tiles (key 1): M = 130 leaves a second slab of 2 rows, N = 144 a second column tile with one
    live n-tile (the aliased tiles past N), K = 896 seven k steps (every ring wraps), key 2 one meeting of two K parts."""
    lib = product_dispatch
    case = rc.Case("gemm8", entry, 130, 144, 896, 0, True, True)
    assert case.K // 128 > rc.KLOOP_STEPS
    dev = torch.device("cuda", 0)
    run = Run(case, 103 + parts, dev)
    buf = _parity.Guarded(case.M, case.N, run.out_dtype, dev)
    lib.ao_gemm8_set_variant(103)
    lib.ao_gemm8_set_tuning(3, 128)
    lib.ao_gemm8_set_tuning(1, 128)
    lib.ao_gemm8_set_tuning(2, parts)
    try:
        run.launch(buf)
    finally:
        lib.ao_gemm8_set_variant(0)
        for key in (3, 1, 2):
            lib.ao_gemm8_set_tuning(key, 0)
    # ao_gemm8_route reports the product route (no override): the shape is rb8_kernel's; variant 103 and keys 1 - 3 change no route, only the
    # launch shape inside it (rb8_launch_plan), which no query reports under an override
    assert rc.route8(lib, entry, case.M, case.N, case.K, True)["kernel"] == "rb8"
    _parity.check(buf, **run.ref)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,M,N,form", [
    ("e4m3_codes", 100, 1000, 1), ("e4m3_fused", 100, 1000, 1), ("e2m1_codes", 100, 257, 1), ("e2m1_fused", 70, 257, 1),
    ("e4m3_codes", 5, 1000, 2), ("e2m1_codes", 32, 257, 2),
])
def test_mx_linear_forced_forms(entry, M, N, form):
    """ao_mx_linear_set_form: the stream form above the seam (4 m-tiles, more than one grid row), the tiled form at M <= seam; the
    route query reads the same override, so the form that runs is asserted."""
    lib = _lib.lib()
    K = 160
    case = rc.Case("mx", entry, M, N, K, 0, True, True)
    dev = torch.device("cuda", 0)
    for mode in (MX_MODES if entry.endswith("fused") else (None,)):
        run = Run(case, 31 + M, dev, mode)
        buf = _parity.Guarded(M, N, torch.bfloat16, dev)
        lib.ao_mx_linear_set_form(form)
        try:
            r = rc.mx_route(lib, rc.MX_FMT[run.fmt], M, N, K)
            run.launch(buf)
        finally:
            lib.ao_mx_linear_set_form(0)
        product = rc.mx_route(lib, rc.MX_FMT[run.fmt], M, N, K)["kernel"]
        assert r["kernel"] == rc.MX_KERNELS[form] != product, (r, product)
        if form == 1:
            assert r["mt"] == 4 and r["grid_y"] > 1, r
        _parity.check(buf, **run.ref)
