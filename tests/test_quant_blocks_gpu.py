"""The kernels around the 8-bit GEMMs (quant_kernels.hip) at their addressing edges, HIP against the numpy oracles, bit for bit:

* the K-sharded casts (rowwise_amax and the int8 / fp8 casts with a given amax) through the C ABI on a window of a wider matrix whose other
  columns hold +-3.0e38, at every register depth of the one-sweep kernels and the two-sweep kernels, with the window's own, a larger and
  a smaller amax (the last saturates the codes); every bf16 value with power-of-two scales; the layouts the Python wrapper has to copy;
* the scale epilogues on their own: outputs that name their (m, n) at the seams of the row-chunk and column-stride loops, and arbitrary
  int32 / fp32 accumulators against the oracle (fp8: inside the interval three fp32 roundings allow);
* the static, asymmetric and per-tensor casts and the int8 row sums;
* the rank-local chain of the row-parallel protocol captured in one graph.

Every output of a C entry point sits in a guarded, poisoned buffer (_parity.Guarded)."""
import numpy as np
import pytest
import torch

import _parity
from oracle import bf16, fp8_ref as F8, int8_ref as I8

pytestmark = pytest.mark.gpu

from ao_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda", 0)
POISON = 3.0e38  # finite in bf16; an amax that meets it is wrong by 2^100, a cast that meets it saturates


def stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """`count` elements of a numpy dtype in a guarded buffer of bytes (16-byte aligned, 256 guard bytes before and at least 32 after)."""

    def __init__(self, count, dtype):
        self.count, self.dtype = count, np.dtype(dtype)
        self.nbytes = count * self.dtype.itemsize
        self.g = _parity.Guarded(1, (self.nbytes + 1) // 2, torch.bfloat16, DEV)
        self.ptr = self.g.out.data_ptr()

    def get(self):
        """The elements written, after asserting that nothing around them was."""
        assert not self.g.guard_problems(), self.g.guard_problems()
        raw = self.g.bits().contiguous().view(torch.uint8).reshape(-1).cpu().numpy()
        if self.nbytes % 2:
            assert raw[self.nbytes] == (_parity.SENTINEL[torch.bfloat16] >> 8), "write into the byte after the output"
        return raw[:self.nbytes].view(self.dtype).copy()


def dev_bf16(a):
    """bf16-valued fp32 numpy -> bf16 device tensor (exact)"""
    assert bf16.is_bf16(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_fp8(got, want, what):
    """e4m3 codes, bit for bit but for the NaN codes of a 0 / 0 row, whose sign falls as it falls (as test_cast_shape_sweep)"""
    nan_w, nan_g = (want & 0x7F) == 0x7F, (got & 0x7F) == 0x7F
    assert np.array_equal(nan_w, nan_g) and np.array_equal(got[~nan_g], want[~nan_w]), what


def rows_of_many_magnitudes(M, K, seed):
    """bf16-valued fp32 [M, K]: every row its own magnitude 2^[-20, 20], one all-zero row where there is more than one"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-20, 21, (M, 1), generator=g).float())
    if M > 1:
        x[M // 2] = 0
    return x.to(torch.bfloat16).float().numpy()


def wide_with_window(x, W, c0):
    """[M, W] bf16 on the device, +-POISON everywhere but x in the columns [c0, c0 + K); the window view"""
    M, K = x.shape
    wide = torch.full((M, W), POISON, dtype=torch.bfloat16)
    wide[:, 1::2] = -POISON
    wide[:, c0:c0 + K] = torch.from_numpy(x).to(torch.bfloat16)
    wide = wide.to(DEV)
    return wide, wide[:, c0:c0 + K]


def given_amaxes(x):
    """(name, amax [M]) x 3: the window's own; a larger one (the row's maximum sits in another shard: 1.0 for the zero row); a quarter
    of the true one (codes saturate)"""
    own = np.abs(x).max(axis=1).astype(np.float32)
    return [("own", own), ("larger", np.where(own > 0, own * np.float32(4.0), np.float32(1.0)).astype(np.float32)),
            ("quarter", (own * np.float32(0.25)).astype(np.float32))]


# ---- 1. the K-sharded casts ------------------------------------------------------------------------------------------------------------
# vectors of 8 per thread: 1, 1, 2, 2, 4, 8, 8, then the two-sweep kernels (K > 16384); a ragged last vector wherever K allows one
SHARD_KS = [8, 2048, 2056, 4096, 4104, 8200, 16384, 16392, 20000]


@pytest.mark.parametrize("K", SHARD_KS)
def test_sharded_casts_on_a_window_of_a_wider_matrix_through_the_c_abi(K):
    lib = _lib.lib()
    for M in (1, 3, 17):
        x = rows_of_many_magnitudes(M, K, 1000 * M + K)
        amaxes = given_amaxes(x)
        want = {(fmt, name): ref.quantize_rowwise(x, amax=a) for fmt, ref in (("int8", I8), ("fp8", F8)) for name, a in amaxes}
        contiguous = dev_bf16(x)
        whole = {"int8": ops.int8_quantize_rowwise(contiguous), "fp8": ops.fp8_quantize_rowwise(contiguous)}
        for W, c0 in ((K + 8, 0), (K + 264, 128)):
            where = "M=%d K=%d W=%d c0=%d" % (M, K, W, c0)
            wide, view = wide_with_window(x, W, c0)
            assert view.data_ptr() % 16 == 0 and view.stride(0) == W
            am = Out(M, np.float32)
            _lib.check(lib.ao_rowwise_amax(view.data_ptr(), W, am.ptr, M, K, stream()))
            assert np.array_equal(u32(am.get()), u32(amaxes[0][1])), ("amax", where)
            assert torch.equal(ops.rowwise_amax(view), dev(amaxes[0][1])), ("ops.rowwise_amax", where)
            for name, a in amaxes:
                ad = dev(a)
                for fmt, entry, wrapper in (("int8", lib.ao_int8_quantize_rowwise_amax, ops.int8_quantize_rowwise_amax),
                                            ("fp8", lib.ao_fp8_quantize_rowwise_amax, ops.fp8_quantize_rowwise_amax)):
                    q, s = Out(M * K, np.uint8), Out(M, np.float32)
                    _lib.check(entry(view.data_ptr(), W, ad.data_ptr(), q.ptr, s.ptr, M, K, stream()))
                    wq, ws = want[(fmt, name)]
                    what = (fmt, name, where)
                    got_q, got_s = q.get().reshape(M, K), s.get()
                    assert np.array_equal(u32(got_s), u32(ws)), ("scale",) + what
                    if fmt == "int8":
                        assert np.array_equal(got_q.view(np.int8), wq), ("codes",) + what
                    else:
                        same_fp8(got_q, wq, ("codes",) + what)
                    if name == "quarter" and K >= 2048:  # both clamps are met (+-448 are the codes 0x7e and 0xfe)
                        hi, lo = (0x7F, 0x80) if fmt == "int8" else (0x7E, 0xFE)
                        assert (got_q == hi).any() and (got_q == lo).any(), ("no clamp",) + what
                    pq, ps = wrapper(view, ad)  # the wrapper takes the view as it is
                    assert np.array_equal(pq.view(torch.uint8).cpu().numpy(), got_q) and np.array_equal(ps.flatten().cpu().numpy(), got_s), ("ops",) + what
                    if name == "own":  # a shard that holds its rows' maxima casts like a matrix of its own
                        cq, cs = whole[fmt]
                        assert np.array_equal(cq.view(torch.uint8).cpu().numpy(), got_q) and np.array_equal(cs.flatten().cpu().numpy(), got_s), ("whole",) + what
        torch.cuda.synchronize()


def copied_layouts(x):
    """(name, view) of the layouts _strided_rows cannot hand over as they are: a base that is not 16-byte aligned, a row stride that is no
    multiple of 8, rows that are not contiguous"""
    M, K = x.shape
    yield "c0=4", wide_with_window(x, K + 8, 4)[1]
    yield "stride K+4", wide_with_window(x, K + 4, 0)[1]
    yield "x.t()", dev_bf16(np.ascontiguousarray(x.T)).t()


@pytest.mark.parametrize("K", [8, 2056, 16392])
def test_the_wrappers_copy_the_layouts_the_kernels_cannot_take(K):
    for M in (1, 3, 17):
        x = rows_of_many_magnitudes(M, K, 77 * M + K)
        amaxes = given_amaxes(x)
        for layout, view in copied_layouts(x):
            assert tuple(view.shape) == (M, K)
            assert torch.equal(ops.rowwise_amax(view), dev(amaxes[0][1])), (layout, M, K)
            for name, a in amaxes:
                wq, ws = I8.quantize_rowwise(x, amax=a)
                q, s = ops.int8_quantize_rowwise_amax(view, dev(a))
                assert np.array_equal(q.cpu().numpy(), wq) and np.array_equal(u32(s.flatten().cpu().numpy()), u32(ws)), ("int8", layout, name, M, K)
                wq, ws = F8.quantize_rowwise(x, amax=a)
                q, s = ops.fp8_quantize_rowwise_amax(view, dev(a))
                assert np.array_equal(u32(s.flatten().cpu().numpy()), u32(ws)), ("fp8 scale", layout, name, M, K)
                same_fp8(q.view(torch.uint8).cpu().numpy(), wq, ("fp8", layout, name, M, K))


def test_no_rows_of_any_layout_give_empty_outputs():
    K = 24
    x = rows_of_many_magnitudes(3, K, 5)
    views = [("window", wide_with_window(x, K + 8, 0)[1]), ("contiguous", dev_bf16(x))] + list(copied_layouts(x))
    for layout, view in views:
        empty = view[:0]
        none = torch.empty((0,), dtype=torch.float32, device=DEV)
        a = ops.rowwise_amax(empty)
        assert tuple(a.shape) == (0,) and a.dtype == torch.float32, layout
        for fn, dtype in ((ops.int8_quantize_rowwise_amax, torch.int8), (ops.fp8_quantize_rowwise_amax, torch.float8_e4m3fn)):
            q, s = fn(empty, none)
            assert tuple(q.shape) == (0, K) and q.dtype == dtype and tuple(s.shape) == (0, 1) and s.dtype == torch.float32, layout
    t = dev_bf16(np.ascontiguousarray(x.T))[:, :0].t()  # x.t() of a [K, 0] tensor
    assert tuple(ops.rowwise_amax(t).shape) == (0,)


def every_bf16_value():
    """The 65536 bit patterns as bf16-valued fp32 [256, 256]: NaNs replaced by 0, +-Inf kept"""
    v = bf16.from_bits(np.arange(65536, dtype=np.uint32).astype(np.uint16)).reshape(256, 256).copy()
    v[np.isnan(v)] = 0.0
    return v


@pytest.mark.parametrize("e", [-3, 0, 6])
def test_every_bf16_value_with_a_power_of_two_scale_and_a_given_amax(e):
    """amax = 127.5 2^e (int8) and 448 2^e (fp8) make the scale exactly 2^e: a sixteenth of all inputs then sit on a rounding tie, and
    everything beyond the range on a clamp."""
    x = every_bf16_value()
    xd = dev_bf16(x)
    for ref, fn, top in ((I8, ops.int8_quantize_rowwise_amax, 127.5), (F8, ops.fp8_quantize_rowwise_amax, 448.0)):
        a = np.full((256,), np.float32(top) * np.float32(2.0 ** e), dtype=np.float32)
        with np.errstate(all="ignore"):
            wq, ws = ref.quantize_rowwise(x, amax=a)
        assert (ws == np.float32(2.0 ** e)).all()
        q, s = fn(xd, dev(a))
        assert np.array_equal(u32(s.flatten().cpu().numpy()), u32(ws)), (ref.__name__, e)
        got = q.view(torch.uint8).cpu().numpy()
        bad = np.argwhere(got != wq.view(np.uint8))
        assert bad.size == 0, "%s e=%d: %d codes differ, first bf16 pattern 0x%04x: %d vs %d" % (
            ref.__name__, e, len(bad), bad[0][0] * 256 + bad[0][1], got[tuple(bad[0])], wq.view(np.uint8)[tuple(bad[0])])


# ---- 2. the scale epilogues on their own -----------------------------------------------------------------------------------------------
# (3, 16645): 66 column blocks under the cap of 64, some threads stride twice; 65535 rows is one launch, 65536 / 65537 one row or two past
# it, 131071 a second launch one row short of full
INDEX_SHAPES = [(1, 1), (3, 255), (5, 257), (3, 16645), (65535, 8), (65536, 8), (65537, 3), (131071, 3)]
ROW_CHUNK = 65535


def index_case(M, N):
    """Operands whose output names its (m, n): small integers and powers of two, so that the int32 -> fp32 conversion, both products and the
    bias add are exact in fp32 whichever way the compiler fuses them; what is left are the oracle's bf16 roundings."""
    m, n = np.arange(M, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    acc = ((m * N + n) % 2039).astype(np.int32)  # < 2^11; neighbours along either axis differ, and so do rows 65535 apart (N < 2039)
    assert M <= ROW_CHUNK or (ROW_CHUNK * N) % 2039 != 0
    rs = np.exp2(np.arange(M) % 7).astype(np.float32)  # 65535 % 7 = 1: a row of the second launch has another scale than its twin
    cs = np.exp2(-(np.arange(N) % 5)).astype(np.float32)
    bias = ((np.arange(N) % 11) - 5).astype(np.float32)
    return acc, rs, cs, bias


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("kind", ["int8", "fp8", "asym"])
@pytest.mark.parametrize("M,N", INDEX_SHAPES)
def test_the_epilogues_put_every_element_where_it_belongs(M, N, kind, with_bias):
    lib = _lib.lib()
    acc, rs, cs, bias = index_case(M, N)
    b = bias if with_bias else None
    bd = dev_bf16(bias) if with_bias else None
    bp = bd.data_ptr() if with_bias else None
    rsd, csd = dev(rs), dev(cs)
    runs = []
    if kind == "int8":
        accd = dev(acc)
        runs.append((I8.scale_epilogue(acc, rs, cs, b), lambda y: lib.ao_int8_scale_epilogue(accd.data_ptr(), rsd.data_ptr(), csd.data_ptr(), bp, y, M, N, stream())))
    elif kind == "fp8":
        accd = dev(acc.astype(np.float32))
        r = acc.astype(np.float64) * rs[:, None].astype(np.float64) * cs[None, :].astype(np.float64) + (0.0 if b is None else b[None, :].astype(np.float64))
        assert np.array_equal(r.astype(np.float32).astype(np.float64), r)  # exact in fp32: one rounding, to bf16, is left
        runs.append((bf16.bf16_round(r.astype(np.float32)), lambda y: lib.ao_fp8_scale_epilogue(accd.data_ptr(), rsd.data_ptr(), csd.data_ptr(), bp, y, M, N, stream())))
    else:
        accd = dev(acc)
        wsum = (np.arange(N) % 9).astype(np.int32)
        wsd = dev(wsum)
        # (m % 5) - 2 repeats every 65535 rows: the second zero-point, shifted by one in the second launch, tells the two launches apart
        zps = [((np.arange(M) % 5) - 2).astype(np.int8)]
        if M > ROW_CHUNK:
            zps.append((((np.arange(M) + np.arange(M) // ROW_CHUNK) % 5) - 2).astype(np.int8))
        for zp in zps:
            zpd = dev(zp)
            runs.append((I8.scale_epilogue_asym(acc, rs, zp, wsum, cs, b),
                         lambda y, zpd=zpd: lib.ao_int8_scale_epilogue_asym(accd.data_ptr(), rsd.data_ptr(), zpd.data_ptr(), wsd.data_ptr(), csd.data_ptr(), bp, y, M, N, stream())))
    for want, call in runs:
        buf = _parity.Guarded(M, N, torch.bfloat16, DEV)
        _lib.check(call(buf.out.data_ptr()))
        torch.cuda.synchronize()
        _parity.check(buf, ref_bits=dev_bf16(want))


ARITH_SHAPES = [(37, 512), (130, 1040)]


def arith_case(M, N, seed):
    """int32 accumulators of every magnitude, the ones next to 2^24 (where (float)c starts to round) and both ends of the range among them;
    fp32 scales with full significands; a bf16 bias"""
    rng = np.random.default_rng(seed)
    acc = (rng.integers(-(1 << 31), 1 << 31, size=(M, N)) >> rng.integers(0, 31, size=(M, N))).astype(np.int32)
    acc.reshape(-1)[:6] = np.array([(1 << 24) + 1, -((1 << 24) + 1), (1 << 31) - 1, -(1 << 31), (1 << 25) + 3, 0], dtype=np.int64).astype(np.int32)
    acc[M - 1, N - 4:] = np.array([(1 << 31) - 1, -(1 << 31), (1 << 24) + 1, -((1 << 24) + 1)], dtype=np.int64).astype(np.int32)
    rs = np.exp(rng.uniform(-9.0, -2.0, size=M)).astype(np.float32)
    cs = np.exp(rng.uniform(-9.0, -2.0, size=N)).astype(np.float32)
    bias = bf16.bf16_round(rng.standard_normal(N).astype(np.float32))
    zp = rng.integers(-128, 128, size=M).astype(np.int8)
    wsum = rng.integers(-500000, 500000, size=N).astype(np.int32)
    return acc, rs, cs, bias, zp, wsum


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N", ARITH_SHAPES)
def test_the_int8_epilogues_match_the_oracle_on_any_accumulator(M, N, with_bias):
    lib = _lib.lib()
    acc, rs, cs, bias, zp, wsum = arith_case(M, N, 31 * M + N)
    b = bias if with_bias else None
    bd = dev_bf16(bias) if with_bias else None
    bp = bd.data_ptr() if with_bias else None
    accd, rsd, csd, zpd, wsd = dev(acc), dev(rs), dev(cs), dev(zp), dev(wsum)
    buf = _parity.Guarded(M, N, torch.bfloat16, DEV)
    _lib.check(lib.ao_int8_scale_epilogue(accd.data_ptr(), rsd.data_ptr(), csd.data_ptr(), bp, buf.out.data_ptr(), M, N, stream()))
    torch.cuda.synchronize()
    _parity.check(buf, ref_bits=dev_bf16(I8.scale_epilogue(acc, rs, cs, b)))
    buf = _parity.Guarded(M, N, torch.bfloat16, DEV)
    _lib.check(lib.ao_int8_scale_epilogue_asym(accd.data_ptr(), rsd.data_ptr(), zpd.data_ptr(), wsd.data_ptr(), csd.data_ptr(), bp, buf.out.data_ptr(), M, N,
                                               stream()))
    torch.cuda.synchronize()
    _parity.check(buf, ref_bits=dev_bf16(I8.scale_epilogue_asym(acc, rs, zp, wsum, cs, b)))
    # the Python wrappers, same bits
    assert torch.equal(ops.int8_scale_epilogue(accd, rsd, csd, bd), dev_bf16(I8.scale_epilogue(acc, rs, cs, b)))
    assert torch.equal(ops.int8_scale_epilogue_asym(accd, rsd, zpd, wsd, csd, bd), dev_bf16(I8.scale_epilogue_asym(acc, rs, zp, wsum, cs, b)))


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N", ARITH_SHAPES)
def test_the_fp8_epilogue_stays_inside_what_three_fp32_roundings_allow(M, N, with_bias):
    """The kernel computes c * sr * sc (+ bias) in fp32 and the compiler may fuse the add, so there is no single fp32 restatement.  With
    r = c sr sc + bias in float64 and d = 3 * 2^-24 (|c sr sc| + |bias|), the bound of three fp32 roundings, the fp32 value the kernel
    rounds to bf16 lies in [r - d, r + d]; rounding is monotone, so bf16(r - d) <= y <= bf16(r + d) is exactly what a correct kernel can
    give."""
    lib = _lib.lib()
    acc, rs, cs, bias, _, _ = arith_case(M, N, 77 * M + N)
    rng = np.random.default_rng(M)
    c = (acc.astype(np.float32) * rng.uniform(0.5, 1.0, size=acc.shape).astype(np.float32)).astype(np.float32)  # fp32 sums are no integers
    bd = dev_bf16(bias) if with_bias else None
    cd, rsd, csd = dev(c), dev(rs), dev(cs)
    buf = _parity.Guarded(M, N, torch.bfloat16, DEV)
    _lib.check(lib.ao_fp8_scale_epilogue(cd.data_ptr(), rsd.data_ptr(), csd.data_ptr(), bd.data_ptr() if with_bias else None, buf.out.data_ptr(), M, N,
                                         stream()))
    torch.cuda.synchronize()
    assert not _parity.problems(buf, ref_bits=buf.bits().clone()), _parity.problems(buf, ref_bits=buf.bits().clone())  # guards, nothing unwritten
    y = buf.out.float().cpu().numpy().astype(np.float64)
    p = c.astype(np.float64) * rs[:, None].astype(np.float64) * cs[None, :].astype(np.float64)
    b64 = bias[None, :].astype(np.float64) if with_bias else np.zeros((1, N))
    r = p + b64
    d = 3.0 * 2.0 ** -24 * (np.abs(p) + np.abs(b64))
    lo = bf16.bf16_round((r - d).astype(np.float32)).astype(np.float64)
    hi = bf16.bf16_round((r + d).astype(np.float32)).astype(np.float64)
    nearest = float(np.mean(y == bf16.bf16_round(r.astype(np.float32)).astype(np.float64)))
    bad = np.argwhere(~((lo <= y) & (y <= hi)))
    assert bad.size == 0, "%d elements outside [bf16(r - d), bf16(r + d)], first at %s: y=%r r=%r d=%r; %.4f of all elements equal bf16(r)" % (
        len(bad), tuple(bad[0]), y[tuple(bad[0])], r[tuple(bad[0])], d[tuple(bad[0])], nearest)
    assert torch.equal(ops.fp8_scale_epilogue(cd, rsd, csd, bd), buf.out)


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("M,N", ARITH_SHAPES)
def test_the_epilogue_wrappers_take_a_rank_s_rows_of_the_accumulator(M, N, world):
    """What RowParallelLinear's reduce-scatter path hands them: a row slice of the accumulator and of the activation scale."""
    acc, rs, cs, bias, _, _ = arith_case(M, N, 5 * M + N)
    accd, rsd, csd, bd = dev(acc), dev(rs).reshape(M, 1), dev(cs), dev_bf16(bias)
    accf = accd.float() * 0.75
    full8, fullf = ops.int8_scale_epilogue(accd, rsd, csd, bd), ops.fp8_scale_epilogue(accf, rsd, csd, bd)
    rows = M // world
    for rank in range(world):
        r0 = rank * rows
        assert torch.equal(ops.int8_scale_epilogue(accd[r0:r0 + rows], rsd[r0:r0 + rows], csd, bd), full8[r0:r0 + rows]), (rank, "int8")
        assert torch.equal(ops.fp8_scale_epilogue(accf[r0:r0 + rows], rsd[r0:r0 + rows], csd, bd), fullf[r0:r0 + rows]), (rank, "fp8")
        assert torch.equal(ops.int8_scale_epilogue(accd[r0:r0 + rows], rsd[r0:r0 + rows], csd), ops.int8_scale_epilogue(accd, rsd, csd)[r0:r0 + rows])


# ---- 3. static, asymmetric and per-tensor casts, the row sums ---------------------------------------------------------------------------
def static_ref(x, scale, zp):
    """clip(rint(x * f32(1 / scale)) + zp, -128, 127) in fp32; scale / zp of 1 or M entries"""
    inv = (np.float32(1.0) / np.asarray(scale, np.float32)).astype(np.float32).reshape(-1, 1)
    z = np.zeros((1, 1), np.float32) if zp is None else np.asarray(zp, np.float32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        q = np.rint((x * inv).astype(np.float32)).astype(np.float32) + z
    return np.clip(q, -128, 127).astype(np.int8)


def static_call(x, scale, zp, per_row):
    lib = _lib.lib()
    M, K = x.shape
    xd, sd = dev_bf16(x), dev(np.asarray(scale, np.float32).reshape(-1))
    zd = dev(np.asarray(zp, np.int8).reshape(-1)) if zp is not None else None
    q = Out(M * K, np.int8)
    _lib.check(lib.ao_int8_quantize_static(xd.data_ptr(), sd.data_ptr(), zd.data_ptr() if zp is not None else None, per_row, q.ptr, M, K, stream()))
    torch.cuda.synchronize()
    return q.get().reshape(M, K), xd, sd, zd


@pytest.mark.parametrize("with_zp", [False, True])
@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("K", [8, 2056, 16392])
def test_the_static_cast_with_given_scales_and_zero_points(K, per_row, with_zp):
    for M in (1, 5):
        rng = np.random.default_rng(K + 10 * M + per_row)
        n = M if per_row else 1
        scale = np.exp(rng.uniform(-4.0, 1.0, size=n)).astype(np.float32)
        scale[0] = 0.25  # a power of two: the half-integers below land on ties
        x = rng.standard_normal((M, K)).astype(np.float32) * 40.0
        x[:, :8] = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, -127.5], np.float32) * 0.25
        x = bf16.bf16_round(x)
        zp = rng.integers(-128, 128, size=n).astype(np.int8) if with_zp else None
        want = static_ref(x, scale, zp)
        got, xd, sd, zd = static_call(x, scale, zp, per_row)
        assert np.array_equal(got, want), (M, K, per_row, with_zp)
        # the wrapper: per-row scales of a single row go the per-tensor (stride 0) way
        assert np.array_equal(ops.int8_quantize_static(xd, sd, zd).cpu().numpy(), want), ("ops", M, K, per_row, with_zp)


@pytest.mark.parametrize("zp", [-128, 0, 127])
@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_the_static_cast_of_every_bf16_value(scale, zp):
    x = every_bf16_value()
    want = static_ref(x, [scale], [zp])
    got, _, _, _ = static_call(x, [scale], [zp], 0)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d codes differ, first bf16 pattern 0x%04x: %d vs %d" % (len(bad), bad[0][0] * 256 + bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (want == 127).any() and (want == -128).any()


ASYM_KINDS = ["positive", "negative", "zero", "constant", "gaussian", "huge"]


def asym_row(kind, K, rng):
    g = rng.standard_normal(K).astype(np.float32) * np.float32(2.0 ** int(rng.integers(-10, 11)))
    if kind == "positive":
        g = np.abs(g) + np.float32(0.125)
    elif kind == "negative":
        g = -np.abs(g) - np.float32(0.125)
    elif kind == "zero":
        g[:] = 0.0
    elif kind == "constant":
        g[:] = 0.37
    elif kind == "huge":  # mx - mn overflows, in the oracle's fp32 as in the kernel's: whatever that arithmetic gives is expected
        g[K // 3], g[K - 1] = POISON, -POISON
    return bf16.bf16_round(g)


@pytest.mark.parametrize("K", [8, 24, 1000, 2056, 16392, 40000])
def test_the_asymmetric_cast_matches_the_oracle(K):
    rng = np.random.default_rng(K)
    six = np.stack([asym_row(kind, K, rng) for kind in ASYM_KINDS])
    for x in [six] + [six[i:i + 1] for i in range(6)]:  # M = 6, and M = 1 of every kind
        with np.errstate(all="ignore"):
            wq, ws, wz = I8.quantize_rowwise_asym(x)
        q, s, z = ops.int8_quantize_rowwise_asym(dev_bf16(x))
        what = (K, x.shape[0], ASYM_KINDS)
        assert np.array_equal(u32(s.flatten().cpu().numpy()), u32(ws)), ("scale", s.flatten().cpu().numpy(), ws) + what
        assert np.array_equal(z.flatten().cpu().numpy(), wz), ("zero point", z.flatten().cpu().numpy(), wz) + what
        assert np.array_equal(q.cpu().numpy(), wq), ("codes", np.argwhere(q.cpu().numpy() != wq)[:4]) + what


def test_the_asymmetric_cast_stays_inside_its_outputs():
    lib = _lib.lib()
    M, K = 6, 2056
    rng = np.random.default_rng(9)
    x = np.stack([asym_row(kind, K, rng) for kind in ASYM_KINDS])
    with np.errstate(all="ignore"):
        wq, ws, wz = I8.quantize_rowwise_asym(x)
    xd = dev_bf16(x)
    q, s, z = Out(M * K, np.int8), Out(M, np.float32), Out(M, np.int8)
    _lib.check(lib.ao_int8_quantize_rowwise_asym(xd.data_ptr(), q.ptr, s.ptr, z.ptr, M, K, stream()))
    torch.cuda.synchronize()
    assert np.array_equal(q.get().reshape(M, K), wq) and np.array_equal(u32(s.get()), u32(ws)) and np.array_equal(z.get(), wz)


@pytest.mark.parametrize("M,K", [(1, 8), (3, 2056), (130, 16392)])
def test_the_per_tensor_casts_find_a_maximum_in_the_last_element(M, K):
    x = rows_of_many_magnitudes(M, K, M + K) * np.float32(2.0 ** -20)  # |x| < 8
    x[M - 1, K - 1] = -16.0  # the tensor's amax, in the last element of the last row
    assert bf16.is_bf16(x) and np.abs(x).max() == 16.0 and np.abs(x.reshape(-1)[:-1]).max() < 16.0
    xd = dev_bf16(x)
    wq, ws = I8.quantize_tensorwise(x)
    q, s = ops.int8_quantize_tensorwise(xd)
    assert tuple(s.shape) == (1, 1) and u32(s.cpu().numpy())[0, 0] == u32(ws) and np.array_equal(q.cpu().numpy(), wq)
    wq, ws = F8.quantize_tensorwise(x)
    q, s = ops.fp8_quantize_tensorwise(xd)
    assert tuple(s.shape) == (1, 1) and u32(s.cpu().numpy())[0, 0] == u32(ws)
    same_fp8(q.view(torch.uint8).cpu().numpy(), wq, (M, K))


@pytest.mark.parametrize("K", [16, 32, 1008, 16400])
@pytest.mark.parametrize("N", [1, 3, 5, 130])
def test_the_row_sums_are_the_integer_sums(N, K):
    """One wave per row, four rows per block: N that is no multiple of 4 leaves waves without a row."""
    lib = _lib.lib()
    rng = np.random.default_rng(N * 100000 + K)
    fills = [None] if N >= 3 else [None, -128, 127]
    for fill in fills:
        w = rng.integers(-128, 128, size=(N, K)).astype(np.int8)
        if N >= 3:
            w[0], w[N - 1] = -128, 127
        if fill is not None:
            w[:] = fill
        wd = dev(w)
        out = Out(N, np.int32)
        _lib.check(lib.ao_int8_row_sums(wd.data_ptr(), out.ptr, N, K, stream()))
        torch.cuda.synchronize()
        want = w.astype(np.int64).sum(axis=1)
        assert np.array_equal(out.get().astype(np.int64), want), (N, K, fill)
        assert np.array_equal(ops.int8_row_sums(wd).cpu().numpy().astype(np.int64), want)


# ---- 4. the rank-local chain of the row-parallel protocol in one graph ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int8", "fp8"])
def test_the_rank_local_chain_can_be_captured_in_a_graph(kind):
    """rowwise_amax -> cast with that amax -> unscaled GEMM -> scale epilogue on a window of a wider matrix, captured on one stream and
    replayed on new values: the bits of the eager calls.  (K = 2064: the GEMMs take multiples of 16, and 2064 / 8 = 258 vectors is two per
    thread with a ragged last one, like 2056.)"""
    M, N, K, W, c0 = 17, 256, 2064, 2064 + 264, 128
    cast = ops.int8_quantize_rowwise_amax if kind == "int8" else ops.fp8_quantize_rowwise_amax
    mm = ops.int_mm if kind == "int8" else ops.fp8_mm_f32
    epilogue = ops.int8_scale_epilogue if kind == "int8" else ops.fp8_scale_epilogue
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    wq, ws = (ops.int8_quantize_rowwise if kind == "int8" else ops.fp8_quantize_rowwise)(w)
    wt = wq.t()
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(DEV)
    first = wide_with_window(rows_of_many_magnitudes(M, K, 1), W, c0)[0]
    second = wide_with_window(rows_of_many_magnitudes(M, K, 2), W, c0)[0]
    wide = first.clone()
    view = wide[:, c0:c0 + K]

    def chain():
        a = ops.rowwise_amax(view)
        q, s = cast(view, a)
        return a, q, s, epilogue(mm(q, wt), s, ws, bias)

    y_first = chain()[3].clone()  # warm: the allocator's pools, the GEMM's workspace
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = chain()
        wide.copy_(second)
        graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    eager = chain()
    torch.cuda.synchronize()
    for name, got, want in zip(("amax", "codes", "scale", "y"), replayed, eager):  # (bits: the zero row's 0 / 0 makes NaNs of the fp8 chain)
        assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), name
    # (and the replay did see the new values)
    assert torch.equal(replayed[0], second[:, c0:c0 + K].float().abs().amax(dim=1)) and not torch.equal(replayed[3].view(torch.int16), y_first.view(torch.int16))
