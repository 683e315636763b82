"""GPU: the training casts (float8 rowwise / jagged, blockwise float8, MXFP8 row+col, NVFP4 RHT) at every launch form, past one trip of a
grid-stride loop, under every bf16 amax and on every bf16 value -- bit for bit against the restatements the fixtures pin to the reference
(tests/fp8_training_ref.py, fp8_grouped_training_ref.py, blockwise_fp8_training_ref.py, nvfp4_train_ref.py, oracle/mx_ref.py).  The
inputs are built, and their reach is checked on the CPU, in tests/training_cast_cases.py and tests/test_training_casts_host.py.

Every output of a C entry point is a _parity.Guarded poisoned buffer: 256 guard bytes before it, 16 guard rows after it, checked after
each call.  No comparison has a tolerance.

  1. test_the_one_launch_row_cast_*        fp8_train_quant_rowwise_kernel<1 | 2 | 4 | 8 | 0>, full and ragged, the maximum in the row's
                                           last and first vector
  2. test_the_nvfp4_amax_*, test_an_nvfp4_cast_of_17_x_3_tiles   the second trip of nvfp4_train_amax_kernel's loop; the SR counter past
                                           the first tiles
  3. test_every_amax_*                     the 32 640 non-negative finite bf16 as the amax of a row, column, group, block
  4. test_every_value_*                    the 65 536 bf16 patterns (non-finite ones zeroed: outside the contract) through every cast
Measured on an MI355X: 76 tests in 3.2 s, the slowest 0.3 s (profiles/pytest_gpu_training_casts.log).
"""
import numpy as np
import pytest
import torch

import _parity
import fp8_grouped_training_ref as G
import blockwise_fp8_training_ref as B
import fp8_training_ref as R
import nvfp4_train_ref as T
import training_cast_cases as K
from ao_amd import _lib, ops
from oracle import mx_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
MASK = ops.nvfp4_sign_mask(K.SIGN)


def _device():
    return torch.device(DEV, 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _x(xb):
    """bf16 bit patterns -> a bf16 tensor on the device"""
    return K.t_bf16(xb).to(DEV)


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


class Out:
    """A guarded, poisoned output of a C entry point: uint8 or fp32 [rows, cols]."""

    def __init__(self, rows, cols, f32=False):
        self.rows, self.cols, self.f32 = rows, cols, f32
        if f32:
            self.g = _parity.Guarded(rows, cols, torch.float32, _device())
        elif cols % 2 == 0:
            self.g = _parity.Guarded(rows, cols // 2, torch.bfloat16, _device())
        else:  # (an odd row of bytes: the small scale arrays)
            assert rows * cols % 2 == 0
            self.g = _parity.Guarded(1, rows * cols // 2, torch.bfloat16, _device())
        self.ptr = self.g.out.data_ptr()

    def get(self):
        """the output as numpy (uint8, or the fp32 bits as uint32) once the guards are seen untouched"""
        torch.cuda.synchronize()
        msgs = self.g.guard_problems()
        assert not msgs, "; ".join(msgs)
        raw = self.g.bits().contiguous().view(torch.uint8).reshape(-1).cpu().numpy()
        return (raw.view(np.uint32) if self.f32 else raw).reshape(self.rows, self.cols)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: %#x vs %#x" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                         want[tuple(bad[0])])


# ---- the C entry points on guarded outputs -------------------------------------------------------------------------------------------------
def c_fp8_rowwise(x, pow2):
    r, c = x.shape
    q, s, inv = Out(r, c), Out(r, 1, True), Out(r, 1, True)
    _lib.check(_lib.lib().ao_fp8_train_quantize_rowwise(x.data_ptr(), q.ptr, s.ptr, inv.ptr, int(pow2), r, c, _stream()))
    return q.get(), s.get(), inv.get()


def c_fp8_amax(x, rows=True, cols=False):
    r, c = x.shape
    ra, ca = (Out(r, 1, True) if rows else None), (Out(1, c, True) if cols else None)
    _lib.check(_lib.lib().ao_fp8_train_amax(x.data_ptr(), ra.ptr if rows else None, ca.ptr if cols else None, r, c, _stream()))
    return ra, ca


def c_fp8_cast(x, row_amax, col_amax, pow2):
    """row_amax / col_amax: None, an Out of one amax a row / column (stride 1) or a 0-d fp32 tensor (stride 0) -> (rows, cols), each
    (q, s, inv) or None"""
    r, c = x.shape
    ptr = lambda a: None if a is None else (a.ptr if isinstance(a, Out) else a.data_ptr())  # noqa: E731
    stride = lambda a: int(isinstance(a, Out))  # noqa: E731
    rows = (Out(r, c), Out(r, 1, True), Out(r, 1, True)) if row_amax is not None else (None, None, None)
    cols = (Out(c, r), Out(c, 1, True), Out(c, 1, True)) if col_amax is not None else (None, None, None)
    p = [None if o is None else o.ptr for o in rows + cols]
    _lib.check(_lib.lib().ao_fp8_train_cast(x.data_ptr(), ptr(row_amax), stride(row_amax), ptr(col_amax), stride(col_amax), int(pow2), *p, r, c,
                                            _stream()))
    return tuple(None if t[0] is None else tuple(o.get() for o in t) for t in (rows, cols))


def c_fp8_group(x, offs, pow2):
    r, c = x.shape
    e = offs.numel()
    qt, s, inv = Out(c, r), Out(e, c, True), Out(e, c, True)
    _lib.check(_lib.lib().ao_fp8_train_quantize_group_colwise_t(x.data_ptr(), offs.data_ptr(), qt.ptr, s.ptr, inv.ptr, int(pow2), r, c, e, _stream()))
    return qt.get(), s.get(), inv.get()


def c_block_cast(x, rows=True, cols=False):
    r, c = x.shape
    q, inv = (Out(r, c), Out(r, c // 128, True)) if rows else (None, None)
    qt, invt = (Out(c, r), Out(r // 128, c, True)) if cols else (None, None)
    p = [None if o is None else o.ptr for o in (q, inv, qt, invt)]
    _lib.check(_lib.lib().ao_fp8_block_train_cast(x.data_ptr(), *p, r, c, _stream()))
    return tuple(None if o is None else o.get() for o in (q, inv, qt, invt))


def c_block_weight(w):
    """both pairs from one read: (q [N, K], inv [N/128, K/128], q_t [K, N], inv_t [K/128, N/128])"""
    n, k = w.shape
    outs = (Out(n, k), Out(n // 128, k // 128, True), Out(k, n), Out(k // 128, n // 128, True))
    _lib.check(_lib.lib().ao_fp8_block_train_cast_weight(w.data_ptr(), *[o.ptr for o in outs], n, k, _stream()))
    return tuple(o.get() for o in outs)


def c_mx_rows(x, mode):
    r, c = x.shape
    q, s = Out(r, c), Out(r, c // 32)
    _lib.check(_lib.lib().ao_mxfp8_quantize_rowwise(x.data_ptr(), q.ptr, s.ptr, r, c, mode, _stream()))
    return q.get(), s.get()


def c_mx_cols(x, mode):
    r, c = x.shape
    qt, s = Out(c, r), Out(r // 32, c)
    _lib.check(_lib.lib().ao_mxfp8_quantize_colwise(x.data_ptr(), qt.ptr, s.ptr, r, c, mode, _stream()))
    return qt.get(), s.get()


def c_mx_rowcol(x, mode):
    r, c = x.shape
    outs = (Out(r, c), Out(r, c // 32), Out(c, r), Out(r // 32, c))
    _lib.check(_lib.lib().ao_mxfp8_quantize_rowcol(x.data_ptr(), *[o.ptr for o in outs], r, c, mode, _stream()))
    return tuple(o.get() for o in outs)


def c_nvfp4_amax(x, want_rht):
    m, n = x.shape
    out = Out(1, 2, True)
    _lib.check(_lib.lib().ao_nvfp4_train_amax(x.data_ptr(), out.ptr, m, n, MASK, int(want_rht), _stream()))
    return out.get().reshape(2)


def _i64(v):
    v = int(v) & (2 ** 64 - 1)
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v], dtype=torch.int64, device=DEV)


def c_nvfp4_row_col(x, amax2, sr=None, want_col=True):
    """sr = (seed, column offset, row offset) or None -> (col_q, col_s, row_q, row_s), the column pair None when not wanted"""
    m, n = x.shape
    a = torch.as_tensor(amax2, dtype=torch.float32).reshape(2).to(DEV)
    col = (Out(n, m // 2), Out(n, m // 16)) if want_col else (None, None)
    row = (Out(m, n // 2), Out(m, n // 16))
    keep = [None, None, None] if sr is None else [_i64(v) for v in sr]
    p = [None if o is None else o.ptr for o in col + row]
    _lib.check(_lib.lib().ao_nvfp4_train_quantize_row_col(x.data_ptr(), a.data_ptr(), MASK, *[None if t is None else t.data_ptr() for t in keep],
                                                          *p, m, n, _stream()))
    return tuple(None if o is None else o.get() for o in col + row)


def c_nvfp4_weight(w, amax):
    n, k = w.shape
    a = torch.as_tensor(amax, dtype=torch.float32).reshape(1).to(DEV)
    outs = (Out(n, k // 2), Out(n, k // 16), Out(k, n // 2), Out(k, n // 16))
    _lib.check(_lib.lib().ao_nvfp4_train_quantize_weight_2d(w.data_ptr(), a.data_ptr(), *[o.ptr for o in outs], n, k, _stream()))
    return tuple(o.get() for o in outs)


def _np(ts):
    return tuple(t.numpy() for t in ts)


# ---- 1. every launch form of the one-launch row cast ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_", K.ROW_R)
@pytest.mark.parametrize("C", K.ROW_C)
def test_the_one_launch_row_cast_equals_the_restatement_and_the_two_call_form(C, R_):
    for plant in ("last", "first"):
        xb = K.row_case(R_, C, plant)
        x = _x(xb)
        for pow2 in (0, 1):
            what = "C=%d (depth %d) R=%d plant=%s pow2=%d" % (C, K.row_depth(C), R_, plant, pow2)
            wq, ws, winv = R.cast(xb, -1, bool(pow2))
            q, s, inv = c_fp8_rowwise(x, pow2)
            _same(s, _u32(ws), what + ": scale")
            _same(inv, _u32(winv), what + ": reciprocal")
            _same(q, wq, what + ": codes")
            ra, _ = c_fp8_amax(x)
            (q2, s2, inv2), none = c_fp8_cast(x, ra, None, pow2)
            assert none is None
            _same(q2, q, what + ": amax + cast codes")
            _same(s2, s, what + ": amax + cast scale")
            _same(inv2, inv, what + ": amax + cast reciprocal")


# ---- 2. the NVFP4 amax past one trip of its grid, and a cast past the first tiles -------------------------------------------------------------
@pytest.mark.parametrize("m,n,plant", [(m, n, p) for m, n in K.AMAX_SHAPES for p in K.amax_plants(m, n)])
def test_the_nvfp4_amax_finds_a_unit_in_any_trip_of_its_loop(m, n, plant):
    xc, with_rht, without = K.amax_case(m, n, plant)
    assert float(without[1]) == 200.0 and float(with_rht[0]) > 16.0  # the planted unit decides both (the rest: |x| <= 1, transform <= 4)
    x = xc.to(DEV)
    _same(c_nvfp4_amax(x, True), with_rht.numpy().view(np.uint32), "%d x %d %s, with the transform" % (m, n, plant))
    _same(c_nvfp4_amax(x, False), without.numpy().view(np.uint32), "%d x %d %s, without" % (m, n, plant))
    assert float(without[0]) == 0.0


def test_an_nvfp4_cast_of_17_x_3_tiles_under_either_rounding_and_as_a_weight():
    m, n = K.NVFP4_CAST_SHAPE
    xc = K.nvfp4_matrix(m, n, 2064)
    x = xc.to(DEV)
    amax2 = T.amaxes(xc, K.SIGN)
    _same(c_nvfp4_amax(x, True), amax2.numpy().view(np.uint32), "amax")
    names = ("col_q", "col_s", "row_q", "row_s")
    rne = c_nvfp4_row_col(x, amax2)
    for name, got, want in zip(names, rne, _np(T.quantize_row_col(xc, amax2, K.SIGN))):
        _same(got, want, "round to nearest even " + name)
    seed, co, ro = K.NVFP4_CAST_SR
    sr = c_nvfp4_row_col(x, amax2, (seed, co, ro))
    for name, got, want in zip(names, sr, _np(T.quantize_row_col(xc, amax2, K.SIGN, seed, co, ro))):
        _same(got, want, "stochastic rounding " + name)
    assert not np.array_equal(sr[0], rne[0]) and not np.array_equal(sr[2], rne[2])
    for name, got, want in zip(("q", "s", "qt", "st"), c_nvfp4_weight(x, amax2[1]), _np(T.quantize_weight_2d(xc, amax2[1]))):
        _same(got, want, "16 x 16 " + name)


# ---- 3. every amax -> scale ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pow2", [0, 1], ids=["plain", "pow2"])
def test_every_amax_through_the_fp8_row_casts(pow2):
    xb = K.amax_rows(16)
    x = _x(xb)
    ws = R.amax_to_scale(K.amax_values(), bool(pow2)).reshape(-1, 1)
    winv = (np.float32(1.0) / ws).astype(np.float32)
    wq, ws2, winv2 = R.cast(xb, -1, bool(pow2))
    assert np.array_equal(_u32(ws), _u32(ws2)) and np.array_equal(_u32(winv), _u32(winv2))
    q, s, inv = c_fp8_rowwise(x, pow2)
    _same(s, _u32(ws), "one launch: scale")
    _same(inv, _u32(winv), "one launch: reciprocal")
    _same(q, wq, "one launch: codes")
    ra, _ = c_fp8_amax(x)
    _same(ra.get(), _u32(K.amax_values()).reshape(-1, 1), "row amax")
    (q, s, inv), _ = c_fp8_cast(x, ra, None, pow2)
    _same(s, _u32(ws), "amax + cast: scale")
    _same(inv, _u32(winv), "amax + cast: reciprocal")
    _same(q, wq, "amax + cast: codes")


@pytest.mark.parametrize("pow2", [0, 1], ids=["plain", "pow2"])
def test_every_amax_through_the_transposing_fp8_cast(pow2):
    xb = np.ascontiguousarray(K.amax_rows(16).T)  # [16, 32640]: every column its amax
    x = _x(xb)
    wq, ws, winv = R.cast(xb, 0, bool(pow2))
    assert np.array_equal(_u32(ws).reshape(-1), _u32(R.amax_to_scale(K.amax_values(), bool(pow2))))
    _, ca = c_fp8_amax(x, rows=False, cols=True)
    _same(ca.get().reshape(-1), _u32(K.amax_values()), "column amax")
    _, (qt, s, inv) = c_fp8_cast(x, None, ca, pow2)
    _same(s.reshape(-1), _u32(ws).reshape(-1), "scale")
    _same(inv.reshape(-1), _u32(winv).reshape(-1), "reciprocal")
    _same(qt, wq.T, "codes")


@pytest.mark.parametrize("pow2", [0, 1], ids=["plain", "pow2"])
def test_every_amax_through_the_jagged_fp8_cast_of_2040_groups(pow2):
    xb, offs = K.amax_groups()
    wq, ws, winv = G.group_colwise(xb, offs, bool(pow2))
    assert np.array_equal(_u32(ws).reshape(-1), _u32(R.amax_to_scale(K.amax_values(), bool(pow2))))
    qt, s, inv = c_fp8_group(_x(xb), torch.from_numpy(offs).to(DEV), pow2)
    _same(s, _u32(ws), "scale")
    _same(inv, _u32(winv), "reciprocal")
    _same(qt, wq.T, "codes")


def test_every_amax_through_the_blockwise_1_x_128_cast():
    xb = K.amax_rows(128)
    wq, winv, ws = B.cast_rows(xb)
    assert np.array_equal(_u32(ws).reshape(-1), _u32(B.scale_of(K.amax_values())))
    q, inv, _, _ = c_block_cast(_x(xb))
    _same(inv, _u32(B._inv(B.scale_of(K.amax_values()))).reshape(-1, 1), "reciprocal")
    _same(q, wq, "codes")


def test_every_exponent_of_amax_through_the_blockwise_128_x_128_cast():
    """2 040 blocks stacked [2040 * 128, 128] (67 MB): the reciprocals of both outputs, and the codes (the blocks are zeros but for six
    values, so the expected codes are the restatement's cast of those six under the block's scale)."""
    wb = K.weight_blocks()
    nb = wb.shape[0] // 128
    scale = B.scale_of(K.f32(K.weight_block_amaxes()))
    winv = B._inv(scale)
    q, inv, qt, invt = c_block_weight(_x(wb))
    _same(inv, _u32(winv).reshape(nb, 1), "reciprocal")
    _same(invt, _u32(winv).reshape(1, nb), "reciprocal, transposed")
    blocks = wb.reshape(nb, 128 * 128)
    rows, cols = np.nonzero(blocks)
    wq = np.zeros(blocks.shape, dtype=np.uint8)
    wq[rows, cols] = B._codes(K.f32(blocks[rows, cols]), scale[rows])
    wq = wq.reshape(nb * 128, 128)
    _same(q, wq, "codes")
    _same(qt, wq.T, "codes, transposed")


@pytest.mark.parametrize("mode", [mx_ref.FLOOR, mx_ref.RCEIL], ids=["floor", "rceil"])
def test_every_amax_through_the_mxfp8_casts(mode):
    xb = K.amax_rows(32)  # [32640, 32]: a block a row
    wq, we, _ = K.mx_rows(xb, mode)
    wqt, wet, _ = K.mx_cols(xb, mode)
    x = _x(xb)
    q, e = c_mx_rows(x, mode)
    _same(e, we, "rowwise: E8M0")
    _same(q, wq, "rowwise: codes")
    q, e, qt, et = c_mx_rowcol(x, mode)
    _same(e, we, "row+col: row E8M0")
    _same(q, wq, "row+col: row codes")
    _same(et, wet, "row+col: column E8M0")
    _same(qt, wqt, "row+col: column codes")
    # the transpose [32, 32640]: a block a column
    xt = _x(np.ascontiguousarray(xb.T))
    qt, et = c_mx_cols(xt, mode)
    _same(et, we.T, "colwise: E8M0")
    _same(qt, wq, "colwise: codes")
    q2, e2, qt2, et2 = c_mx_rowcol(xt, mode)
    _same(et2, we.T, "row+col of the transpose: column E8M0")
    _same(qt2, wq, "row+col of the transpose: column codes")
    _same(e2, wet.T, "row+col of the transpose: row E8M0")
    _same(q2, wqt, "row+col of the transpose: row codes")


@pytest.mark.parametrize("amax_bits", K.NVFP4_TENSOR_AMAX_BITS, ids=["%#06x" % b for b in K.NVFP4_TENSOR_AMAX_BITS])
def test_every_block_amax_through_the_nvfp4_cast(amax_bits):
    xb = K.amax_rows(16)  # [32640, 16]: a block a row
    amax = float(K.f32(np.array([amax_bits], dtype=np.uint16))[0])
    wq, ws = _np(T.cast(K.t_bf16(xb), amax))
    _, _, q, s = c_nvfp4_row_col(_x(xb), (amax, amax), want_col=False)
    _same(s, ws, "scale bytes")
    _same(q, wq, "codes")


# ---- 4. every bf16 value -> code -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amax", K.FP8_GIVEN_AMAX, ids=["%.3g" % a for a in K.FP8_GIVEN_AMAX])
def test_every_value_through_the_fp8_cast_under_a_given_amax(amax):
    xb = K.all_values()
    x = _x(xb)
    a = torch.tensor(amax, dtype=torch.float32, device=DEV)  # 0-d: the tensor's one amax, stride 0
    for pow2 in (0, 1):
        wq, ws, _ = K.fp8_given(xb, amax, bool(pow2))
        winv = (np.float32(1.0) / ws).astype(np.float32)
        (q, s, inv), (qt, st, invt) = c_fp8_cast(x, a, a, pow2)
        for got in (s, st):
            _same(got, np.full((256, 1), _u32(ws)), "scale")
        for got in (inv, invt):
            _same(got, np.full((256, 1), _u32(winv)), "reciprocal")
        _same(q, wq, "pow2=%d: codes" % pow2)
        _same(qt, wq.T, "pow2=%d: transposed codes" % pow2)


@pytest.mark.parametrize("sr", [None, K.NVFP4_VALUES_SR], ids=["rne", "sr"])
@pytest.mark.parametrize("amax", K.NVFP4_GIVEN_AMAX, ids=["%.3g" % a for a in K.NVFP4_GIVEN_AMAX])
def test_every_value_through_the_nvfp4_cast_under_a_given_amax(amax, sr):
    xb = K.row_blocks(16)
    xc = K.t_bf16(xb)
    want = T.quantize_row_col(xc, torch.tensor([amax, amax]), K.SIGN, *((None, 0, 0) if sr is None else sr))
    got = c_nvfp4_row_col(_x(xb), (amax, amax), sr)
    for name, g, w in zip(("col_q", "col_s", "row_q", "row_s"), got, _np(want)):
        _same(g, w, name)


@pytest.mark.parametrize("pow2", [0, 1], ids=["plain", "pow2"])
def test_every_value_through_the_fp8_casts_that_find_their_amax(pow2):
    xb = K.row_blocks(128)
    x = _x(xb)
    wq, ws, winv, _ = K.fp8_rowwise(xb, bool(pow2))
    q, s, inv = c_fp8_rowwise(x, pow2)
    _same(s, _u32(ws), "rowwise: scale")
    _same(inv, _u32(winv), "rowwise: reciprocal")
    _same(q, wq, "rowwise: codes")
    ra, ca = c_fp8_amax(x, rows=True, cols=True)
    (q, s, inv), (qt, st, invt) = c_fp8_cast(x, ra, ca, pow2)
    _same(q, wq, "amax + cast: row codes")
    _same(s, _u32(ws), "amax + cast: row scale")
    cq, cs, cinv = R.cast(xb, 0, bool(pow2))
    _same(qt, cq.T, "amax + cast: column codes")
    _same(st.reshape(-1), _u32(cs).reshape(-1), "amax + cast: column scale")
    _same(invt.reshape(-1), _u32(cinv).reshape(-1), "amax + cast: column reciprocal")


def test_every_value_through_the_blockwise_casts():
    for name, xb in (("1 x 128 blocks in rows", K.row_blocks(128)), ("128 x 1 blocks in columns", K.col_blocks(128))):
        wq, winv, _ = B.cast_rows(xb)
        wqt, winvt, _ = B.cast_cols(xb)
        q, inv, qt, invt = c_block_cast(_x(xb), rows=True, cols=True)
        _same(inv, _u32(winv), name + ": row reciprocals")
        _same(q, wq, name + ": row codes")
        _same(invt, _u32(winvt), name + ": column reciprocals")
        _same(qt, wqt, name + ": column codes")
    for name, wb in (("quadrants", K.weight_quadrants()), ("row blocks", K.row_blocks(128))):
        wq, winv, _ = B.cast_weight(wb)
        q, inv, qt, invt = c_block_weight(_x(wb))
        _same(inv, _u32(winv), name + ": 128 x 128 reciprocals")
        _same(invt, _u32(winv).T, name + ": 128 x 128 reciprocals, transposed")
        _same(q, wq, name + ": 128 x 128 codes")
        _same(qt, wq.T, name + ": 128 x 128 codes, transposed")


@pytest.mark.parametrize("mode", [mx_ref.FLOOR, mx_ref.RCEIL], ids=["floor", "rceil"])
def test_every_value_through_the_mxfp8_row_col_cast(mode):
    for name, xb in (("blocks in rows", K.row_blocks(32)), ("blocks in columns", K.col_blocks(32))):
        wq, we, _ = K.mx_rows(xb, mode)
        wqt, wet, _ = K.mx_cols(xb, mode)
        q, e, qt, et = c_mx_rowcol(_x(xb), mode)
        _same(e, we, name + ": row E8M0")
        _same(q, wq, name + ": row codes")
        _same(et, wet, name + ": column E8M0")
        _same(qt, wqt, name + ": column codes")
