"""CPU: blockwise float8 training -- the numpy restatement of the three casts against the fixture written from the reference's torch
functions (tests/golden/blockwise_fp8_training.npz), byte for byte; the new symbols, ops and prototype names; every refusal with its
reason and no GPU; quantize_ with the config; the C entry points' argument checks (no kernel is launched in this file)."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch import nn

import blockwise_fp8_training_ref as R
from ao_amd import _lib, ops, prototype
from ao_amd.prototype.blockwise_fp8_training import Float8BlockwiseLinear, Float8BlockwiseLinearConfig, fp8_blockwise_mm
from ao_amd.quantization import quantize_

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ("ao_fp8_block_train_cast", "ao_fp8_block_train_cast_weight", "ao_fp8_block_mm_wgrad")
OPS = ("fp8_block_train_cast", "fp8_block_train_cast_weight", "fp8_block_mm_wgrad")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _load("make_golden_blockwise_fp8_training")


@functools.lru_cache(maxsize=None)
def fixture():
    return MAKER.load()


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _rows(G, t):
    return G[t].reshape(-1, G[t].shape[-1])


# ---- the casts ---------------------------------------------------------------------------------------------------------------------------
CASTS = [(t, "row") for t in MAKER.ROW] + [(t, "col") for t in MAKER.COL] + [(t, "blk") for t in MAKER.BLK]


@pytest.mark.parametrize("t,kind", CASTS, ids=["%s_%s" % c for c in CASTS])
def test_the_restatement_reproduces_every_recorded_cast(t, kind):
    G = fixture()
    xb = _rows(G, t)
    q, inv, s = {"row": R.cast_rows, "col": R.cast_cols, "blk": R.cast_weight}[kind](xb)
    if kind == "col":
        q = q.T  # the restatement stores the 128 x 1 cast transposed, the reference's function does not
    key = "%s_%s" % (t, kind)
    assert G[key + "_q"].shape == xb.shape and G[key + "_inv"].dtype == np.float32
    np.testing.assert_array_equal(q, G[key + "_q"])
    np.testing.assert_array_equal(_u32(inv), _u32(G[key + "_inv"]))
    np.testing.assert_array_equal(_u32(inv), _u32(1.0 / torch.from_numpy(s.copy())))  # torch's 1.0 / s


def test_the_fixture_holds_its_shapes_and_edge_cases():
    G = fixture()
    assert G["x"].shape == (2, 128, 256) and G["w"].shape == (128, 256) and G["go"].shape == (2, 128, 128) and G["edge"].shape == (256, 256)
    e = R.bf16.from_bits(G["edge"])
    big = np.float32(torch.finfo(torch.bfloat16).max)
    assert not e[3, :128].any() and not e[128:, 5].any() and not e[128:, 128:].any() and e[7, 139] == big
    assert 0 < e[4, 64] < 1e-19 and 0 < e[200, 6] < 1e-19
    # block maxima in a block's last row and last column
    assert np.abs(e[:128, :128]).max() == -e[127, 127] and np.abs(e[128:, :128]).max() == e[255, 127]
    # rows scaled by 2^-12 .. 2^12
    med = np.median(np.abs(e[:25, 128:]), axis=1)
    assert med[0] < 2.0 ** -11 and med[24] > 2.0 ** 10
    # a zero block: scale f32(448 / 1e-12), codes 0, no NaN -- and bf16(1e-12) as the floor of the 128 x 1 direction
    zero = np.float32(1.0) / np.float32(448.0 / 1e-12)
    assert G["edge_row_inv"][3, 0] == zero and G["edge_row_inv"][4, 0] == zero and G["edge_blk_inv"][1, 1] == zero
    col_zero = np.float32(1.0) / np.float32(448.0 / np.float64(R.EPS_BF16))
    assert G["edge_col_inv"][1, 5] == col_zero and G["edge_col_inv"][1, 6] == col_zero and col_zero != zero
    for k in G:
        if k.endswith("_q"):
            assert not np.any((G[k] & 0x7F) == 0x7F), k  # all codes finite
    assert G["edge_row_q"][7, 139] == 0x7E  # the largest bf16 lands on 448
    # the clamp is live: some |f32(x) * scale| rounds above 448
    over = 0
    for t in MAKER.ROW:
        xb = _rows(G, t)
        _, _, s = R.cast_rows(xb)
        over += int(np.sum(np.abs(R.bf16.from_bits(xb).astype(np.float32) * np.repeat(s, 128, axis=1)) > 448.0))
    assert over > 0


def test_a_blocks_codes_do_not_depend_on_the_layout():
    G = fixture()
    for t in MAKER.BLK:
        q, inv, _ = R.cast_weight(G[t])
        qt, invt, _ = R.cast_weight(np.ascontiguousarray(G[t].T))
        np.testing.assert_array_equal(qt, q.T)
        np.testing.assert_array_equal(_u32(invt), _u32(inv.T))


def test_the_wgrad_chain_equals_the_float64_sum_on_exact_operands():
    from oracle import fp8_ref

    g = np.random.default_rng(0)
    M, N, K = 256, 128, 128
    g_t = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (N, M)).astype(np.float32))
    x_t = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (K, M)).astype(np.float32))
    g_inv = np.exp2(g.integers(-2, 2, (M // 128, N))).astype(np.float32)
    x_inv = np.exp2(g.integers(-2, 3, (M // 128, K))).astype(np.float32)
    y, S = R.wgrad_f64(g_t, g_inv, x_t, x_inv)
    assert S.max() / 2.0 ** -4 < 2.0 ** 24
    want = R.bf16.to_bits(R.bf16.bf16_round(y.astype(np.float32)))
    np.testing.assert_array_equal(R.wgrad_chain_bits(g_t, g_inv, x_t, x_inv), want)


# ---- names ----------------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_ops_and_prototype_names_are_there():
    from ao_amd import torch_ops  # noqa: F401  (registers the ao_mi355 ops)

    names = _lib.declared_symbols()
    for n in SYMBOLS:
        assert n in names and n in _lib._SIGNATURES and hasattr(_lib.lib(), n), n
    for n in OPS:
        assert n in ops.__all__ and callable(getattr(ops, n)), n
        assert hasattr(torch.ops.ao_mi355, n), n
    for n in ("fp8_blockwise_mm", "Float8BlockwiseLinear", "Float8BlockwiseLinearConfig"):
        assert n in prototype.__all__ and hasattr(prototype, n), n
    text = open(_lib.HEADER_PATH).read()
    for cite in ("kernels.py:1031-1156", "kernels.py:320-379", "linear.py:98-211"):
        assert cite in text, cite


def test_the_fakes_give_the_shapes_of_the_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from ao_amd import torch_ops  # noqa: F401

    with FakeTensorMode():
        x = torch.empty(256, 384, dtype=torch.bfloat16, device="cuda")
        q, inv, qt, invt = torch.ops.ao_mi355.fp8_block_train_cast(x, True, True)
        assert (q.shape, inv.shape, qt.shape, invt.shape) == ((256, 384), (256, 3), (384, 256), (2, 384))
        assert q.dtype == qt.dtype == torch.float8_e4m3fn and inv.dtype == invt.dtype == torch.float32
        q, inv, qt, invt = torch.ops.ao_mi355.fp8_block_train_cast(x, False, True)
        assert q.numel() == inv.numel() == 0 and qt.shape == (384, 256)
        q, inv = torch.ops.ao_mi355.fp8_block_train_cast_weight(x, False)
        assert (q.shape, inv.shape) == ((256, 384), (2, 3))
        q, inv = torch.ops.ao_mi355.fp8_block_train_cast_weight(x, True)
        assert (q.shape, inv.shape) == ((384, 256), (3, 2))
        out = torch.ops.ao_mi355.fp8_block_mm_wgrad(qt, invt, qt[:128], invt[:, :128])
        assert out.shape == (384, 128) and out.dtype == torch.bfloat16


# ---- the C entry points -----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_check_their_arguments_on_the_host():
    lib = _lib.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first, and an empty matrix launches nothing
    inv, ok, null = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_OK, _lib.AO_ERR_NULL_POINTER
    cast = lambda r, c, qt=one: lib.ao_fp8_block_train_cast(one, one, one, qt, qt, r, c, None)  # noqa: E731
    wcast = lambda n, k: lib.ao_fp8_block_train_cast_weight(one, one, one, one, one, n, k, None)  # noqa: E731
    wgrad = lambda m, n, k: lib.ao_fp8_block_mm_wgrad(one, one, one, one, one, m, n, k, None)  # noqa: E731
    assert cast(128, 100) == inv and "C=100" in _lib.last_error() and "multiple of 128" in _lib.last_error()
    assert cast(5, 64, None) == inv and "C=64" in _lib.last_error()
    assert cast(130, 256) == inv and "R=130 must be a multiple of 128" in _lib.last_error()
    assert cast(-1, 128) == inv
    assert cast(128 * 65536, 128, None) == inv and "too large" in _lib.last_error()
    assert lib.ao_fp8_block_train_cast(one, None, None, None, None, 128, 128, None) == inv and "neither" in _lib.last_error()
    assert lib.ao_fp8_block_train_cast(None, one, one, None, None, 128, 128, None) == null
    assert lib.ao_fp8_block_train_cast(one, one, None, None, None, 128, 128, None) == null  # half a pair
    assert lib.ao_fp8_block_train_cast(ctypes.c_void_p(8), one, one, None, None, 128, 128, None) == inv and "aligned" in _lib.last_error()
    assert wcast(128, 100) == inv and "C=100" in _lib.last_error()
    assert wcast(100, 128) == inv and "R=100 must be a multiple of 128" in _lib.last_error()
    assert lib.ao_fp8_block_train_cast_weight(one, None, None, None, None, 128, 128, None) == inv and "neither" in _lib.last_error()
    assert lib.ao_fp8_block_train_cast_weight(one, None, None, one, None, 128, 128, None) == null
    for m, n, k, bad in ((100, 128, 128, "M=100"), (128, 100, 128, "N=100"), (128, 128, 100, "K=100")):
        assert wgrad(m, n, k) == inv and bad in _lib.last_error() and "multiples of 128" in _lib.last_error()
    assert wgrad(128, 0, 128) == inv and wgrad(128, 128, 0) == inv and wgrad(-128, 128, 128) == inv
    assert wgrad(1 << 24, 128, 128) == inv and "below 2^31" in _lib.last_error()  # an operand of 2 GiB
    assert lib.ao_fp8_block_mm_wgrad(one, one, one, one, None, 128, 128, 128, None) == null
    assert lib.ao_fp8_block_mm_wgrad(None, one, one, one, one, 128, 128, 128, None) == null
    # the empty cases
    for r, c in ((0, 128), (0, 0), (128, 0), (5, 0)):
        assert cast(r, c, None if r % 128 else one) == ok
    assert cast(0, 100) == inv  # the shape is checked before the matrix is found empty
    for n, k in ((0, 128), (128, 0), (0, 0)):
        assert wcast(n, k) == ok
    with pytest.raises(ValueError, match="R=130"):
        _lib.check(cast(130, 256))


# ---- the Python refusals, each before any GPU requirement ---------------------------------------------------------------------------------
def _bf(*shape, **kw):
    return torch.zeros(*shape, dtype=torch.bfloat16, **kw)


def test_the_ops_refuse_dtypes_ranks_and_shapes_before_the_library_is_touched():
    with pytest.raises(ValueError, match="fp8_block_train_cast: x must be a bfloat16 tensor"):
        ops.fp8_block_train_cast(torch.zeros(128, 128))
    with pytest.raises(ValueError, match="x must be 2-D"):
        ops.fp8_block_train_cast(_bf(2, 128, 128))
    with pytest.raises(ValueError, match="x has 100 columns.*multiple of 128"):
        ops.fp8_block_train_cast(_bf(128, 100))
    with pytest.raises(ValueError, match="x has 130 rows.*multiple of 128"):
        ops.fp8_block_train_cast(_bf(130, 128), rows=True, cols=True)
    with pytest.raises(ValueError, match="neither rows nor cols"):
        ops.fp8_block_train_cast(_bf(128, 128), rows=False, cols=False)
    with pytest.raises(ValueError, match="fp8_block_train_cast_weight: w must be a bfloat16 tensor"):
        ops.fp8_block_train_cast_weight(torch.zeros(128, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="w must be 2-D"):
        ops.fp8_block_train_cast_weight(_bf(128))
    with pytest.raises(ValueError, match="w has 130 rows"):
        ops.fp8_block_train_cast_weight(_bf(130, 128))
    with pytest.raises(ValueError, match="w has 200 columns"):
        ops.fp8_block_train_cast_weight(_bf(128, 200), transposed=True)
    q = lambda *s: torch.zeros(*s, dtype=torch.uint8).view(torch.float8_e4m3fn)  # noqa: E731
    f = lambda *s: torch.ones(*s, dtype=torch.float32)  # noqa: E731
    with pytest.raises(ValueError, match="g_t must hold float8_e4m3fn codes"):
        ops.fp8_block_mm_wgrad(_bf(128, 128), f(1, 128), q(128, 128), f(1, 128))
    with pytest.raises(ValueError, match="x_t must be 2-D"):
        ops.fp8_block_mm_wgrad(q(128, 128), f(1, 128), q(128), f(1, 128))
    with pytest.raises(ValueError, match=r"x_t must be \[K, M=128\]"):
        ops.fp8_block_mm_wgrad(q(128, 128), f(1, 128), q(128, 256), f(1, 128))
    with pytest.raises(ValueError, match="M .*= 130 must be a multiple of 128"):
        ops.fp8_block_mm_wgrad(q(128, 130), f(1, 128), q(128, 130), f(1, 128))
    with pytest.raises(ValueError, match="N .*= 64 must be a multiple of 128"):
        ops.fp8_block_mm_wgrad(q(64, 128), f(1, 64), q(128, 128), f(1, 128))
    with pytest.raises(ValueError, match="K .*= 64 must be a multiple of 128"):
        ops.fp8_block_mm_wgrad(q(128, 128), f(1, 128), q(64, 128), f(1, 64))
    with pytest.raises(ValueError, match=r"g_inv must be float32 \[M/128, 128\]"):
        ops.fp8_block_mm_wgrad(q(128, 256), f(1, 128), q(128, 256), f(2, 128))
    with pytest.raises(ValueError, match="x_inv must be float32"):
        ops.fp8_block_mm_wgrad(q(128, 128), f(1, 128), q(128, 128), f(1, 128).double())
    # what passes the checks fails only at the GPU requirement
    for call in (lambda: ops.fp8_block_train_cast(_bf(5, 128)), lambda: ops.fp8_block_train_cast_weight(_bf(128, 256)),
                 lambda: ops.fp8_block_mm_wgrad(q(128, 128), f(1, 128), q(256, 128), f(1, 256))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_function_refuses_what_it_does_not_take_on_the_cpu():
    w = _bf(128, 256)
    with pytest.raises(AssertionError, match="Only support block_size=128, got 64"):
        fp8_blockwise_mm.apply(_bf(128, 256), w, 64)
    with pytest.raises(AssertionError, match="x and weight must be bfloat16.*float32"):
        fp8_blockwise_mm.apply(torch.zeros(128, 256), w, 128)
    with pytest.raises(AssertionError, match="x and weight must be bfloat16.*float16"):
        fp8_blockwise_mm.apply(_bf(128, 256), w.to(torch.float16), 128)
    with pytest.raises(AssertionError, match="out_dtype must be bfloat16"):
        fp8_blockwise_mm.apply(_bf(128, 256), w, 128, torch.float32)
    with pytest.raises(AssertionError, match="K and N must be positive multiples of 128.*K=192"):
        fp8_blockwise_mm.apply(_bf(128, 192), _bf(128, 192), 128)
    with pytest.raises(AssertionError, match="K and N must be positive multiples of 128.*N=64"):
        fp8_blockwise_mm.apply(_bf(128, 256), _bf(64, 256), 128)
    with pytest.raises(AssertionError, match="not compatible"):
        fp8_blockwise_mm.apply(_bf(128, 128), w, 128)
    with pytest.raises(AssertionError, match="M=130 tokens must be a multiple of 128 while the weight needs a gradient.*freeze the weight"):
        fp8_blockwise_mm.apply(_bf(2, 65, 256), _bf(128, 256, requires_grad=True), 128)
    # M = 130 passes the checks where no weight gradient is asked for, and fails only at the GPU requirement
    for weight, ctx in ((w, torch.enable_grad()), (_bf(128, 256, requires_grad=True), torch.no_grad())):
        with ctx, pytest.raises(RuntimeError, match="no CPU fallback"):
            fp8_blockwise_mm.apply(_bf(2, 65, 256, requires_grad=True), weight, 128, torch.bfloat16, True)  # (use_triton is accepted)


def test_the_module_refuses_a_bias_and_features_that_are_no_multiples_of_128():
    with pytest.raises(ValueError, match="takes no bias"):
        Float8BlockwiseLinear(256, 128, bias=True)
    with pytest.raises(ValueError, match="takes no bias"):
        Float8BlockwiseLinear(256, 128)  # nn.Linear's default
    with pytest.raises(AssertionError, match="Unsupported dtype"):
        Float8BlockwiseLinear(256, 128, bias=False, dtype=torch.float32)
    with pytest.raises(AssertionError, match="block_size=128"):
        Float8BlockwiseLinear(256, 128, bias=False, block_size=64)
    with pytest.raises(AssertionError, match="has a bias"):
        Float8BlockwiseLinear.from_float(nn.Linear(256, 128, bias=True))
    with pytest.raises(AssertionError, match="in_features=192"):
        Float8BlockwiseLinear.from_float(nn.Linear(192, 128, bias=False))
    with pytest.raises(AssertionError, match="out_features=64"):
        Float8BlockwiseLinear.from_float(nn.Linear(256, 64, bias=False))
    m = Float8BlockwiseLinear(256, 128, bias=False, use_triton=True)
    assert m.block_size == 128 and m.dtype == torch.bfloat16 and m.use_triton and m.bias is None and tuple(m.weight.shape) == (128, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.to(torch.bfloat16)(_bf(128, 256))


def test_quantize_swaps_a_bias_free_linear_and_shares_its_parameter():
    model = nn.Sequential(nn.Linear(256, 128, bias=False), nn.ReLU(), nn.Linear(128, 64, bias=True)).to(torch.bfloat16)
    weight, other = model[0].weight, model[2]
    quantize_(model, Float8BlockwiseLinearConfig(), filter_fn=lambda m, fqn: isinstance(m, nn.Linear) and fqn == "0")
    assert type(model[0]) is Float8BlockwiseLinear and model[0].weight is weight and model[0].bias is None
    assert (model[0].in_features, model[0].out_features) == (256, 128) and weight.device.type == "cpu" and weight.requires_grad
    assert model[2] is other and type(other) is nn.Linear
    with pytest.raises(AssertionError, match="has a bias"):
        quantize_(model, Float8BlockwiseLinearConfig(), filter_fn=lambda m, fqn: fqn == "2")
