"""CPU: blockwise float8 training of the MoE grouped GEMM -- the fixture recorded from the reference's torch functions
(tests/golden/fp8_block_grouped_training.npz) against the numpy restatement; the new symbols, ops and prototype names; every refusal
with its reason and no GPU; the C entry points' argument checks (no kernel is launched in this file)."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import blockwise_fp8_training_ref as R
import fp8_block_grouped_training_ref as G
from ao_amd import _lib, ops, prototype
from ao_amd.prototype.blockwise_fp8_grouped_training import (
    _Float8BlockwiseGroupedMM,
    _to_fp8_blockwise_then_emulated_scaled_grouped_mm,
    _to_fp8_blockwise_then_scaled_grouped_mm,
)
from ao_amd.quantization.config import KernelPreference

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ("ao_fp8_block_train_cast_weight_3d", "ao_fp8_block_grouped_mm_wgrad")
OPS = ("fp8_block_train_cast_weight_3d", "fp8_block_grouped_mm_wgrad")
NAMES = ("_to_fp8_blockwise_then_scaled_grouped_mm", "_to_fp8_blockwise_then_emulated_scaled_grouped_mm", "_Float8BlockwiseGroupedMM")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _load("make_golden_fp8_block_grouped_training")


@functools.lru_cache(maxsize=None)
def fixture():
    return MAKER.load()


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_the_restatement_reproduces_the_recorded_operands_casts_and_products(case):
    F, spec = fixture(), G.CASES[case]
    ab, wb, gob = G.operands(case)
    M, E = spec["offs"][-1], len(spec["offs"])
    assert ab.shape == (M, 256) and wb.shape == (E, 256, 256) and gob.shape == (M, 256)
    np.testing.assert_array_equal(F[case + "_offs"], np.array(spec["offs"], dtype=np.int32))
    for t, b in (("a", ab), ("w", wb), ("go", gob)):
        np.testing.assert_array_equal(G.sha(b), F["%s_%s_sha" % (case, t)], err_msg="the generated operand %s is not the recorded one" % t)
    casts, starts, ends = G.function_casts(ab, wb, gob, spec["offs"], spec["pad"])
    rows = casts["a_row"][0].shape[0]
    assert rows % 128 == 0 and rows == (896 if spec["pad"] else 512)
    for name in MAKER.CASTS:
        q, inv = casts[name]
        np.testing.assert_array_equal(G.sha(q), F["%s_%s_q_sha" % (case, name)], err_msg=name)
        np.testing.assert_array_equal(_u32(inv), _u32(F["%s_%s_inv" % (case, name)]), err_msg=name)
    ref64 = G.function_f64(casts, spec["offs"], starts, ends, M)
    for name, r in zip(MAKER.RESULTS, ref64):
        np.testing.assert_allclose(np.sum(r ** 2), float(F["%s_%s_energy" % (case, name)]), rtol=1e-12)
        s = F["%s_%s_sample" % (case, name)]
        assert s.shape == G.sample(r).shape and s.dtype == np.uint16
        # the recorded rows of the reference's result are results of THIS product: they sit where the whole tensor's SQNR sits
        got, whole = G.sqnr(R.bf16.from_bits(s).astype(np.float64), G.sample(r)), float(F["%s_%s_ref_sqnr" % (case, name)])
        assert 45.0 < whole < 52.0 and abs(got - whole) < 1.0, (name, got, whole)


def test_the_padding_of_the_restatement_puts_every_group_on_whole_blocks():
    xb = np.arange(500 * 2, dtype=np.uint16).reshape(500, 2) + 1
    padded, starts, ends = G.pad_groups(xb, (129, 384, 500))
    np.testing.assert_array_equal(starts, [0, 256, 512])
    np.testing.assert_array_equal(ends, [256, 512, 640])
    assert padded.shape == (896, 2) and not padded[129:256].any() and not padded[640:].any()
    np.testing.assert_array_equal(padded[256:256 + 255], xb[129:384])
    np.testing.assert_array_equal(G.unpad_groups(padded, (129, 384, 500), starts, 500), xb)
    assert G.bounds((0, 600, 300), 512) == [(0, 0), (0, 512), (512, 512)]
    assert G.bounds((128, 128, 384, 512), 512) == [(0, 128), (128, 128), (128, 384), (384, 512)]


def test_the_grouped_chain_equals_the_float64_sum_on_exact_operands():
    case = G.exact_operands(256, 128, 128, 7)
    offs = (129, 200, 256)
    bits = G.grouped_wgrad_chain_bits(*case, offs)
    assert bits.shape == (3, 128, 128)
    for e, (y, _) in enumerate(G.grouped_wgrad_f64(*case, offs)):
        np.testing.assert_array_equal(bits[e], R.bf16.to_bits(R.bf16.bf16_round(y.astype(np.float32))))
    # the groups partition the tokens: their float64 sums add up to the dense one
    total = sum(y for y, _ in G.grouped_wgrad_f64(*case, offs))
    np.testing.assert_allclose(total, R.wgrad_f64(*case)[0], rtol=0, atol=1e-9)


# ---- names ----------------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_ops_and_prototype_names_are_there():
    from ao_amd import torch_ops  # noqa: F401  (registers the ao_mi355 ops)

    names = _lib.declared_symbols()
    for n in SYMBOLS:
        assert n in names and n in _lib._SIGNATURES and hasattr(_lib.lib(), n), n
    for n in OPS:
        assert n in ops.__all__ and callable(getattr(ops, n)), n
        assert hasattr(torch.ops.ao_mi355, n), n
    for n in NAMES:
        assert n in prototype.__all__ and hasattr(prototype, n), n
    text = open(_lib.HEADER_PATH).read()
    for cite in ("grouped_mm.py:98-265", "grouped_mm_backend.py:158-194"):
        assert cite in text, cite


def test_the_fakes_give_the_shapes_of_the_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from ao_amd import torch_ops  # noqa: F401

    with FakeTensorMode():
        w = torch.empty(3, 256, 384, dtype=torch.bfloat16, device="cuda")
        q, inv = torch.ops.ao_mi355.fp8_block_train_cast_weight_3d(w, False)
        assert (q.shape, inv.shape) == ((3, 256, 384), (3, 2, 3)) and q.dtype == torch.float8_e4m3fn and inv.dtype == torch.float32
        q, inv = torch.ops.ao_mi355.fp8_block_train_cast_weight_3d(w, True)
        assert (q.shape, inv.shape) == ((3, 384, 256), (3, 3, 2))
        g_t = torch.empty(256, 512, dtype=torch.float8_e4m3fn, device="cuda")
        x_t = torch.empty(128, 512, dtype=torch.float8_e4m3fn, device="cuda")
        gi, xi = torch.empty(4, 256, device="cuda"), torch.empty(4, 128, device="cuda")
        offs = torch.empty(5, dtype=torch.int32, device="cuda")
        out = torch.ops.ao_mi355.fp8_block_grouped_mm_wgrad(g_t, gi, x_t, xi, offs)
        assert out.shape == (5, 256, 128) and out.dtype == torch.bfloat16
        assert torch.ops.ao_mi355.fp8_block_grouped_mm_wgrad(g_t, gi, x_t, xi, None).shape == (1, 256, 128)


# ---- the C entry points -----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_check_their_arguments_on_the_host():
    lib = _lib.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first, and an empty tensor launches nothing
    inv, ok, null = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_OK, _lib.AO_ERR_NULL_POINTER
    cast = lambda e, n, k: lib.ao_fp8_block_train_cast_weight_3d(one, one, one, one, one, e, n, k, None)  # noqa: E731
    wgrad = lambda m, n, k, e, offs=one: lib.ao_fp8_block_grouped_mm_wgrad(one, one, one, one, offs, one, m, n, k, e, None)  # noqa: E731
    assert cast(2, 100, 128) == inv and "N=100" in _lib.last_error() and "multiples of 128" in _lib.last_error()
    assert cast(2, 128, 200) == inv and "K=200" in _lib.last_error()
    assert cast(-1, 128, 128) == inv
    assert cast(65536, 128, 128) == inv and "E=65536" in _lib.last_error()
    assert cast(40000, 256, 128) == inv and "too large" in _lib.last_error()  # 80000 row tiles
    assert lib.ao_fp8_block_train_cast_weight_3d(one, None, None, None, None, 2, 128, 128, None) == inv and "neither" in _lib.last_error()
    assert lib.ao_fp8_block_train_cast_weight_3d(None, one, one, None, None, 2, 128, 128, None) == null
    assert lib.ao_fp8_block_train_cast_weight_3d(one, one, None, None, None, 2, 128, 128, None) == null  # half a pair
    assert lib.ao_fp8_block_train_cast_weight_3d(ctypes.c_void_p(8), one, one, None, None, 2, 128, 128, None) == inv
    assert "aligned" in _lib.last_error()
    for e, n, k in ((0, 128, 128), (2, 0, 128), (2, 128, 0), (0, 0, 0)):
        assert cast(e, n, k) == ok
    assert cast(0, 100, 128) == inv  # the shape is checked before the tensor is found empty
    for m, n, k, bad in ((100, 128, 128, "M=100"), (128, 100, 128, "N=100"), (128, 128, 100, "K=100")):
        assert wgrad(m, n, k, 2) == inv and bad in _lib.last_error() and "multiples of 128" in _lib.last_error()
    assert wgrad(128, 0, 128, 2) == inv and wgrad(128, 128, 0, 2) == inv and wgrad(-128, 128, 128, 2) == inv
    assert wgrad(128, 128, 128, 0) == inv and "E=0" in _lib.last_error()
    assert wgrad(128, 128, 128, 65536) == inv and "E=65536" in _lib.last_error()
    assert wgrad(128, 128, 128, 2, None) == inv and "without offs" in _lib.last_error()
    assert wgrad(1 << 24, 128, 128, 2) == inv and "below 2^31" in _lib.last_error()  # an operand of 2 GiB
    assert lib.ao_fp8_block_grouped_mm_wgrad(one, one, one, one, one, None, 128, 128, 128, 2, None) == null
    assert lib.ao_fp8_block_grouped_mm_wgrad(None, one, one, one, one, one, 128, 128, 128, 2, None) == null
    assert lib.ao_fp8_block_grouped_mm_wgrad(one, one, one, None, one, one, 128, 128, 128, 2, None) == null
    with pytest.raises(ValueError, match="N=100"):
        _lib.check(cast(2, 100, 128))


# ---- the Python refusals, each before any GPU requirement ---------------------------------------------------------------------------------
def _bf(*shape, **kw):
    return torch.zeros(*shape, dtype=torch.bfloat16, **kw)


def test_the_ops_refuse_dtypes_ranks_and_shapes_before_the_library_is_touched():
    with pytest.raises(ValueError, match="fp8_block_train_cast_weight_3d: w must be a bfloat16 tensor"):
        ops.fp8_block_train_cast_weight_3d(torch.zeros(2, 128, 128))
    with pytest.raises(ValueError, match=r"w must be 3-D \[E, N, K\]"):
        ops.fp8_block_train_cast_weight_3d(_bf(128, 128))
    with pytest.raises(ValueError, match="w has 130 rows an expert"):
        ops.fp8_block_train_cast_weight_3d(_bf(2, 130, 128))
    with pytest.raises(ValueError, match="w has 200 columns"):
        ops.fp8_block_train_cast_weight_3d(_bf(2, 128, 200), transposed=None)
    with pytest.raises(ValueError, match="at most 65535"):
        ops.fp8_block_train_cast_weight_3d(torch.empty(65536, 128, 0, dtype=torch.bfloat16), transposed=True)
    q = lambda *s: torch.zeros(*s, dtype=torch.uint8).view(torch.float8_e4m3fn)  # noqa: E731
    f = lambda *s: torch.ones(*s, dtype=torch.float32)  # noqa: E731
    offs = torch.tensor([64, 128], dtype=torch.int32)
    with pytest.raises(ValueError, match="fp8_block_grouped_mm_wgrad: g_t must hold float8_e4m3fn codes"):
        ops.fp8_block_grouped_mm_wgrad(_bf(128, 128), f(1, 128), q(128, 128), f(1, 128), offs)
    with pytest.raises(ValueError, match="x_t must be 2-D"):
        ops.fp8_block_grouped_mm_wgrad(q(128, 128), f(1, 128), q(128), f(1, 128), offs)
    with pytest.raises(ValueError, match=r"x_t must be \[K, M=128\]"):
        ops.fp8_block_grouped_mm_wgrad(q(128, 128), f(1, 128), q(128, 256), f(1, 128), offs)
    with pytest.raises(ValueError, match="M .*= 130 must be a multiple of 128"):
        ops.fp8_block_grouped_mm_wgrad(q(128, 130), f(1, 128), q(128, 130), f(1, 128), offs)
    with pytest.raises(ValueError, match="N .*= 64 must be a multiple of 128"):
        ops.fp8_block_grouped_mm_wgrad(q(64, 128), f(1, 64), q(128, 128), f(1, 128), offs)
    with pytest.raises(ValueError, match="K .*= 64 must be a multiple of 128"):
        ops.fp8_block_grouped_mm_wgrad(q(128, 128), f(1, 128), q(64, 128), f(1, 64), offs)
    with pytest.raises(ValueError, match=r"g_inv must be float32 \[M/128, 128\]"):
        ops.fp8_block_grouped_mm_wgrad(q(128, 256), f(1, 128), q(128, 256), f(2, 128), offs)
    with pytest.raises(ValueError, match="x_inv must be float32"):
        ops.fp8_block_grouped_mm_wgrad(q(128, 128), f(1, 128), q(128, 128), f(1, 128).double(), offs)
    for bad in (offs.long(), offs.reshape(1, 2), offs[:0], [64, 128]):
        with pytest.raises(ValueError, match="offs must be a non-empty int32"):
            ops.fp8_block_grouped_mm_wgrad(q(128, 128), f(1, 128), q(128, 128), f(1, 128), bad)
    # what passes the checks fails only at the GPU requirement
    for call in (lambda: ops.fp8_block_train_cast_weight_3d(_bf(2, 128, 256)),
                 lambda: ops.fp8_block_grouped_mm_wgrad(q(128, 128), f(1, 128), q(256, 128), f(1, 256), offs),
                 lambda: ops.fp8_block_grouped_mm_wgrad(q(128, 128), f(1, 128), q(256, 128), f(1, 256), None)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def _good():
    return _bf(256, 256), _bf(2, 128, 256).transpose(-2, -1), torch.tensor([128, 256], dtype=torch.int32)


def test_the_function_refuses_what_it_does_not_take_on_the_cpu():
    f = _to_fp8_blockwise_then_scaled_grouped_mm
    A, B_t, offs = _good()
    bad = [
        (dict(A=_bf(2, 128, 256)), "A must be 2D"),
        (dict(B_t=_bf(256, 128)), "B_t must be 3D"),
        (dict(A=A.float()), "A must be bfloat16"),
        (dict(B_t=B_t.float()), "B_t must be bfloat16"),
        (dict(out_dtype=torch.float32), "out_dtype must be bfloat16"),
        (dict(float8_dtype=torch.float8_e5m2), "float8_dtype must be torch.float8_e4m3fn"),
        (dict(block_size=64), "Only block_size=128 is supported"),
        (dict(offs=None), "offs must be an int32 tensor"),
        (dict(offs=offs.long()), "offs must be an int32 tensor"),
        (dict(offs=torch.tensor([256], dtype=torch.int32)), "offs must have one end per expert"),
        (dict(offs=offs.reshape(2, 1)), "offs must have one end per expert"),
        (dict(A=_bf(256, 128)), "are not compatible"),
        (dict(A=_bf(256, 256).t()), "A must be row-major"),
        (dict(B_t=_bf(2, 256, 128)), "B_t must be per-expert column-major"),
        (dict(A=_bf(256, 192), B_t=_bf(2, 128, 192).transpose(-2, -1)), "K and N must be positive multiples"),
        (dict(B_t=_bf(2, 192, 256).transpose(-2, -1)), "K and N must be positive multiples"),
        (dict(kernel_preference=KernelPreference.TORCH), "kernel_preference must be AUTO, DEEPGEMM, or EMULATED"),
        (dict(kernel_preference="auto_"), "kernel_preference must be"),
    ]
    for change, reason in bad:
        kw = dict(A=A, B_t=B_t, offs=offs)
        kw.update(change)
        with pytest.raises(AssertionError, match=reason):
            f(**kw)
    # M no multiple of 128 without padding: refused only while B_t needs a gradient
    A130, offs130 = _bf(130, 256), torch.tensor([60, 130], dtype=torch.int32)
    with pytest.raises(AssertionError, match="M=130 tokens must be a multiple of 128 while B_t needs a gradient"):
        f(A130, B_t.detach().requires_grad_(True), offs130, pad_token_groups_for_grouped_mm=False)
    for call in (lambda: f(A130, B_t, offs130, pad_token_groups_for_grouped_mm=False),
                 lambda: f(A130, B_t.detach().requires_grad_(True), offs130),
                 lambda: _Float8BlockwiseGroupedMM.apply(A, B_t, offs),
                 lambda: _to_fp8_blockwise_then_emulated_scaled_grouped_mm(A, B_t, offs)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # past every refusal: only the GPU is missing
            call()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        f(A130, B_t.detach().requires_grad_(True), offs130, pad_token_groups_for_grouped_mm=False)
    # the Function's own apply refuses too
    with pytest.raises(AssertionError, match="B_t must be per-expert column-major"):
        _Float8BlockwiseGroupedMM.apply(A, _bf(2, 256, 128), offs)


@pytest.mark.parametrize("pref", [KernelPreference.AUTO, KernelPreference.DEEPGEMM, KernelPreference.EMULATED])
def test_the_three_kernel_preferences_are_accepted(pref):
    A, B_t, offs = _good()
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # accepted: the call goes on to the kernels
        _to_fp8_blockwise_then_scaled_grouped_mm(A, B_t, offs, kernel_preference=pref)


def test_the_left_out_sentences_are_gone():
    from ao_amd.prototype import blockwise_fp8_training

    assert "Left out: the grouped blockwise training op" not in blockwise_fp8_training.__doc__
    assert "blockwise_fp8_grouped_training" in blockwise_fp8_training.__doc__
