"""CPU: the MXFP8 grouped GEMM's backward at the host -- the wgrad entry's declaration, export and signature, the argument checks of the
C ABI, the two new keywords of _to_mxfp8_then_scaled_grouped_mm and its refusals when a tensor requires grad, the fake kernel, and the
fixture written from the reference (tests/golden/mxfp8_grouped_bwd.npz) against the oracle's cast.  No kernel is launched in this file."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from ao_amd import _lib, ops
from ao_amd.prototype import mx
from oracle import mx_ref

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "ao_mxfp8_grouped_mm_wgrad"


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_mxfp8_bwd", os.path.join(HERE, "golden", "make_golden_mxfp8_bwd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_signed():
    lib = _lib.lib()
    assert hasattr(lib, NAME) and NAME in _lib.declared_symbols() and NAME in _lib._SIGNATURES
    assert len(_lib._SIGNATURES[NAME]) == 11
    assert "mxfp8_grouped_mm_wgrad" in ops.__all__ and callable(ops.mxfp8_grouped_mm_wgrad)
    assert list(inspect.signature(ops.mxfp8_grouped_mm_wgrad).parameters) == ["g_t", "g_scale", "x_t", "x_scale", "offs", "N", "K"]


def _scratch():
    buf = ctypes.create_string_buffer(4096)
    return buf, (ctypes.addressof(buf) + 15) & ~15


@pytest.mark.parametrize("shape,reason", [
    ((48, 128, 128, 2), "M_total=48 must be a multiple of 32"),
    ((64, 24, 128, 2), "N=24 must be a multiple of 16"),
    ((64, 128, 40, 2), "K=40 must be a multiple of 16"),
    ((64, 128, 128, 65536), "E=65536 must be below 65536"),
    ((64, 128, 128, 0), "bad shape"),
    ((1 << 20, 1 << 11, 128, 2), "below 2^31"),
    ((1 << 20, 128, 1 << 11, 2), "below 2^31"),
    ((1 << 31, 16, 16, 2), "below 2^31"),
])
def test_host_checks_reject_the_shape_with_a_reason(shape, reason):
    lib = _lib.lib()
    _buf, p = _scratch()
    assert getattr(lib, NAME)(p, p, p, p, p, p, *shape, None) == _lib.AO_ERR_INVALID_ARGUMENT
    msg = lib.ao_last_error().decode()
    assert NAME in msg and reason in msg, msg


def test_host_checks_reject_null_and_misaligned_pointers():
    lib = _lib.lib()
    _buf, p = _scratch()
    fn = getattr(lib, NAME)
    for i in range(6):  # g_t, g_scale, x_t, x_scale, offs, out
        args = [p] * 6
        args[i] = None
        assert fn(*args, 64, 128, 128, 2, None) == _lib.AO_ERR_NULL_POINTER, i
        assert NAME + ": null pointer" in lib.ao_last_error().decode()
    assert fn(p + 8, p, p, p, p, p, 64, 128, 128, 2, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert fn(p, p, p + 8, p, p, p, 64, 128, 128, 2, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "16-byte aligned" in lib.ao_last_error().decode()
    assert fn(None, None, None, None, None, None, 0, 128, 128, 2, None) == _lib.AO_ERR_NULL_POINTER  # M_total = 0 still writes out


def test_ops_check_before_any_launch():
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    offs = torch.tensor([64], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="mxfp8_grouped_mm_wgrad: .*no CPU fallback"):
        ops.mxfp8_grouped_mm_wgrad(z(128, 64), z(2, 128), z(128, 64), z(2, 128), offs, 128, 128)


def test_fake_kernel_gives_the_shape():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ao_amd.torch_ops  # noqa: F401

    with FakeTensorMode():
        g_t, x_t = torch.empty(64, 128, dtype=torch.float8_e4m3fn).t(), torch.empty(256, 128, dtype=torch.float8_e4m3fn).t()
        gs, xs = torch.empty(4, 64, dtype=torch.float8_e8m0fnu).t(), torch.empty(4, 256, dtype=torch.float8_e8m0fnu).t()
        y = torch.ops.ao_mi355.mxfp8_grouped_mm_wgrad(g_t, gs, x_t, xs, torch.empty(3, dtype=torch.int32), 64, 256)
    assert tuple(y.shape) == (3, 64, 256) and y.dtype == torch.bfloat16


# ---- the Python entry --------------------------------------------------------------------------------------------------------------------
def test_the_entry_takes_the_references_keywords():
    p = inspect.signature(mx._to_mxfp8_then_scaled_grouped_mm).parameters
    assert p["wgrad_with_hp"].default is False and p["pad_token_groups_for_grouped_mm"].default is False
    assert issubclass(mx._MXFP8GroupedMM, torch.autograd.Function)


def _operands(m=64, k=128, n=128, e=2):
    a = torch.zeros(m, k, dtype=torch.bfloat16, requires_grad=True)
    w = torch.zeros(e, n, k, dtype=torch.bfloat16, requires_grad=True)
    return a, w, torch.tensor([m // 2, m], dtype=torch.int32)


def test_training_refuses_a_frozen_cast():
    a, w, offs = _operands()
    frozen = mx.MXFP8ExpertWeights(torch.zeros(2, 128, 128, dtype=torch.uint8), torch.zeros(2, 128, 4, dtype=torch.uint8))
    with pytest.raises(AssertionError, match="MXFP8ExpertWeights is a frozen cast"):
        mx._to_mxfp8_then_scaled_grouped_mm(a, frozen, offs)
    with pytest.raises(AssertionError, match="cache_weights=True memoises a frozen cast"):
        mx._to_mxfp8_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs, cache_weights=True)
    with pytest.raises(AssertionError, match="cache_weights=True memoises a frozen cast"):
        mx._to_mxfp8_then_scaled_grouped_mm(a.detach(), w.transpose(-2, -1), offs, cache_weights=True)


def test_training_refuses_other_out_dtypes_and_shapes():
    a, w, offs = _operands()
    with pytest.raises(AssertionError, match="Only bfloat16 out_dtype is supported"):
        mx._to_mxfp8_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs, out_dtype=torch.float32)
    a, w, offs = _operands(n=64)
    with pytest.raises(AssertionError, match="N and K to be multiples of 128.*N=64 K=128"):
        mx._to_mxfp8_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs)
    a, w, offs = _operands(k=192)
    with pytest.raises(AssertionError, match="N and K to be multiples of 128.*N=128 K=192"):
        mx._to_mxfp8_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs)
    a, w, offs = _operands(m=48)
    with pytest.raises(AssertionError, match="M_total=48 must be a multiple of 32.*pad_token_groups_for_grouped_mm=True"):
        mx._to_mxfp8_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs)


def test_without_grad_the_refusals_do_not_apply():
    """Under no_grad a tensor that requires grad is an inference input: the call reaches the kernels' own device check, as it always did."""
    a, w, offs = _operands(m=48, n=64)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        mx._to_mxfp8_then_scaled_grouped_mm(a, w.transpose(-2, -1), offs)


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_references_casts_and_gradients():
    gen = _generator()
    G = gen.load()
    E, N, K, M = gen.E, gen.N, gen.K, sum(gen.SIZES)
    np.testing.assert_array_equal(G["offs"], np.cumsum(gen.SIZES))
    assert G["a"].shape == (M, K) and G["w"].shape == (E, N, K) and G["go"].shape == (M, N)
    for pad in ("nopad", "pad"):
        for hp in ("mx", "hp"):
            assert G[f"gi_{pad}_{hp}"].shape == (M, K) and G[f"gi_{pad}_{hp}"].dtype == np.uint16
            assert G[f"gw_{pad}_{hp}"].shape == (E, N, K) and not G[f"gw_{pad}_{hp}"][1].any()  # the empty expert
    # the oracle's cast gives the reference's bytes for the three 32 x 1 casts of the backward
    for name, src in (("go_t", "go"), ("a_t", "a")):
        q, s = mx_ref.to_mx(np.ascontiguousarray(_bf16(G[src]).float().numpy().T), mx_ref.RCEIL)
        np.testing.assert_array_equal(q, G[name + "_q"])
        np.testing.assert_array_equal(s, G[name + "_s"])
    q, s = mx_ref.to_mx(np.ascontiguousarray(_bf16(G["w"]).float().numpy().transpose(0, 2, 1)), mx_ref.RCEIL)  # [E, K, N], blocks along N
    np.testing.assert_array_equal(q.transpose(0, 2, 1), G["w_n_q"])
    np.testing.assert_array_equal(s.transpose(0, 2, 1), G["w_n_s"])
