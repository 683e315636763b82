"""FP8 attention without a GPU: the ABI, the named refusals, the wrapper's restore, and the kernel test's bound checked against a CPU
emulation of the kernel's arithmetic (if the emulation left the bound, the derivation would be wrong, not the kernel)."""
import pytest
import torch
import torch.nn.functional as F

import fp8_attention_ref as R
from ao_amd import _lib, ops
from ao_amd.prototype import attention as A


def test_abi_declared_and_exported():
    lib, declared = _lib.lib(), _lib.declared_symbols()
    for name, nargs in (("ao_fp8_attn_fits", 6), ("ao_fp8_attn_quantize", 19), ("ao_fp8_attn_fwd", 17)):
        assert hasattr(lib, name) and name in declared and len(_lib._SIGNATURES[name]) == nargs
    for name in ("fp8_attn_quantize", "fp8_attn_fwd", "fp8_attn_fits"):
        assert name in ops.__all__
    assert hasattr(torch.ops.ao_mi355, "fp8_sdpa")


@pytest.mark.parametrize("q,k,v,word", [
    ((2, 8, 16, 96), (2, 8, 16, 96), (2, 8, 16, 96), "D=96"),
    ((2, 6, 16, 64), (2, 4, 16, 64), (2, 4, 16, 64), "multiple of Hkv"),
    ((2, 8, 16, 64), (2, 8, 16, 64), (2, 8, 17, 64), "K and V must have the same shape"),
    ((2, 8, 16), (2, 8, 16, 64), (2, 8, 16, 64), "4-D"),
])
def test_fits_names_each_refusal(q, k, v, word):
    assert ops.fp8_attn_fits((2, 8, 200, 128), (2, 2, 77, 128), (2, 2, 77, 128)) is None
    assert word in ops.fp8_attn_fits(q, k, v)


def test_fp8_sdpa_refusals():
    q = torch.zeros(1, 2, 4, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="attn_mask not supported for FP8"):
        A.fp8_sdpa(q, q, q, attn_mask=torch.ones(4, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="dropout_p must be 0.0 for FP8"):
        A.fp8_sdpa(q, q, q, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="RoPE-fused"):
        A._fp8_rope_sdpa(q, q, q, None, None)


def test_apply_refusals():
    with pytest.raises(RuntimeError, match="FP8_FA3 requires Hopper"):
        A.apply_low_precision_attention(torch.nn.Linear(4, 4), backend=A.AttentionBackend.FP8_FA3)
    with pytest.raises(NotImplementedError, match="HadamardMode.QKV"):
        A.apply_low_precision_attention(torch.nn.Linear(4, 4), hadamard=A.HadamardMode.QKV)
    wrapped = A.apply_low_precision_attention(torch.nn.Linear(4, 4))
    assert wrapped.in_features == 4  # attribute access reaches the wrapped module
    with pytest.raises(RuntimeError, match="already been applied"):
        A.apply_low_precision_attention(wrapped)


def test_wrapper_restores_sdpa_after_a_raising_forward():
    seen = []

    class Raises(torch.nn.Module):
        def forward(self, x):
            seen.append(F.scaled_dot_product_attention)
            raise KeyError("inside forward")

    original = F.scaled_dot_product_attention
    with pytest.raises(KeyError):
        A.apply_low_precision_attention(Raises())(torch.zeros(1))
    assert seen == [A.fp8_sdpa] and F.scaled_dot_product_attention is original


@pytest.mark.parametrize("D,Sq,Skv,causal", R.KERNEL_SHAPES)
@pytest.mark.parametrize("groups,spread,scale", [(1, 1.0, None), (4, 1.0, None), (1, 8.0, None), (4, 1.0, 0.21)])
def test_emulated_kernel_chain_sits_inside_the_bound(D, Sq, Skv, causal, groups, spread, scale):
    q8, k8, v8, dq, dk, dv = R.kernel_case(D, Sq, Skv, groups, spread)
    v_deq = R.dequant(v8, dv).repeat_interleave(groups, 1)
    ref, p, l, _ = R.sdpa_f64(R.dequant(q8, dq, groups), R.dequant(k8, dk), R.dequant(v8, dv), causal, scale)
    got = R.emulate_kernel(q8, k8, v8, dq, dk, dv, causal, scale, torch.bfloat16).double()
    assert bool(((got - ref).abs() <= R.kernel_bound(ref, p, l, v_deq, causal)).all())
