"""Int8 mixed-precision training without a GPU: the config, every named refusal, the exports."""
import pytest
import torch
import torch.nn.functional as F

from ao_amd import _lib, ops
from ao_amd.prototype import quantized_training as Q
from ao_amd.quantization import config_from_dict, config_to_dict, quantize_

BF16 = torch.bfloat16


def test_config_fields_alias_and_round_trip():
    c = Q.Int8MixedPrecisionTrainingConfig()
    assert (c.output, c.grad_input, c.grad_weight, c.module_swap) == (True, True, True, False)
    assert Q.int8_mixed_precision_training is Q.Int8MixedPrecisionTrainingConfig
    c = Q.Int8MixedPrecisionTrainingConfig(True, False, True, True)  # the reference's argument order
    assert (c.grad_input, c.module_swap) == (False, True)
    d = config_to_dict(c)
    assert d["_type"] == "Int8MixedPrecisionTrainingConfig" and d["_data"] == {"output": True, "grad_input": False, "grad_weight": True, "module_swap": True}
    assert config_from_dict(d) == c


def test_exports():
    for name in ("int8_train_quantize", "int8_train_mm", "int8_train_mm_fits", "int8_train_mm_kernel_name"):
        assert name in ops.__all__
    for name in ("quantize_int8_rowwise", "Int8MixedPrecisionTrainingConfig", "Int8MixedPrecisionTrainingLinear", "Int8MixedPrecisionTrainingLinearWeight",
                 "int8_mixed_precision_training", "_dynamic_int8_mm", "_Int8MixedPrecisionTrainingLinearFunction"):
        assert hasattr(Q, name)
    assert not hasattr(Q, "Int8QuantizedTrainingLinearWeight") and "Int8QuantizedTrainingLinearWeight" in Q.__doc__
    assert _lib.lib().ao_int8_train_quantize_workspace_bytes(130, 4112) == ((5 * 4112 + 130 * 2) * 2 + 15) // 16 * 16
    assert [ops.int8_train_mm_kernel_name(a, b) for a in (0, 1) for b in (0, 1)] == [f"int8_train_mm_kernel<{a},{b}>" for a in (0, 1) for b in (0, 1)]


@pytest.mark.parametrize("m,n,kc,a_t,b_t,word", [
    (4, 24, 64, 0, 0, "N=24 must be a multiple of 16"), (4, 16, 0, 1, 1, "bad shape"), (4, 16, 2 ** 17 + 16, 0, 0, "above 2^17"),
    (4, 16, 64, 1, 0, "M=4, its contiguous dimension"), (16, 16, 8, 0, 1, "Kc=8 a multiple of 16"), (2 ** 22 + 16, 16, 16, 0, 0, "too large")])
def test_mm_fits_names_each_refusal(m, n, kc, a_t, b_t, word):
    assert ops.int8_train_mm_fits(7, 144, 80) is None and ops.int8_train_mm_fits(16, 16, 1, True, True) is None
    assert word in ops.int8_train_mm_fits(m, n, kc, a_t, b_t)
    one = 16  # never dereferenced: the shape is refused first
    assert _lib.lib().ao_int8_train_mm(one, one, one, one, one, m, n, kc, a_t, b_t, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert _lib.lib().ao_int8_train_mm(None, None, None, None, None, 0, 16, 16, 0, 0, None) == _lib.AO_OK  # empty M: no launch


def test_ops_refuse_before_any_launch():
    x, q, s = torch.zeros(4, 32, dtype=BF16), torch.zeros(4, 32, dtype=torch.int8), torch.zeros(4, dtype=BF16)
    with pytest.raises(RuntimeError, match="int8_train_quantize: expected all tensors on the GPU.*no CPU fallback"):
        ops.int8_train_quantize(x)
    with pytest.raises(RuntimeError, match="int8_train_mm: expected all tensors on the GPU.*no CPU fallback"):
        ops.int8_train_mm(q, q, s, s)
    one = 16
    lib = _lib.lib()
    assert lib.ao_int8_train_quantize(one, one, one, None, None, None, 4, 24, 1e-12, 0, 0, 0, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "K=24 must be a multiple of 16" in _lib.last_error()
    assert lib.ao_int8_train_quantize(one, None, None, one, one, one, 4, 32, 1e-12, 1, 0, 0, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "stochastic rounding is the row cast's" in _lib.last_error()
    assert lib.ao_int8_train_quantize(one, one, None, None, None, None, 4, 32, 1e-12, 0, 0, 0, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_int8_train_quantize(None, None, None, None, None, None, 0, 32, 1e-12, 0, 0, 0, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_int8_train_quantize(None, one, one, None, None, None, 0, 32, 1e-12, 0, 0, 0, None) == _lib.AO_OK  # no rows: no launch


def test_module_refusals_name_the_argument():
    w = Q.Int8MixedPrecisionTrainingLinearWeight(torch.zeros(32, 64, dtype=BF16), Q.Int8MixedPrecisionTrainingConfig())
    for dtype in (torch.float16, torch.float32):
        with pytest.raises(NotImplementedError, match="the input must be bfloat16.*float16 and float32 are not built"):
            F.linear(torch.zeros(2, 64, dtype=dtype), w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.linear(torch.zeros(2, 64, dtype=BF16), w)
    for k, n in ((72, 32), (64, 40)):
        for swap in (False, True):
            with pytest.raises(ValueError, match=f"in_features={k} and out_features={n} must be multiples of 16"):
                quantize_(torch.nn.Linear(k, n, dtype=BF16), Q.Int8MixedPrecisionTrainingConfig(module_swap=swap))
        with pytest.raises(ValueError, match=f"in_features={k} and out_features={n} must be multiples of 16"):
            Q._Int8MixedPrecisionTrainingLinearFunction.apply(torch.zeros(2, k, dtype=BF16), torch.zeros(n, k, dtype=BF16), None)
    with pytest.raises(NotImplementedError, match="fsdp_pre_all_gather"):
        w.fsdp_pre_all_gather(None)
    with pytest.raises(NotImplementedError, match="fsdp_post_all_gather"):
        w.fsdp_post_all_gather((), None, BF16)
    assert isinstance(w.t(), Q.Int8MixedPrecisionTrainingLinearWeight) and type(w + 1) is torch.Tensor and torch.equal(w.to_original(), w._data)
