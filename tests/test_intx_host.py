"""Intx without a GPU: the restatement against the reference's recorded bytes, the configs' defaults and assertions, each named refusal, the ABI."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import intx_ref as R
from ao_amd import _lib, ops
from ao_amd.prototype import IntxBitPackedTensor
from ao_amd.quantization import (Int8DynamicActivationIntxWeightConfig, IntxChooseQParamsAlgorithm, IntxPackingFormat, IntxUnpackedToInt8Tensor,
                                 IntxWeightOnlyConfig, MappingType, PerAxis, PerGroup, PerRow, config_from_dict, config_to_dict, quantize_)

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intx.npz"))


@pytest.mark.parametrize("mapping", R.MAPPINGS)
@pytest.mark.parametrize("b", range(1, 9))
def test_restatement_reproduces_every_recorded_byte(b, mapping):
    for g in (32, 128, 256):
        key = f"b{b}_{mapping}_g{g}"
        q, s, zp = R.from_hp(GOLDEN["w"], b, mapping, g)
        assert np.array_equal(q, GOLDEN[key + "_q"]) and np.array_equal(s, GOLDEN[key + "_s"]) and np.array_equal(zp, GOLDEN[key + "_zp"])
        assert np.array_equal(R.dequantize(q, s, zp), GOLDEN[key + "_dq"])
        assert q.min() >= R.bounds(b)[0] and q.max() <= R.bounds(b)[1]
    assert np.array_equal(R.act_fake_quant(GOLDEN["x"]), GOLDEN["x_fq"])


def test_config_defaults_assertions_and_json():
    c = IntxWeightOnlyConfig()
    assert (c.weight_dtype, c.granularity, c.mapping_type, c.scale_dtype, c.intx_packing_format, c.intx_choose_qparams_algorithm, c.version) == (
        torch.int8, PerAxis(0), MappingType.SYMMETRIC, None, IntxPackingFormat.UNPACKED_TO_INT8, IntxChooseQParamsAlgorithm.AFFINE, 2)
    d = Int8DynamicActivationIntxWeightConfig()
    assert (d.weight_dtype, d.weight_granularity, d.weight_mapping_type, d.weight_scale_dtype, d.act_mapping_type, d.intx_packing_format,
            d.intx_choose_qparams_algorithm, d.version) == (torch.int8, PerGroup(32), MappingType.SYMMETRIC, None, MappingType.ASYMMETRIC,
                                                            IntxPackingFormat.UNPACKED_TO_INT8, IntxChooseQParamsAlgorithm.AFFINE, 2)
    for cls, gran in ((IntxWeightOnlyConfig, "granularity"), (Int8DynamicActivationIntxWeightConfig, "weight_granularity")):
        with pytest.raises(AssertionError, match="weight_dtype must be torch.intx"):
            cls(weight_dtype=torch.int16)
        with pytest.raises(AssertionError, match="must be PerAxis or PerGroup"):
            cls(**{gran: PerRow()})
        with pytest.raises(AssertionError, match="axis must be 0"):
            cls(**{gran: PerAxis(1)})
    with pytest.raises(AssertionError, match="act_mapping_type must be"):
        Int8DynamicActivationIntxWeightConfig(act_mapping_type=MappingType.SYMMETRIC_NO_CLIPPING_ERR)
    for cfg in (IntxWeightOnlyConfig(torch.int3, PerGroup(64), MappingType.ASYMMETRIC, intx_packing_format="bit_packed"),
                Int8DynamicActivationIntxWeightConfig(torch.int4, PerAxis(0))):
        assert config_from_dict(config_to_dict(cfg)) == cfg


def _lin(k=64, n=16, dtype=torch.bfloat16):
    return torch.nn.Linear(k, n, dtype=dtype)


@pytest.mark.parametrize("make,cfg,exc,word", [
    (_lin, IntxWeightOnlyConfig(intx_choose_qparams_algorithm="hqq_scale_only"), NotImplementedError, "HQQ_SCALE_ONLY is not built"),
    (_lin, IntxWeightOnlyConfig(intx_packing_format="opaque_torchao_auto"), NotImplementedError, "opaque_torchao_auto is a CPU kernel's opaque layout"),
    (_lin, Int8DynamicActivationIntxWeightConfig(intx_packing_format="opaque_aten_kleidiai"), NotImplementedError, "opaque_aten_kleidiai is a CPU"),
    (lambda: _lin(dtype=torch.float16), IntxWeightOnlyConfig(), NotImplementedError, "float16 and float32 are not built"),
    (lambda: _lin(dtype=torch.float32), Int8DynamicActivationIntxWeightConfig(), NotImplementedError, "float16 and float32 are not built"),
    (_lin, IntxWeightOnlyConfig(scale_dtype=torch.float32), NotImplementedError, "scale dtype of torch.float32 is not built"),
    (_lin, Int8DynamicActivationIntxWeightConfig(weight_scale_dtype=torch.float16), NotImplementedError, "scale dtype of torch.float16 is not built"),
    (lambda: torch.nn.Conv2d(32, 8, 3, dtype=torch.bfloat16), IntxWeightOnlyConfig(), NotImplementedError, "4-D conv weights are not built"),
    (lambda: torch.nn.Embedding(8, 64, dtype=torch.bfloat16), IntxWeightOnlyConfig(), NotImplementedError, "F.embedding"),
    (lambda: _lin(k=48), IntxWeightOnlyConfig(), ValueError, "K=48 must be a multiple of 32"),
    (_lin, IntxWeightOnlyConfig(granularity=PerGroup(16)), ValueError, "group size 16 must be a multiple of 32 that divides K=64"),
    (lambda: _lin(k=96), Int8DynamicActivationIntxWeightConfig(weight_granularity=PerGroup(64)), ValueError, "group size 64 must be a multiple of 32 that divides K=96"),
    (_lin, Int8DynamicActivationIntxWeightConfig(act_mapping_type=MappingType.SYMMETRIC), NotImplementedError, "act_mapping_type=SYMMETRIC is not built"),
])
def test_named_refusals_before_any_launch(make, cfg, exc, word):
    with pytest.raises(exc, match=word):
        quantize_(make(), cfg, filter_fn=lambda m, fqn: True)


def test_tensor_refusals_and_no_cpu_fallback():
    w = torch.zeros(16, 64, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="float zero-points are not built"):
        IntxUnpackedToInt8Tensor.from_hp(w, (1, 32), torch.int4, intx_choose_qparams_algorithm=None, custom_scale=torch.ones(16, 2, dtype=torch.bfloat16),
                                         custom_zero_point=torch.zeros(16, 2, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IntxUnpackedToInt8Tensor.from_hp(w, (1, 32), torch.int4)
    args = (torch.zeros(16, 2, dtype=torch.bfloat16), torch.zeros(16, 2, dtype=torch.int8), torch.int4, (1, 32), torch.bfloat16, None)
    for t in (IntxUnpackedToInt8Tensor(torch.zeros(16, 64, dtype=torch.int8), *args), IntxBitPackedTensor(torch.zeros(16, 8, dtype=torch.int32), *args)):
        assert t.shape == (16, 64) and t.dtype == torch.bfloat16
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            F.linear(torch.zeros(2, 64, dtype=torch.bfloat16), t)
        with pytest.raises(NotImplementedError, match="F.embedding is not built"):
            F.embedding(torch.zeros(2, dtype=torch.long), t)
    t = IntxUnpackedToInt8Tensor(torch.zeros(16, 64, dtype=torch.int8), *args)
    s = t[4:8, 32:]
    assert s.shape == (4, 32) and s.scale.shape == (4, 1) and s.block_size == (1, 32) and isinstance(s.detach().clone(), IntxUnpackedToInt8Tensor)
    with pytest.raises(AssertionError, match="incompatible with blocking"):
        t[:, 16:]


def test_abi_refuses_shapes_then_null_pointers():
    lib, declared = _lib.lib(), _lib.declared_symbols()
    for name in ("ao_intx_quantize", "ao_int8_fake_quantize_per_token_asym", "ao_intx_pack", "ao_intx_unpack", "ao_intx_dequantize", "ao_intx_linear_fits",
                 "ao_intx_linear_route", "ao_intx_linear_set_form", "ao_intx_linear"):
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    for name in ("intx_quantize", "int8_fake_quantize_per_token_asym", "intx_pack", "intx_unpack", "intx_dequantize", "intx_linear", "intx_linear_fits"):
        assert name in ops.__all__
    assert hasattr(torch.ops.ao_mi355, "intx_linear")
    calls = [
        (lambda: lib.ao_intx_quantize(None, None, None, None, 4, 64, 32, 9, 0, 0, None), "bits must be 1 .. 8"),
        (lambda: lib.ao_intx_quantize(None, None, None, None, 4, 64, 32, 4, 3, 0, None), "mapping must be"),
        (lambda: lib.ao_intx_quantize(None, None, None, None, 4, 64, 24, 4, 0, 0, None), "group_size=24 must be a multiple of 8 that divides K=64"),
        (lambda: lib.ao_intx_pack(None, None, 4, 48, 3, None), "K=48 must be a multiple of 32"),
        (lambda: lib.ao_intx_unpack(None, None, 4, 64, 0, None), "bits must be 1 .. 8"),
        (lambda: lib.ao_intx_dequantize(None, None, None, None, 4, 64, 48, 3, None), "group_size=48 must be a multiple of 32"),
        (lambda: lib.ao_int8_fake_quantize_per_token_asym(None, None, 4, 12, None), "K=12 must be a multiple of 8"),
        (lambda: lib.ao_intx_linear(None, None, None, None, None, None, 4, 16, 80, 16, 4, None), "K must be a multiple of 32"),
        (lambda: lib.ao_intx_linear(None, None, None, None, None, None, 4, 16, 96, 64, 4, None), "multiple of 32 that divides K"),
    ]
    for call, word in calls:
        assert call() == _lib.AO_ERR_INVALID_ARGUMENT and word in _lib.last_error(), (word, _lib.last_error())
    for call in (lambda: lib.ao_intx_quantize(None, None, None, None, 4, 64, 32, 4, 0, 0, None), lambda: lib.ao_intx_pack(None, None, 4, 64, 3, None),
               lambda: lib.ao_intx_unpack(None, None, 4, 64, 3, None), lambda: lib.ao_intx_dequantize(None, None, None, None, 4, 64, 32, 3, None),
               lambda: lib.ao_int8_fake_quantize_per_token_asym(None, None, 4, 64, None), lambda: lib.ao_intx_linear(None, None, None, None, None, None, 4, 16, 64, 32, 4, None)):
        assert call() == _lib.AO_ERR_NULL_POINTER and "null pointer" in _lib.last_error()
    assert ops.intx_linear_fits(3, 17, 40, 320, 64) is None and "multiple of 32" in ops.intx_linear_fits(3, 17, 40, 300, 100)
    seam = 64
    assert ops.intx_linear_route(3, seam, 40, 320, 64)[0] == 1 and ops.intx_linear_route(3, seam + 1, 40, 320, 64)[0] == 2
