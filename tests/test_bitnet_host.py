"""BitNet b1.58 without a GPU: the ABI, the pack / unpack pair over every byte, each named refusal, the quantize_ handlers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bitnet_ref as R
from ao_amd import _lib, ops
from ao_amd.prototype import quantized_training as Q
from ao_amd.quantization import quantize_


def test_abi_declared_and_exported():
    lib, declared = _lib.lib(), _lib.declared_symbols()
    for name, nargs in (("ao_bitnet_absmean", 6), ("ao_bitnet_quantize_weight", 7), ("ao_bitnet_dequantize", 5), ("ao_bitnet_quantize_act", 6),
                        ("ao_bitnet_mm_fits", 3), ("ao_bitnet_mm", 11)):
        assert hasattr(lib, name) and name in declared and len(_lib._SIGNATURES[name]) == nargs
    for name in ("bitnet_absmean", "bitnet_quantize_weight", "bitnet_dequantize", "bitnet_quantize_act", "bitnet_mm", "bitnet_mm_fits", "bitnet_linear"):
        assert name in ops.__all__
    assert hasattr(torch.ops.ao_mi355, "bitnet_linear")


def test_pack_unpack_round_trip_over_every_byte():
    every = torch.arange(-128, 128, dtype=torch.int8).reshape(8, 32)
    fields = Q._unpack_i2_in_i8(every)
    assert fields.shape == (8, 128) and fields.dtype == torch.int8 and fields.min() == -2 and fields.max() == 1
    assert torch.equal(Q._pack_i2_in_i8(fields), every)
    assert np.array_equal(fields.numpy(), R.unpack(every.numpy())) and np.array_equal(R.pack(fields.numpy()), every.numpy())
    assert Q._pack_i2_in_i8(torch.tensor([[1, -1, 0, 1]], dtype=torch.int8)).item() == 0b01110001


@pytest.mark.parametrize("m,n,k,word", [(4, 16, 100, "multiple of 64"), (4, 16, 0, "bad shape"), (2 ** 19 + 1, 16, 64, "too large")])
def test_mm_fits_names_each_refusal(m, n, k, word):
    assert ops.bitnet_mm_fits(17, 150, 832) is None
    assert word in ops.bitnet_mm_fits(m, n, k)


def test_named_refusals():
    lin = torch.nn.Linear(64, 16, dtype=torch.bfloat16)
    w = Q.BitNetTrainingLinearWeight(lin.weight.detach())
    with pytest.raises(NotImplementedError, match="fsdp_pre_all_gather"):
        w.fsdp_pre_all_gather(None)
    with pytest.raises(NotImplementedError, match="fsdp_post_all_gather"):
        w.fsdp_post_all_gather((), None, torch.bfloat16)
    with pytest.raises(NotImplementedError, match="precompute_bitnet_scale_for_fsdp"):
        Q.precompute_bitnet_scale_for_fsdp(lin)
    torch.set_autocast_enabled("cuda", True)  # (the context manager switches itself off where there is no GPU)
    try:
        with pytest.raises(NotImplementedError, match="autocast"):
            F.linear(torch.zeros(2, 64, dtype=torch.bfloat16), w)
    finally:
        torch.set_autocast_enabled("cuda", False)
    for dtype in (torch.float16, torch.float32):
        with pytest.raises(NotImplementedError, match="float16 and float32 are not built"):
            quantize_(torch.nn.Linear(64, 16, dtype=dtype), Q.BitNetTrainingConfig())
        with pytest.raises(NotImplementedError, match="float16 and float32 are not built"):
            F.linear(torch.zeros(2, 64, dtype=dtype), w)
    with pytest.raises(ValueError, match="K=100 must be a multiple of 64"):
        quantize_(torch.nn.Linear(100, 16, dtype=torch.bfloat16), Q.BitNetInferenceConfig())


def test_quantize_handler_swaps_the_weight_class():
    model = torch.nn.Sequential(torch.nn.Linear(64, 32, dtype=torch.bfloat16), torch.nn.ReLU(), torch.nn.Linear(32, 8, dtype=torch.bfloat16))
    before = [m.weight.detach().clone() for m in (model[0], model[2])]
    quantize_(model, Q.bitnet_training())
    for m, w in zip((model[0], model[2]), before):
        assert isinstance(m.weight, Q.BitNetTrainingLinearWeight) and isinstance(m.weight, torch.nn.Parameter) and m.weight.requires_grad
        assert m.weight.shape == w.shape and m.weight.dtype == torch.bfloat16 and torch.equal(m.weight._data, w)
    assert isinstance(model[0].weight.t(), Q.BitNetTrainingLinearWeight) and type(model[0].weight + 1) is torch.Tensor
