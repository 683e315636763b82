"""Blockwise float8 linears (1 x 128 activation blocks, 128 x 128 weight blocks), the parts that need no GPU: the numpy casts against the
reference's recorded bytes, PerBlock, the config and its JSON, get_block_size, the C ABI's argument checks and the route query
(tests/fp8_block_ref.py, tests/golden/fp8_block.npz, tests/golden/fp8_block_configs.json)."""
import ctypes
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import fp8_block_ref as R
from ao_amd import _lib, ops
from ao_amd.quantization import (Float8DynamicActivationFloat8WeightConfig, Float8MMConfig, Float8WeightOnlyConfig,
                                 Int8DynamicActivationInt8WeightConfig, Int8StaticActivationInt8WeightConfig, KernelPreference, PerBlock, PerRow,
                                 PerTensor, config_from_dict, config_to_dict, quantize_)
from ao_amd.quantization.granularity import get_block_size

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "fp8_block.npz"))
with open(os.path.join(HERE, "golden", "fp8_block_configs.json")) as fh:
    UPSTREAM = json.load(fh)
with open(os.path.join(os.path.dirname(HERE), "include", "ao_mi355.h")) as fh:
    SEAM = int(re.search(r"#define AO_FP8_BLOCK_STREAM_MAX_ROWS (\d+)", fh.read()).group(1))
NEW = ["ao_fp8_quantize_block_1x128", "ao_fp8_quantize_block_128x128", "ao_fp8_block_linear", "ao_fp8_block_dynamic_linear_fits",
       "ao_fp8_block_dynamic_linear", "ao_fp8_block_linear_route", "ao_fp8_block_linear_kernel_name", "ao_fp8_block_linear_set_form"]
PAIR = [PerBlock([1, 128]), PerBlock([128, 128])]


# ---- the numpy restatement against the reference's bytes ---------------------------------------------------------------------------
def test_weight_cast_equals_the_fixture():
    q, s = R.cast_128x128(GOLDEN["w"])
    assert R.same_codes(q, GOLDEN["w_q"])
    np.testing.assert_array_equal(s, GOLDEN["w_s"])
    # the all-zero block: scale 0, every code NaN; the saturating block: 3e38 at 448, its small neighbours flushed to zero
    assert s[1, 0] == 0.0 and R.is_nan_code(GOLDEN["w_q"][128:256, 0:128]).all()
    assert GOLDEN["w_q"][5, 300] == 0x7E and (GOLDEN["w_q"][0:128, 256:384] & 0x7F == 0).sum() == 128 * 128 - 1


@pytest.mark.parametrize("name", ["seeded", "edge", "x3d"])
def test_activation_cast_equals_the_fixture(name):
    x = GOLDEN[f"{name}_x"]
    q, s = R.cast_1x128(x.reshape(-1, x.shape[-1]))
    assert R.same_codes(q.reshape(x.shape), GOLDEN[f"{name}_q"])
    np.testing.assert_array_equal(s.reshape(GOLDEN[f"{name}_s"].shape), GOLDEN[f"{name}_s"])


def _same_bf16(a, b):
    nan = lambda v: (v & 0x7FFF) > 0x7F80  # noqa: E731
    return np.array_equal(nan(a), nan(b)) and np.array_equal(np.where(nan(a), 0, a), np.where(nan(b), 0, b))


def test_dequantize_and_slice_equal_the_fixture():
    assert _same_bf16(R.dequantize(GOLDEN["w_q"], GOLDEN["w_s"], 128, 128), GOLDEN["w_dequant"])
    np.testing.assert_array_equal(GOLDEN["w_slice_q"], GOLDEN["w_q"][128:256, 128:384])
    np.testing.assert_array_equal(GOLDEN["w_slice_s"], GOLDEN["w_s"][1:2, 1:3])
    assert _same_bf16(R.dequantize(GOLDEN["w_slice_q"], GOLDEN["w_slice_s"], 128, 128), GOLDEN["w_slice_dequant"])


def test_chain_and_float64_agree_on_exact_sums():
    """Integer codes |q| <= 15 and power-of-two scales within 2^7: every partial sum is exact in fp32, so the chain is the float64 sum."""
    g = np.random.default_rng(0)
    M, N, K = 33, 130, 384
    from oracle import bf16, fp8_ref

    aq = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (M, K)).astype(np.float32))
    bq = fp8_ref.f32_to_e4m3(g.integers(-15, 16, (N, K)).astype(np.float32))
    a_s = np.exp2(g.integers(-3, 4, (M, K // 128))).astype(np.float32)
    b_s = np.exp2(g.integers(-3, 4, (2, K // 128))).astype(np.float32)
    y, _ = R.linear_f64(aq, a_s, bq, b_s)
    assert np.array_equal(y, y.astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(R.chain_bits(aq, a_s, bq, b_s), bf16.to_bits(bf16.bf16_round(y.astype(np.float32))))


# ---- PerBlock ----------------------------------------------------------------------------------------------------------------------
def test_per_block_equality_hash_and_safe_globals():
    assert PerBlock([1, 128]) == PerBlock((1, 128)) and hash(PerBlock([1, 128])) == hash(PerBlock((1, 128)))
    assert PerBlock([1, 128]) != PerBlock([128, 128]) and PerBlock([128, 128]) != PerRow()
    assert len({PerBlock([1, 128]), PerBlock((1, 128)), PerBlock([128, 128])}) == 2
    with pytest.raises(ValueError):
        PerBlock([])
    buf = io.BytesIO()
    torch.save({"g": PerBlock([128, 128]), "pair": PAIR}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)
    assert back["g"] == PerBlock((128, 128)) and back["pair"] == PAIR


def test_get_block_size():
    assert tuple(get_block_size((256, 384), PerBlock([128, 128]))) == (128, 128)
    assert tuple(get_block_size((7, 384), PerBlock([1, 128]))) == (1, 128)
    assert tuple(get_block_size((3, 5, 384), PerBlock([1, 128]))) == (1, 1, 128)       # left-padded with 1s
    assert tuple(get_block_size((4, 256, 384), PerBlock((128, 128)))) == (1, 128, 128)
    with pytest.raises(AssertionError, match=r"\(200, 384\)"):
        get_block_size((200, 384), PerBlock([128, 128]))
    with pytest.raises(AssertionError, match="are divisible by block size"):
        get_block_size((256, 100), PerBlock([1, 128]))
    with pytest.raises(AssertionError, match="same number of dimensions"):
        get_block_size((384,), PerBlock([128, 128]))


# ---- the config --------------------------------------------------------------------------------------------------------------------
def test_config_accepts_the_pair():
    c = Float8DynamicActivationFloat8WeightConfig(granularity=PAIR)
    assert c.granularity == PAIR and c.mm_config == Float8MMConfig(use_fast_accum=False) and c.version == 2
    assert Float8DynamicActivationFloat8WeightConfig(granularity=(PerBlock((1, 128)), PerBlock((128, 128)))).granularity == PAIR
    assert Float8DynamicActivationFloat8WeightConfig(granularity=PAIR, kernel_preference=KernelPreference.TORCH).granularity == PAIR
    assert Float8DynamicActivationFloat8WeightConfig(granularity=PAIR, mm_config=Float8MMConfig(use_fast_accum=True)).mm_config.use_fast_accum
    # the other granularities keep their default
    assert Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()).mm_config == Float8MMConfig(use_fast_accum=True)
    assert Float8DynamicActivationFloat8WeightConfig().granularity == [PerTensor(), PerTensor()]


@pytest.mark.parametrize("gran", [PerBlock([128, 128]), PerBlock([1, 128]), [PerBlock([128, 128]), PerBlock([1, 128])],
                                  [PerBlock([1, 128]), PerBlock([1, 128])], [PerBlock([128, 128]), PerBlock([128, 128])],
                                  [PerBlock([1, 64]), PerBlock([128, 128])], [PerBlock([1, 128]), PerBlock([64, 64])],
                                  [PerRow(), PerBlock([128, 128])], [PerBlock([1, 128]), PerRow()], [PerBlock([1, 128]), PerTensor()]])
def test_config_refuses_every_other_per_block(gran):
    with pytest.raises(ValueError, match="Unsupported granularity types"):
        Float8DynamicActivationFloat8WeightConfig(granularity=gran)


def test_config_block_pair_conditions():
    with pytest.raises(NotImplementedError, match="kernel_preference"):
        Float8DynamicActivationFloat8WeightConfig(granularity=PAIR, kernel_preference=KernelPreference.TRITON)
    with pytest.raises(ValueError, match="version >= 2"):
        Float8DynamicActivationFloat8WeightConfig(granularity=PAIR, version=1)
    with pytest.raises(ValueError, match="activation_value"):
        Float8DynamicActivationFloat8WeightConfig(granularity=PAIR, activation_value_lb=1e-12)
    with pytest.raises(ValueError, match="activation_value"):
        Float8DynamicActivationFloat8WeightConfig(granularity=PAIR, activation_value_ub=100.0)


@pytest.mark.parametrize("cls", [Int8DynamicActivationInt8WeightConfig, Int8StaticActivationInt8WeightConfig])
@pytest.mark.parametrize("gran", [PerBlock([128, 128]), [PerBlock([1, 128]), PerBlock([128, 128])], [PerRow(), PerBlock([128, 128])]])
def test_int8_configs_refuse_per_block(cls, gran):
    with pytest.raises(ValueError, match="Unsupported granularity types"):
        cls(granularity=gran)


def test_weight_only_config_refuses_block_granularities():
    with pytest.raises(AssertionError, match="granularity"):
        Float8WeightOnlyConfig(granularity=PerBlock([128, 128]))


def test_config_json_equals_upstream_both_ways():
    want = UPSTREAM["Float8DynamicActivationFloat8WeightConfig_block"]
    cfg = Float8DynamicActivationFloat8WeightConfig(granularity=PAIR, set_inductor_config=want["_data"]["set_inductor_config"])
    ours = config_to_dict(cfg)
    assert ours == want                                   # what upstream writes
    assert ours["_data"]["granularity"][0]["_data"]["block_size"] == [1, 128]
    assert ours["_data"]["mm_config"]["_data"]["use_fast_accum"] is False
    assert json.loads(json.dumps(ours)) == ours
    assert config_from_dict(want) == cfg                  # upstream's JSON decodes
    assert config_to_dict(config_from_dict(json.loads(json.dumps(want)))) == want
    # a tuple block_size is written as a list too
    assert config_to_dict(Float8DynamicActivationFloat8WeightConfig(granularity=[PerBlock((1, 128)), PerBlock((128, 128))],
                                                                     set_inductor_config=True)) == want


def test_quantize_skips_incompatible_weights_and_names_bad_shapes():
    """A linear whose weight fails the float8 shape rule is left alone, as today; a shape the block does not divide raises and names it
    (before any kernel: no GPU needed)."""
    lin = torch.nn.Linear(24, 8, dtype=torch.bfloat16)
    quantize_(lin, Float8DynamicActivationFloat8WeightConfig(granularity=PAIR))
    assert type(lin.weight) is torch.nn.Parameter
    lin = torch.nn.Linear(128, 48, dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match=r"\(48, 128\)"):
        quantize_(lin, Float8DynamicActivationFloat8WeightConfig(granularity=PAIR))


# ---- subclass refusals that need no kernel -------------------------------------------------------------------------------------------
def _raw_weight(n=256, k=384, act=True, block=(128, 128)):
    from ao_amd.quantization import Float8Tensor, QuantizeTensorToFloat8Kwargs

    kw = QuantizeTensorToFloat8Kwargs(granularity=PerBlock([1, 128])) if act else None
    return Float8Tensor(torch.zeros(n, k, dtype=torch.float8_e4m3fn), torch.ones((n + 127) // 128, k // 128), list(block), torch.bfloat16, kw)


def test_refusals_name_blockwise():
    import torch.nn.functional as F

    from ao_amd.quantization import Float8Tensor, QuantizeTensorToFloat8Kwargs

    w = _raw_weight()
    x = torch.zeros(2, 384, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="blockwise"):
        torch.cat([w, w], dim=0)
    with pytest.raises(NotImplementedError, match="blockwise"):
        torch.split(w, 128, 0)
    with pytest.raises(NotImplementedError, match="blockwise"):
        F.linear(x, _raw_weight(act=False))                      # weight-only
    with pytest.raises(NotImplementedError, match="blockwise"):
        F.linear(x.to(torch.float16), w)                         # no fp16 / fp32 slow path
    with pytest.raises(NotImplementedError, match="blockwise"):
        F.linear(x.to(torch.float32), w)
    w3 = Float8Tensor(torch.zeros(2, 256, 384, dtype=torch.float8_e4m3fn), torch.ones(2, 2, 3), [1, 128, 128], torch.bfloat16,
                      QuantizeTensorToFloat8Kwargs(granularity=PerBlock([1, 128])))
    with pytest.raises(NotImplementedError, match="blockwise"):
        F.linear(x, w3)                                          # 3-D weights
    with pytest.raises(NotImplementedError, match="blockwise"):
        torch._grouped_mm(torch.zeros(4, 384, dtype=torch.bfloat16), w3.transpose(-2, -1), offs=torch.tensor([2, 4], dtype=torch.int32))
    # a blockwise weight under rowwise activations, and a rowwise weight under blockwise activations
    wr = Float8Tensor(torch.zeros(256, 384, dtype=torch.float8_e4m3fn), torch.ones(2, 3), [128, 128], torch.bfloat16,
                      QuantizeTensorToFloat8Kwargs(granularity=PerRow()))
    with pytest.raises(NotImplementedError, match="blockwise"):
        F.linear(x, wr)
    with pytest.raises(NotImplementedError, match="blockwise"):
        F.linear(x, _raw_weight(block=(1, 384)))
    with pytest.raises(NotImplementedError, match="blockwise"):
        Float8Tensor.from_hp(torch.zeros(2, 128, 128, dtype=torch.bfloat16), granularity=PerBlock([128, 128]))
    with pytest.raises(NotImplementedError, match="blockwise"):
        Float8Tensor.from_hp(torch.zeros(128, 128, dtype=torch.bfloat16), granularity=PerBlock([64, 64]))


def test_slice_and_transpose_follow_the_blocks():
    w = _raw_weight()
    w.scale.copy_(torch.arange(6, dtype=torch.float32).reshape(2, 3))
    s = w[128:256, 128:384]
    assert s.shape == (128, 256) and list(s.block_size) == [128, 128] and torch.equal(s.scale, torch.tensor([[4.0, 5.0]]))
    assert torch.equal(w[0:128].scale, torch.tensor([[0.0, 1.0, 2.0]]))
    t = w.t()
    assert t.shape == (384, 256) and list(t.block_size) == [128, 128] and tuple(t.scale.shape) == (3, 2)
    for bad in (lambda: w[64:256], lambda: w[:, 0:200], lambda: w[0:100]):
        with pytest.raises(NotImplementedError, match="multiples of 128"):
            bad()
    assert w.dequantize().shape == (256, 384)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_new_symbols():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW:
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    for name in ("fp8_quantize_block_1x128", "fp8_quantize_block_128x128", "fp8_block_linear", "fp8_block_linear_kernel_name",
                 "fp8_block_linear_route"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    import ao_amd.quantization as Q

    assert Q.PerBlock is PerBlock


def test_argument_checks_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    lin, dyn = lib.ao_fp8_block_linear, lib.ao_fp8_block_dynamic_linear
    INV, NUL = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_ERR_NULL_POINTER
    for M, N, K in ((4, 16, 64), (4, 16, 192), (4, 16, 0), (4, 0, 128), (-1, 16, 128), (4, 16, 1 << 31), (1 << 20, 16, 1 << 12), (16, 1 << 20, 1 << 12)):
        assert lin(p, p, p, p, None, p, M, N, K, None) == INV, (M, N, K)
        assert "bad shape" in lib.ao_last_error().decode()
        assert dyn(p, p, p, None, p, M, N, K, None) == INV, (M, N, K)
    assert lin(None, p, p, p, None, p, 4, 16, 128, None) == NUL
    assert lin(p, None, p, p, None, p, 4, 16, 128, None) == NUL      # a call without activation scales
    assert lin(p, p, None, p, None, p, 4, 16, 128, None) == NUL
    assert lin(p, p, p, None, None, p, 4, 16, 128, None) == NUL      # a call without weight scales
    assert lin(p, p, p, p, None, None, 4, 16, 128, None) == NUL
    assert dyn(None, p, p, None, p, 4, 16, 128, None) == NUL
    assert dyn(p, p, None, None, p, 4, 16, 128, None) == NUL
    assert lin(p + 8, p, p, p, None, p, 4, 16, 128, None) == INV     # codes not 16-byte aligned
    assert lin(p, p + 2, p, p, None, p, 4, 16, 128, None) == INV     # scales not 4-byte aligned
    assert dyn(p + 8, p, p, None, p, 4, 16, 128, None) == INV
    assert lin(None, None, p, p, None, None, 0, 16, 128, None) == _lib.AO_OK   # M = 0: nothing to launch
    assert dyn(None, p, p, None, None, 0, 16, 128, None) == _lib.AO_OK
    assert dyn(p, p, p, None, p, SEAM + 1, 16, 128, None) == INV     # the tiled form has no fused cast
    assert "tiled form" in lib.ao_last_error().decode()
    for cast in (lib.ao_fp8_quantize_block_1x128, lib.ao_fp8_quantize_block_128x128):
        assert cast(p, p, p, 128, 64, None) == INV
        assert cast(p, p, p, 128, 192, None) == INV
        assert cast(None, p, p, 128, 128, None) == NUL
        assert cast(p, None, p, 128, 128, None) == NUL
        assert cast(p, p, None, 128, 128, None) == NUL
        assert cast(p + 2, p, p, 128, 128, None) == INV
        assert cast(None, None, None, 0, 128, None) == _lib.AO_OK
    assert lib.ao_fp8_quantize_block_128x128(p, p, p, 200, 128, None) == INV
    out = (ctypes.c_int32 * 7)()
    assert lib.ao_fp8_block_linear_route(1, 16, 128, None, 7) == NUL
    assert lib.ao_fp8_block_linear_route(1, 16, 128, out, 6) == INV
    assert lib.ao_fp8_block_linear_set_form(3) == INV and lib.ao_fp8_block_linear_set_form(-1) == INV


def test_route_fields_at_the_seam_and_the_grid_cap():
    assert SEAM == 192
    r = ops.fp8_block_linear_route(1, 4096, 4096)
    assert r == {"kernel": "fp8_block_stream_kernel", "waves": 8, "m_tiles": 1, "tile_m": 16, "tile_n": 16, "grid": (256, 1)}
    r = ops.fp8_block_linear_route(64, 130, 256)
    assert r == {"kernel": "fp8_block_stream_kernel", "waves": 2, "m_tiles": 4, "tile_m": 64, "tile_n": 16, "grid": (9, 1)}
    r = ops.fp8_block_linear_route(SEAM, 130, 256)  # 64 rows a grid row
    assert r == {"kernel": "fp8_block_stream_kernel", "waves": 2, "m_tiles": 4, "tile_m": 64, "tile_n": 16, "grid": (9, 3)}
    r = ops.fp8_block_linear_route(SEAM + 1, 130, 256)
    assert r == {"kernel": "fp8_block_tile_kernel", "waves": 4, "m_tiles": 4, "tile_m": 128, "tile_n": 128, "grid": (2, 2)}
    assert ops.fp8_block_linear_route(17, 257, 1152)["m_tiles"] == 2 and ops.fp8_block_linear_route(17, 257, 1152)["waves"] == 8
    assert ops.fp8_block_linear_route(0, 16, 128)["kernel"] == "fp8_block_stream_kernel"
    for bad in ((1, 16, 64), (1, 16, 192), (1, 0, 128), (-1, 16, 128), (1 << 20, 16, 1 << 12)):
        assert ops.fp8_block_linear_route(*bad)["kernel"] == "invalid"
        assert ops.fp8_block_linear_kernel_name(*bad) == "invalid"
    # rows ride on grid y, which ends at 65535: 128 rows a tile
    assert ops.fp8_block_linear_route(65535 * 128, 128, 128)["grid"] == (1, 65535)
    assert ops.fp8_block_linear_route(65535 * 128 + 1, 128, 128)["kernel"] == "invalid"
    try:
        ops.fp8_block_linear_set_form(1)
        assert ops.fp8_block_linear_route(65535 * 64, 128, 128)["grid"] == (8, 65535)
        assert ops.fp8_block_linear_route(65535 * 64 + 1, 128, 128)["kernel"] == "invalid"
        assert ops.fp8_block_linear_kernel_name(300, 128, 128) == "fp8_block_stream_kernel"
        ops.fp8_block_linear_set_form(2)
        assert ops.fp8_block_linear_kernel_name(1, 128, 128) == "fp8_block_tile_kernel"
    finally:
        ops.fp8_block_linear_set_form(0)
    assert ops.fp8_block_linear_kernel_name(1, 128, 128) == "fp8_block_stream_kernel"


def test_dynamic_linear_fits_agrees_with_the_route():
    lib = _lib.lib()
    for M in (0, 1, 16, 17, 64, 65, 129, SEAM - 1, SEAM, SEAM + 1, 300):
        for N, K in ((17, 128), (130, 256), (384, 1152)):
            assert lib.ao_fp8_block_dynamic_linear_fits(M, N, K) == (1 if ops.fp8_block_linear_kernel_name(M, N, K) == "fp8_block_stream_kernel" else 0)
    assert lib.ao_fp8_block_dynamic_linear_fits(1, 16, 64) == 0


def test_ops_refuse_cpu_tensors_and_bad_scales():
    x = torch.zeros(2, 256, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fp8_block_linear(x, torch.zeros(16, 256, dtype=torch.float8_e4m3fn), torch.ones(1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fp8_quantize_block_1x128(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fp8_quantize_block_128x128(torch.zeros(128, 128, dtype=torch.bfloat16))


def test_fake_kernels_trace_shapes():
    import ao_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty(5, 256, dtype=torch.bfloat16, device="cuda")
        y = torch.ops.ao_mi355.fp8_block_linear(x, torch.empty(130, 256, dtype=torch.float8_e4m3fn, device="cuda"),
                                                torch.empty(2, 2, device="cuda"), None)
        assert y.shape == (5, 130) and y.dtype == torch.bfloat16
        q, s = torch.ops.ao_mi355.fp8_quantize_block_1x128(torch.empty(3, 5, 256, dtype=torch.bfloat16, device="cuda"))
        assert q.shape == (3, 5, 256) and q.dtype == torch.float8_e4m3fn and s.shape == (3, 5, 2) and s.dtype == torch.float32
        q, s = torch.ops.ao_mi355.fp8_quantize_block_128x128(torch.empty(256, 384, dtype=torch.bfloat16, device="cuda"))
        assert q.shape == (256, 384) and s.shape == (2, 3)
