"""int8 / float8 weight-only linears, the parts that need no GPU: the restated arithmetic against the reference's recorded outputs, the
configs and their JSON, quantize_ dispatch, the C ABI's argument checks and the route query (tests/wo8_ref.py, tests/golden/wo8.npz,
tests/golden/wo8_configs.json)."""
import ctypes
import json
import os
import threading

import numpy as np
import pytest
import torch

import wo8_ref as R
from ao_amd import _lib, ops
from ao_amd.quantization import (Float8WeightOnlyConfig, FqnToConfig, Int8WeightOnlyConfig, PerGroup, PerRow, PerTensor, config_from_dict,
                                 config_to_dict, quantize_)
from ao_amd.quantization import quant_api

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "wo8.npz"))
with open(os.path.join(HERE, "golden", "wo8_configs.json")) as fh:
    UPSTREAM = json.load(fh)
NEW = ["ao_wo8_linear", "ao_wo8_linear_route", "ao_wo8_linear_set_form"]


def bf(name):
    return torch.from_numpy(GOLDEN[name].view(np.int16)).view(torch.bfloat16)


def codes(fmt, name):
    q = torch.from_numpy(GOLDEN[name])
    return q if fmt == "int8" else q.view(torch.float8_e4m3fn)


@pytest.mark.parametrize("fmt", ["int8", "e4m3"])
@pytest.mark.parametrize("gran", ["row", "tensor"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_ref_reproduces_the_reference_bit_for_bit(fmt, gran, with_bias):
    x, bias = bf("x"), bf("bias")
    q, s = codes(fmt, f"{fmt}_{gran}_q"), torch.from_numpy(GOLDEN[f"{fmt}_{gran}_s"])
    y = R.linear(R.FMTS[fmt], x, q, s, bias if with_bias else None)
    want = bf(f"{fmt}_{gran}_y" if with_bias else f"{fmt}_{gran}_y_nobias")
    assert torch.equal(R.bits(y), R.bits(want))


def test_ref_one_hot_returns_dequantize():
    q, s = codes("e4m3", "onehot_q"), torch.from_numpy(GOLDEN["onehot_s"])
    x = torch.eye(16, q.shape[1], dtype=torch.bfloat16)
    y = R.linear(R.FMT_E4M3, x, q, s)
    assert torch.equal(R.bits(y), R.bits(bf("onehot_y")))
    assert torch.equal(R.bits(y), R.bits(bf("onehot_dequant")[:, :16].t()))


def test_golden_inputs_have_exact_sums():
    x = bf("x").double()
    assert float(x.abs().max()) <= 8 and torch.equal(x, x.round())
    K = x.shape[1]
    for gran in ("row", "tensor"):
        q = codes("e4m3", f"e4m3_{gran}_q").double()
        assert float(q.abs().max()) <= 15 and torch.equal(q, q.round())
        s = torch.from_numpy(GOLDEN[f"e4m3_{gran}_s"]).double()
        assert torch.equal(torch.log2(s), torch.log2(s).round())
        assert K * 8 * 127 <= 2 ** 22
    assert len(set(GOLDEN["e4m3_row_s"].reshape(-1).tolist())) > 1


# ---- configs -----------------------------------------------------------------------------------------------------------------------
def test_config_defaults():
    c = Int8WeightOnlyConfig()
    assert (c.group_size, c.granularity, c.set_inductor_config, c.version) == (None, PerRow(), True, 2)
    f = Float8WeightOnlyConfig()
    assert (f.weight_dtype, f.set_inductor_config, f.version, f.granularity) == (torch.float8_e4m3fn, True, 2, PerRow())
    import dataclasses

    assert [x.name for x in dataclasses.fields(c)] == ["group_size", "granularity", "set_inductor_config", "version"]
    assert [x.name for x in dataclasses.fields(f)] == ["weight_dtype", "set_inductor_config", "version", "granularity"]


def test_config_validation():
    with pytest.raises(ValueError, match="version 1"):
        Int8WeightOnlyConfig(version=1)
    with pytest.raises(AssertionError, match="group_size=None"):
        Int8WeightOnlyConfig(group_size=32)
    with pytest.raises(AssertionError, match="granularity"):
        Int8WeightOnlyConfig(granularity="row")
    with pytest.raises(AssertionError, match="granularity"):
        Float8WeightOnlyConfig(granularity=3)
    with pytest.raises(NotImplementedError, match="float8_e4m3fn"):
        Float8WeightOnlyConfig(weight_dtype=torch.float8_e5m2)
    assert Int8WeightOnlyConfig(granularity=PerGroup(64)).granularity == PerGroup(64)  # parses; quantize_ refuses
    assert Float8WeightOnlyConfig(granularity=PerGroup(64), set_inductor_config=False).set_inductor_config is False


@pytest.mark.parametrize("name", sorted(UPSTREAM))
def test_config_json(name):
    cls = {"Int8WeightOnlyConfig": Int8WeightOnlyConfig, "Float8WeightOnlyConfig": Float8WeightOnlyConfig}[name.split("_")[0]]
    cfg = cls(granularity=PerTensor()) if name.endswith("_tensor") else cls()
    ours = config_to_dict(cfg)
    assert ours == UPSTREAM[name]                       # what upstream writes
    assert json.loads(json.dumps(ours)) == ours
    assert config_from_dict(UPSTREAM[name]) == cfg      # upstream's JSON decodes
    assert config_from_dict(json.loads(json.dumps(ours))) == cfg


def test_fqn_to_config_round_trip_finds_both():
    cfg = FqnToConfig({"a": Int8WeightOnlyConfig(), "re:b.*": Float8WeightOnlyConfig(granularity=PerTensor())})
    back = config_from_dict(json.loads(json.dumps(config_to_dict(cfg))))
    assert back.fqn_to_config["a"] == Int8WeightOnlyConfig()
    assert back.fqn_to_config["re:b.*"] == Float8WeightOnlyConfig(granularity=PerTensor())


def test_quantize_dispatch_through_fqn_to_config(monkeypatch):
    """Each config reaches its own handler with the module it names; no GPU: the handlers are replaced by recorders."""
    seen = []
    for cls in (Int8WeightOnlyConfig, Float8WeightOnlyConfig):
        assert cls in quant_api._QUANTIZE_CONFIG_HANDLER
        monkeypatch.setitem(quant_api._QUANTIZE_CONFIG_HANDLER, cls, lambda m, c, **kw: (seen.append((type(c).__name__, m.in_features)), m)[1])
    model = torch.nn.Sequential(torch.nn.Linear(32, 16), torch.nn.Linear(16, 48), torch.nn.Linear(48, 8))
    quantize_(model, FqnToConfig({"0": Int8WeightOnlyConfig(), "re:1": Float8WeightOnlyConfig(), "2": None}))
    assert seen == [("Int8WeightOnlyConfig", 32), ("Float8WeightOnlyConfig", 16)]


@pytest.mark.parametrize("cfg", [Int8WeightOnlyConfig(granularity=PerGroup(32)), Float8WeightOnlyConfig(granularity=PerGroup(32))])
def test_quantize_refuses_per_group_with_the_reason(cfg):
    lin = torch.nn.Linear(64, 16, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="per-group 8-bit weights are not implemented"):
        quantize_(lin, cfg)
    assert type(lin.weight) is torch.nn.Parameter


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_new_symbols():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW:
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    assert lib.ao_abi_version() == 2


def test_argument_checks_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = lambda *a: lib.ao_wo8_linear(*a)  # noqa: E731
    assert ok(0, p, None, p, 16, None, p, 4, 16, 64, None) == _lib.AO_ERR_NULL_POINTER
    assert ok(0, p, p, None, 16, None, p, 4, 16, 64, None) == _lib.AO_ERR_NULL_POINTER
    assert ok(1, None, p, p, 16, None, p, 4, 16, 64, None) == _lib.AO_ERR_NULL_POINTER
    assert ok(1, p, p, p, 16, None, None, 4, 16, 64, None) == _lib.AO_ERR_NULL_POINTER
    for M, N, K in ((4, 16, 72), (4, 16, 0), (4, 16, 8), (4, 0, 64), (-1, 16, 64), (4, 16, 1 << 31), (1, 1, (1 << 31) - 16), (1, 1, (1 << 31) - 1008),
                    (1 << 20, 16, 1 << 12)):
        assert ok(0, p, p, p, N, None, p, M, N, K, None) == _lib.AO_ERR_INVALID_ARGUMENT, (M, N, K)
        assert "bad shape" in lib.ao_last_error().decode()
    for fmt in (-1, 2, 4):
        assert ok(fmt, p, p, p, 16, None, p, 4, 16, 64, None) == _lib.AO_ERR_INVALID_ARGUMENT
        assert "fmt" in lib.ao_last_error().decode()
    assert ok(0, p, p, p, 7, None, p, 4, 16, 64, None) == _lib.AO_ERR_INVALID_ARGUMENT  # scale_count neither N nor 1
    assert ok(0, p + 2, p, p, 16, None, p, 4, 16, 64, None) == _lib.AO_ERR_INVALID_ARGUMENT  # x not 16-byte aligned
    assert ok(0, p, p, p + 2, 16, None, p, 4, 16, 64, None) == _lib.AO_ERR_INVALID_ARGUMENT  # scale not 4-byte aligned
    for fmt in (0, 1):
        assert ok(fmt, None, p, p, 16, None, None, 0, 16, 64, None) == _lib.AO_OK  # M = 0: nothing to launch
        assert ok(fmt, None, p, p, 1, None, None, 0, 16, 64, None) == _lib.AO_OK
    out = (ctypes.c_int32 * 7)()
    assert lib.ao_wo8_linear_route(0, 1, 16, 64, None, 7) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_wo8_linear_route(0, 1, 16, 64, out, 6) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_wo8_linear_set_form(3) == _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_wo8_linear_set_form(-1) == _lib.AO_ERR_INVALID_ARGUMENT


def test_route_answers_on_the_cpu():
    for fmt in (ops.WO8_FMT_INT8, ops.WO8_FMT_E4M3):
        r = ops.wo8_route(fmt, 1, 4096, 4096)
        assert r == {"kernel": "wo8_stream_kernel", "waves": 8, "m_tiles": 1, "tile_m": 16, "tile_n": 16, "grid": (256, 1)}
        assert ops.wo8_route(fmt, 17, 1000, 4096)["m_tiles"] == 2 and ops.wo8_route(fmt, 17, 1000, 4096)["grid"] == (63, 1)
        assert ops.wo8_route(fmt, 64, 28672, 4096)["waves"] == 4
        assert ops.wo8_route(fmt, 1, 48, 16)["waves"] == 1
        r = ops.wo8_route(fmt, 65, 1000, 4096)
        assert r == {"kernel": "wo8_tile_kernel", "waves": 4, "m_tiles": 4, "tile_m": 64, "tile_n": 64, "grid": (16, 2)}
        for bad in ((1, 16, 24), (1, 0, 64), (-1, 16, 64), (1, 16, 0), (1 << 20, 16, 1 << 12)):
            assert ops.wo8_route(fmt, *bad)["kernel"] == "invalid"
        assert ops.wo8_route(fmt, 0, 16, 64)["kernel"] == "wo8_stream_kernel"
    assert ops.wo8_route(2, 1, 16, 64)["kernel"] == "invalid"


def test_set_form_forces_each_form_and_is_thread_local():
    try:
        ops.wo8_set_form(2)
        assert ops.wo8_route(0, 1, 4096, 4096)["kernel"] == "wo8_tile_kernel"
        other = []
        t = threading.Thread(target=lambda: other.append(ops.wo8_route(0, 1, 4096, 4096)["kernel"]))
        t.start()
        t.join()
        assert other == ["wo8_stream_kernel"]
        ops.wo8_set_form(1)
        r = ops.wo8_route(1, 4096, 4096, 4096)
        assert r["kernel"] == "wo8_stream_kernel" and r["m_tiles"] == 4 and r["grid"] == (256, 64)
    finally:
        ops.wo8_set_form(0)
    assert ops.wo8_route(0, 1, 4096, 4096)["kernel"] == "wo8_stream_kernel"
    assert ops.wo8_route(0, 4096, 4096, 4096)["kernel"] == "wo8_tile_kernel"


def test_largest_k_routes():
    """K up to 2^31 - 1024 (the kernels step through k in 32 bits); beyond it nothing takes the shape."""
    assert ops.wo8_route(0, 1, 1, (1 << 31) - 1024)["kernel"] == "wo8_stream_kernel"
    assert ops.wo8_route(0, 1, 1, (1 << 31) - 1008)["kernel"] == "invalid"


@pytest.mark.parametrize("cls_name", ["Int8Tensor", "Float8Tensor"])
def test_per_group_scales_refuse_with_the_reason(cls_name):
    """A weight whose scale is neither one per row nor one per tensor (a PerGroup checkpoint upstream wrote) loads and refuses to run,
    naming why -- before any kernel is reached, so without a GPU."""
    import torch.nn.functional as F

    import ao_amd.quantization as Q

    q = torch.zeros(16, 64, dtype=torch.int8 if cls_name == "Int8Tensor" else torch.float8_e4m3fn)
    w = getattr(Q, cls_name)(q, torch.ones(16, 2), [1, 32], torch.bfloat16)
    with pytest.raises(NotImplementedError, match="PerRow / PerTensor weight scales"):
        F.linear(torch.zeros(2, 64, dtype=torch.bfloat16), w)


def test_ops_refuse_cpu_tensors():
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.int8_wo_linear(x, torch.zeros(16, 64, dtype=torch.int8), torch.ones(16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fp8_wo_linear(x, torch.zeros(16, 64, dtype=torch.float8_e4m3fn), torch.ones(16))


def test_fake_kernels_trace_shapes():
    import ao_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty(5, 64, dtype=torch.bfloat16, device="cuda")
        for op, dt in ((torch.ops.ao_mi355.int8_wo_linear, torch.int8), (torch.ops.ao_mi355.fp8_wo_linear, torch.float8_e4m3fn)):
            y = op(x, torch.empty(24, 64, dtype=dt, device="cuda"), torch.empty(24, device="cuda"), None)
            assert y.shape == (5, 24) and y.dtype == torch.bfloat16
