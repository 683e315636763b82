"""NF4 (QLoRA) weights on the host: the restated contracts (tests/nf4_ref.py) against the reference's recorded bytes
(tests/golden/nf4.npz), the code rule over every bf16 pattern, the ABI, every Python refusal before the library is touched, the committed
route cases and the route's properties."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nf4_cases as nc  # noqa: E402
import nf4_ref as R  # noqa: E402

from ao_amd import _lib, ops  # noqa: E402
from ao_amd.prototype.nf4_api import NF4WeightOnlyConfig, nf4_weight_only  # noqa: E402
from ao_amd.quantization import LinearNF4, NF4Tensor, linear_nf4, quantize_, to_nf4  # noqa: E402
from ao_amd.quantization.nf4_tensor import NF4_TABLE, SubclassTensorArgs  # noqa: E402

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nf4.npz"))
CASES = ["b64", "two", "straddle", "sb8a", "sb8b", "b32", "b128", "planted", "m0", "exact"]
LINEAR_CASES = [c for c in CASES if c != "planted"]
NEW = ["ao_nf4_block_absmax", "ao_nf4_quantize", "ao_nf4_dequantize", "ao_nf4_linear", "ao_nf4_linear_route", "ao_nf4_linear_kernel_name",
       "ao_nf4_linear_set_form"]
NEW_OPS = ["nf4_block_absmax", "nf4_quantize", "nf4_dequantize", "nf4_linear", "nf4_linear_route", "nf4_linear_kernel_name", "nf4_set_form"]


def meta(c):
    return tuple(int(v) for v in GOLDEN[f"{c}_meta"])


def same(a, b):
    """equal bits, or a NaN in both (its sign and payload are the processor's)"""
    a, b = np.asarray(a), np.asarray(b)
    isnan = lambda v: (v & 0x7FFF) > 0x7F80  # noqa: E731
    return bool(np.all((a == b) | (isnan(a) & isnan(b))))


def bf(name, shape):
    return torch.from_numpy(GOLDEN[name].view(np.int16).copy()).view(torch.bfloat16).reshape(shape)


# ---- 1. the restatement against the recorded bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES)
def test_ref_cast_reproduces_the_reference_bytes(c):
    rows, cols, B, SB = meta(c)
    absmax, codes, q, qf, m0 = R.quantize(GOLDEN[f"{c}_x"], B, SB, GOLDEN[f"{c}_mean"])
    assert np.array_equal(absmax, GOLDEN[f"{c}_absmax"])
    assert np.array_equal(codes, GOLDEN[f"{c}_codes"])
    assert same(qf, GOLDEN[f"{c}_factors"])
    assert np.array_equal(m0, GOLDEN[f"{c}_m0"])
    keep = ~np.repeat(m0, SB)  # (m = 0: the reference's NaN -> int8 is undefined behaviour; recorded, not compared)
    assert np.array_equal(q[keep], GOLDEN[f"{c}_scalers"][keep])
    assert not q[~keep].any()


@pytest.mark.parametrize("c", CASES)
def test_ref_dequantize_reproduces_the_reference_bits(c):
    rows, cols, B, SB = meta(c)
    w = R.dequantize(GOLDEN[f"{c}_codes"], GOLDEN[f"{c}_scalers"], GOLDEN[f"{c}_factors"], GOLDEN[f"{c}_mean"], B, SB)
    assert same(w, GOLDEN[f"{c}_w"].reshape(-1))


def test_fixture_holds_the_cases_it_names():
    assert GOLDEN["m0_m0"].tolist() == [False, True] and not any(GOLDEN[f"{c}_m0"].any() for c in CASES if c != "m0")
    x = R.bf16.from_bits(GOLDEN["planted_x"]).reshape(24, 64)
    codes = R.unpack(GOLDEN["planted_codes"]).reshape(24, 64)
    assert not x[0].any() and not codes[0].any()                        # 0 / 0 = NaN -> code 0
    assert len(set(x[1].tolist())) == 1 and set(codes[1].tolist()) == {15}  # all equal: every v = 1
    assert x[2].max() == float(torch.finfo(torch.bfloat16).max)
    assert np.all((GOLDEN["planted_x"].reshape(24, 64)[3] & 0x7F80) == 0)   # subnormals (and zeros) only
    assert x[4].max() == 1.5 and x[4].min() == -1.5
    assert (GOLDEN["planted_w"].reshape(24, 64)[2] & 0x7FFF).min() > 0x7F80  # the largest bf16: factor 0, scaler NaN
    a = R.bf16.from_bits(GOLDEN["exact_absmax"]).astype(np.float64) * 256
    assert np.all(a == np.round(a)) and a.max() <= 256 and a.min() >= 1      # the exact-mean case
    assert float(R.bf16.from_bits(GOLDEN["exact_mean"])[0]) == float(R.bf16.bf16_round(np.array([a.sum() / 256 / len(a)], dtype=np.float32))[0])
    rows, cols, B, SB = meta("straddle")
    assert cols % B != 0                                                    # blocks straddle rows


@pytest.mark.parametrize("c", LINEAR_CASES)
def test_ref_linear_and_grad_input_reproduce_the_recorded_bytes(c):
    """The recorded forward and grad_input are the reference's CPU sums over the recorded dequantized weight: the restated weight's
    float64 sums rounded once give them byte for byte (all 14365 recorded values), and so lie inside _parity.bound."""
    import _parity

    rows, cols, B, SB = meta(c)
    w = R.weight(GOLDEN[f"{c}_codes"], GOLDEN[f"{c}_scalers"], GOLDEN[f"{c}_factors"], GOLDEN[f"{c}_mean"], B, SB, (rows, cols))
    x, go = bf(f"{c}_in", (5, cols)), bf(f"{c}_go", (5, rows))
    for got, a, b, K in ((bf(f"{c}_y", (5, rows)), x, w, cols), (bf(f"{c}_gi", (5, cols)), go, w.t().contiguous(), rows)):
        m64, S = R.sums(a, b)
        assert torch.equal(R.bits(R.linear(a, b)), R.bits(got))
        assert bool(((got.double() - m64).abs() <= _parity.bound(m64, S, K, torch.bfloat16)).all())


def test_code_rule_over_every_bf16_pattern():
    v = R.bf16.from_bits(np.arange(65536, dtype=np.uint16))
    assert np.array_equal(R.codes_of(v), GOLDEN["code_table"])
    assert GOLDEN["code_table"][0x7FC0] == 0 and GOLDEN["code_table"][0x3F80] == 15 and GOLDEN["code_table"][0] == 7
    assert NF4_TABLE == R.TABLE and R.table_is_on_the_2_pow_minus_11_grid()


# ---- 2. the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_new_symbols():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW:
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    assert [len(_lib._SIGNATURES[n]) for n in NEW] == [5, 10, 9, 12, 7, 5, 1]
    for name in NEW_OPS:
        assert name in ops.__all__ and callable(getattr(ops, name))
        if name in ("nf4_block_absmax", "nf4_quantize", "nf4_dequantize", "nf4_linear"):
            import ao_amd.torch_ops  # noqa: F401

            assert hasattr(torch.ops.ao_mi355, name)
    from ao_amd import prototype, quantization

    assert all(hasattr(quantization, n) for n in ("NF4Tensor", "to_nf4", "LinearNF4", "linear_nf4"))
    assert prototype.NF4WeightOnlyConfig is NF4WeightOnlyConfig and nf4_weight_only is NF4WeightOnlyConfig
    assert [(f.name, f.default) for f in dataclasses.fields(NF4WeightOnlyConfig)] == [("block_size", 64), ("scaler_block_size", 256)]


def test_argument_checks_without_a_gpu():
    lib = _lib.lib()
    one = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    bad = _lib.AO_ERR_INVALID_ARGUMENT
    assert lib.ao_nf4_block_absmax(one, one, 4096, 48, None) == bad and "block_size" in _lib.last_error()
    assert lib.ao_nf4_block_absmax(one, one, 4100, 64, None) == bad
    assert lib.ao_nf4_quantize(one, one, one, one, one, one, 4096, 64, 3, None) == bad and "power of two" in _lib.last_error()
    assert lib.ao_nf4_quantize(one, one, one, one, one, one, 4096, 64, 128, None) == bad      # 4096 % (64 x 128) != 0
    assert lib.ao_nf4_quantize(one, one, one, one, one, one, 1 << 31, 64, 1, None) == bad     # 32-bit element counts
    assert lib.ao_nf4_dequantize(one, one, one, one, one, 4096, 16, 1, None) == bad
    assert lib.ao_nf4_linear(one, one, one, one, one, one, 4, 512, 96, 64, 256, None) == bad  # K % block_size != 0
    assert lib.ao_nf4_linear(one, one, one, one, one, one, 4, 17, 64, 64, 2, None) == bad     # N K % (B x SB) != 0
    assert lib.ao_nf4_linear(one, one, one, one, one, one, -1, 64, 64, 64, 1, None) == bad
    assert lib.ao_nf4_linear(one, None, one, one, one, one, 4, 64, 64, 64, 1, None) == _lib.AO_ERR_NULL_POINTER
    assert lib.ao_nf4_linear(ctypes.c_void_p(4098), one, one, one, one, one, 4, 64, 64, 64, 1, None) == bad and "aligned" in _lib.last_error()
    assert lib.ao_nf4_linear(None, one, one, one, one, None, 0, 64, 64, 64, 1, None) == 0     # M = 0: nothing to launch
    assert lib.ao_nf4_block_absmax(None, None, 0, 64, None) == 0
    assert lib.ao_nf4_linear_set_form(2) == bad and "no tiled form" in _lib.last_error()
    assert lib.ao_nf4_linear_route(1, 64, 64, 64, 1, None, 7) == _lib.AO_ERR_NULL_POINTER
    out = (ctypes.c_int32 * 7)()
    assert lib.ao_nf4_linear_route(1, 64, 64, 64, 1, out, 6) == bad


# ---- 3. refusals, each with its reason, before the library is touched ------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def touched():
        raise AssertionError("the library was touched before the refusal")

    monkeypatch.setattr(_lib, "lib", touched)


def test_python_refusals_come_before_the_library(no_library):
    w = torch.zeros(64, 256, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="takes bfloat16 weights, got torch.float32"):
        to_nf4(w.float())
    with pytest.raises(NotImplementedError, match="takes bfloat16 weights, got torch.float16"):
        to_nf4(w.half())
    with pytest.raises(NotImplementedError, match="dim <= 2 but got dim = 3"):
        to_nf4(w.reshape(4, 16, 256))
    with pytest.raises(ValueError, match="block_size must be one of 32, 64, 128, got 16"):
        to_nf4(w, 16, 8)
    with pytest.raises(ValueError, match="scaler_block_size must be a power of two >= 1, got 24"):
        to_nf4(w, 64, 24)
    with pytest.raises(ValueError, match="scaler_block_size must be a power of two >= 1, got 0"):
        to_nf4(w, 64, 0)
    with pytest.raises(ValueError, match=r"numel=16384 must be a multiple of block_size x scaler_block_size = 64 x 512"):
        to_nf4(w, 64, 512)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        to_nf4(w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quantize_(torch.nn.Linear(256, 64, bias=False, dtype=torch.bfloat16), NF4WeightOnlyConfig())
    codes, q, qf, mean = (torch.zeros(8192, dtype=torch.uint8), torch.zeros(256, dtype=torch.int8), torch.ones(1, dtype=torch.bfloat16),
                          torch.zeros((), dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="absmax must be bfloat16"):
        ops.nf4_quantize(w, torch.zeros(256), mean)
    with pytest.raises(RuntimeError, match=r"absmax must be \[numel / block_size\]"):
        ops.nf4_quantize(w, torch.zeros(255, dtype=torch.bfloat16), mean)
    with pytest.raises(RuntimeError, match="codes must be a 1-D uint8"):
        ops.nf4_dequantize(codes.view(64, 128), q, qf, mean)
    with pytest.raises(RuntimeError, match="scalers must be int8"):
        ops.nf4_dequantize(codes, q.to(torch.uint8), qf, mean)
    with pytest.raises(RuntimeError, match="factors must be bfloat16"):
        ops.nf4_dequantize(codes, q, qf.float(), mean)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nf4_dequantize(codes, q, qf, mean)
    x = torch.zeros(3, 256, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="x must be a 2-D bfloat16 tensor"):
        ops.nf4_linear(x.float(), codes, q, qf, mean, 64, 256)
    with pytest.raises(RuntimeError, match=r"weight shape \[64, 128\] does not hold"):
        ops.nf4_linear(x, codes, q, qf, mean, 64, 128)
    with pytest.raises(RuntimeError, match="K mismatch 256 vs 128"):
        ops.nf4_linear(x, codes, q, qf, mean, 128, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nf4_linear(x, codes, q, qf, mean, 64, 256)


def _host_tensor(rows=64, cols=256, B=64, SB=256):
    """an NF4Tensor built by hand on the CPU (storage only: nothing here runs a kernel)"""
    n = rows * cols
    m = SubclassTensorArgs(torch.Size((rows, cols)), (cols, 1), 0, torch.bfloat16, torch.device("cpu"), False)
    return NF4Tensor(m, B, n // B, SB, torch.zeros(n // B, dtype=torch.int8), torch.ones(n // (B * SB), dtype=torch.bfloat16),
                     torch.zeros((), dtype=torch.bfloat16), torch.zeros(n // 2, dtype=torch.uint8), torch.tensor(NF4_TABLE, dtype=torch.bfloat16))


def test_unsupported_aten_ops_are_refused_by_name(no_library):
    t = _host_tensor()
    for call, name in ((lambda: t.split(32), "aten.split"), (lambda: t[:32], "aten.slice"), (lambda: t.view(-1), "aten.view"),
                       (lambda: t.as_strided((64, 256), (256, 1)), "aten.as_strided"), (lambda: t.new_zeros((64, 256)), "aten.new_zeros"),
                       (lambda: torch.cat([t, t]), "aten.cat"), (lambda: t.pin_memory(), "aten.is_pinned|aten._pin_memory"),
                       (lambda: t.narrow(0, 0, 64), "aten.narrow|aten.slice"), (lambda: t.view_as(t), "aten.view"),
                       (lambda: t + 1, "aten.add"), (lambda: t.sum(), "aten.sum")):
        with pytest.raises(NotImplementedError, match=f"NF4Tensor dispatch: attempting to run ({name})"):
            call()
    with pytest.raises(NotImplementedError, match="aten.copy_"):
        t.copy_(_host_tensor(SB=128))
    with pytest.raises(NotImplementedError, match="aten.mm"):
        torch.mm(torch.zeros(2, 64, dtype=torch.bfloat16), t)
    with pytest.raises(NotImplementedError, match="takes bfloat16 activations"):
        linear_nf4(torch.zeros(2, 256), t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.to(torch.bfloat16)


def test_storage_ops_need_no_kernel(no_library):
    t = _host_tensor()
    names, ctx = t.__tensor_flatten__()
    assert names == ["quantized_data", "scaler_mean", "quantization_factor", "quantized_scalers", "nf4"]
    assert (ctx["block_size"], ctx["n_blocks"], ctx["scaler_block_size"]) == (64, 256, 256)
    u = NF4Tensor.__tensor_unflatten__({n: getattr(t, n) for n in names}, ctx, t.shape, t.stride())
    assert type(u) is NF4Tensor and u.shape == t.shape and u.quantized_data is t.quantized_data
    d, c, tt = t.detach(), t.clone(), t.t()
    assert d.quantized_data.data_ptr() == t.quantized_data.data_ptr() and c.quantized_data.data_ptr() != t.quantized_data.data_ptr()
    assert tuple(tt.shape) == (256, 64) and tt.stride() == (1, 256) and tuple(tt.t().shape) == (64, 256) and tt.t().is_contiguous()
    t.quantized_scalers.fill_(3)
    assert c.copy_(t) is c and int(c.quantized_scalers[5]) == 3
    p = torch.nn.Parameter(t, requires_grad=False)
    assert isinstance(p, NF4Tensor) and not p.requires_grad
    assert isinstance(t.cpu(), NF4Tensor) and t.to("cpu").block_size == 64
    assert LinearNF4.apply is not None and "NF4Tensor" in repr(t)


# ---- 4. the route -----------------------------------------------------------------------------------------------------------------------------
def test_committed_cases_are_the_derivation():
    lib = _lib.lib()
    assert nc.CASES == nc.derive_cases(lib), "python tests/nf4_cases.py prints the list to commit"
    with nc.forced_stream(lib):
        sigs = {nc.signature(lib, c) for c in nc.CASES}
        props = set().union(*(nc.properties(lib, c) for c in nc.CASES))
    # every (waves, m-tiles) pair the plan produces below the widest grid, and every one the discovery grid reaches but for the 4-wave
    # plan of N >= 16369 (1024 column tiles: outside a quick test; its kernels are the 4-wave ones K = 512 reaches here)
    assert sigs == {("stream", w, mt) for w in (1, 2, 4, 8, 16) for mt in (1, 2, 4) if (w, mt) != (16, 4)}
    assert {(w, mt) for _, w, mt in nc.reachable(lib)} <= {(w, mt) for _, w, mt in sigs}
    assert props == set(nc.REQUIREMENTS)
    for M, N, K, B, SB in nc.CASES:
        assert K % B == 0 and (N * K) % (B * SB) == 0 and K <= 4096


def test_route_seam_forced_form_and_shapes_the_kernel_does_not_take():
    fused = [ops.nf4_linear_route(m, 4096, 4096)["kernel"] == "nf4_stream_kernel" for m in range(0, 300)]
    seam = max([m for m, f in enumerate(fused) if f], default=-1)
    assert all(fused[:seam + 1]) and not any(fused[seam + 1:]), "one seam: fused up to it, not fused beyond"
    for n, k in ((6144, 4096), (4096, 14336), (28672, 4096)):
        assert [ops.nf4_linear_route(m, n, k)["kernel"] == "nf4_stream_kernel" for m in range(0, 300)] == fused
    above = ops.nf4_linear_route(seam + 1, 4096, 4096)
    assert above == {"kernel": "not fused", "waves": 0, "m_tiles": 0, "tile_m": 0, "tile_n": 0, "grid": (0, 0)}
    assert ops.nf4_linear_kernel_name(seam + 1, 4096, 4096) == "not fused"
    # blocks that straddle rows, a format the tensor cannot have, more rows than the grid has
    assert ops.nf4_linear_route(1, 512, 96)["kernel"] == "not fused"
    assert ops.nf4_linear_route(1, 64, 256, 48, 1)["kernel"] == "not fused" and ops.nf4_linear_route(1, 64, 256, 64, 3)["kernel"] == "not fused"
    assert ops.nf4_linear_route(1, 17, 64, 64, 2)["kernel"] == "not fused"
    ops.nf4_set_form(1)
    try:
        r = ops.nf4_linear_route(4096, 4096, 4096)
        assert r == {"kernel": "nf4_stream_kernel", "waves": 8, "m_tiles": 4, "tile_m": 64, "tile_n": 16, "grid": (256, 64)}
        assert ops.nf4_linear_kernel_name(4096, 4096, 4096) == "nf4_stream_kernel"
        assert ops.nf4_linear_route(1, 512, 96)["kernel"] == "not fused"          # forcing does not make the kernel take a shape
        assert ops.nf4_linear_route(65536 * 64, 16, 32, 32, 1)["kernel"] == "not fused"
    finally:
        ops.nf4_set_form(0)
    with pytest.raises(ValueError, match="no tiled form"):
        ops.nf4_set_form(2)
    assert ops.nf4_linear_route(1, 4096, 4096)["kernel"] in ("nf4_stream_kernel", "not fused")
