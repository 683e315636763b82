"""NVFP4 training, the parts that need no GPU: the restated arithmetic (tests/nvfp4_train_ref.py) against the reference's recorded bytes
(tests/golden/nvfp4_training.npz), the stochastic-rounding contract on the restatement, the config, the module and their refusals, and the
C ABI's argument checks."""
import ctypes
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

import nvfp4_ref as R
import nvfp4_train_ref as T
from ao_amd import _lib, ops
from ao_amd.prototype import DEFAULT_SIGN_VECTOR, NVFP4Linear, NVFP4TrainingConfig, get_wgrad_sign_vector, nvfp4_linear
from ao_amd.quantization import quant_api, quantize_
from ao_amd.quantization.config import KernelPreference

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "nvfp4_training.npz"))
NEW = ["ao_nvfp4_train_amax", "ao_nvfp4_train_quantize_row_col", "ao_nvfp4_train_quantize_weight_2d", "ao_nvfp4_scaled_mm"]
MATRICES = ["act", "edge", "zero"]


def bf(name):
    return torch.from_numpy(GOLDEN[name].view(np.int16).copy()).view(torch.bfloat16)


def u8(name):
    return torch.from_numpy(GOLDEN[name].copy())


# ---- the restatement equals the fixture byte for byte ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATRICES)
def test_ref_amaxes_reproduce_the_reference_bits(name):
    got = T.amaxes(bf(f"{name}_x"))
    assert torch.equal(got.view(torch.int32), torch.from_numpy(GOLDEN[f"{name}_amax2"].copy()).view(torch.int32))


@pytest.mark.parametrize("name", MATRICES)
def test_ref_row_col_cast_reproduces_the_reference_bytes(name):
    cq, cs, rq, rs = T.quantize_row_col(bf(f"{name}_x"), torch.from_numpy(GOLDEN[f"{name}_amax2"].copy()))
    for tag, got in (("col_q", cq), ("col_s", cs), ("row_q", rq), ("row_s", rs)):
        assert torch.equal(got, u8(f"{name}_{tag}")), tag


@pytest.mark.parametrize("name", MATRICES + ["w"])
def test_ref_weight_2d_cast_reproduces_the_reference_bytes(name):
    q, s, qt, st = T.quantize_weight_2d(bf(f"{name}_x"), torch.from_numpy(GOLDEN[f"{name}_amax"].copy()))
    for tag, got in (("w2d_q", q), ("w2d_s", s), ("w2dt_q", qt), ("w2dt_s", st)):
        assert torch.equal(got, u8(f"{name}_{tag}")), tag
    # one set of block scales, the codes of the same values
    assert torch.equal(R.unpack(q).t(), R.unpack(qt)) and torch.equal(s[::16].t(), st[::16])


def test_fixture_holds_the_edge_blocks_it_names():
    s = GOLDEN["edge_row_s"].reshape(-1)[::16].tolist()   # one scale byte a block (a run of 16 rows holds one block)
    q = GOLDEN["edge_row_q"][::16]
    assert float(GOLDEN["edge_amax2"][1]) == 42.0
    assert s[0] == 0 and s[1] == 0                         # zero and -0.0 blocks: NO lower clamp
    assert q[0].tolist() == [0x88] * 8 and GOLDEN["edge_row_q"][1].tolist() == [0] * 8   # row 0 is the zero block negated: -0.0 keeps its sign
    assert s[2] == 0x68                                    # amax 6 under S_enc = 64: scale 64 exactly, enc = 1
    assert q[2].tolist() == [0x08, 0x2A, 0x2A, 0x4C, 0x4C, 0x6E, 0x6E, 0x7F]  # every tie to the even code, both signs (row 0 is negated)
    assert GOLDEN["edge_row_q"][33].tolist() == [0x80, 0xA2, 0xA2, 0xC4, 0xC4, 0xE6, 0xE6, 0xF7]
    assert s[5:11] == [0x38, 0x38, 0x39, 0x39, 0x3A, 0x3A]  # below / at (to even) / above the ties 1.0625 and 1.1875
    assert s[11:14] == [1, 2, 2] and s[14:17] == [0, 0, 1]  # the subnormal tie 1.5 x 2^-9 and the underflow point 2^-10 (to even: 0)
    assert s[17] == 0x7E and s[19] == 0                    # the tensor's amax saturates at 448; 2^-20 underflows to byte 0
    assert GOLDEN["edge_row_q"][19 * 16 + 1].tolist() == [0x77, 0x7F, 0x7F, 0x7F, 0x80, 0xF7, 0xF7, 0x77]  # ... under enc = FLT_MAX: +-6 or a signed 0
    assert not GOLDEN["zero_row_q"].any() and not GOLDEN["zero_col_s"].any() and float(GOLDEN["zero_amax2"].max()) == 0.0


# ---- stochastic rounding on the restatement ---------------------------------------------------------------------------------------------------
def _sr_input():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(32, 64, generator=g) * 2).to(torch.bfloat16)
    x[0, :16] = torch.tensor(T.E2M1_GRID + [-v for v in T.E2M1_GRID])  # a block of grid values, amax 6 ...
    x[1, 0] = 42.0                                                      # ... under S_enc = 2688 / 42 = 64: block scale 64, enc = 1
    return x, x.float().abs().max()


def _scaled(x, amax):
    v = x.float()
    s8, enc = T.encode(v.abs().reshape(32, 4, 16).amax(dim=-1), amax)
    return torch.clamp(v * enc.repeat_interleave(16, dim=1), -6.0, 6.0), s8


def test_sr_codes_are_grid_neighbours_and_grid_values_never_move():
    x, amax = _sr_input()
    scaled, _ = _scaled(x, amax)
    grid = T._f32(T.E2M1_GRID)
    a = scaled.abs()
    lo = grid[(torch.searchsorted(grid, a.contiguous(), right=True) - 1).clamp(0, 7)]
    hi = grid[torch.searchsorted(grid, a.contiguous()).clamp(0, 7)]
    on_grid = lo == hi
    assert bool(on_grid[0, :16].all()) and torch.equal(scaled[0, :16], x[0, :16].float())
    for offset in (0, 1, 99):
        q, _ = T.cast(x, amax, sr=(1234, offset, 0))
        v = R.values(q)
        assert bool(((v.abs() == lo) | (v.abs() == hi)).all())
        assert torch.equal(v[on_grid], scaled[on_grid])
        assert bool((torch.signbit(v) == torch.signbit(scaled)).all())
        rt, _ = T.cast(x, amax)
        assert torch.equal(R.unpack(q)[on_grid], R.unpack(rt)[on_grid])


def test_sr_bytes_depend_on_seed_offset_and_stream_only():
    x, amax = _sr_input()
    a = T.cast(x, amax, sr=(-77, 5, 0))[0]
    assert torch.equal(a, T.cast(x, amax, sr=(-77, 5, 0))[0])
    assert torch.equal(a, T.cast(x, amax, sr=(-77, 5 + 2 ** 32, 0))[0])  # the low 32 bits of the offset
    for other in ((-77, 6, 0), (-77, 5, 1), (-76, 5, 0), (-77 + 2 ** 32, 5, 0)):
        assert not torch.equal(a, T.cast(x, amax, sr=other)[0]), other
    # the published known-answer vectors of Philox4x32-10 (Random123 kat_vectors)
    assert [int(w) for w in T.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(w) for w in T.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)] == [
        0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert [int(w) for w in T.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)] == [
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_sr_is_unbiased_within_five_sigma():
    """The mean of n dequantized draws is within 5 sigma of the scaled input: one draw of an element between lo and hi is lo + step
    Bernoulli(p), so its variance is step^2 p (1 - p) <= step^2 / 4, and the mean of n independent draws has sigma <= step / (2 sqrt(n));
    the rule's own bias, below 2^-16 of a step, is added to the allowance.  A condition, not a measurement: n and the steps are the test's."""
    x, amax = _sr_input()
    scaled, _ = _scaled(x, amax)
    grid = T._f32(T.E2M1_GRID)
    a = scaled.abs()
    lo_c = (torch.searchsorted(grid, a.contiguous(), right=True) - 1).clamp(0, 7)
    step = grid[(lo_c + 1).clamp(max=7)] - grid[lo_c]
    n = 256
    total = torch.zeros_like(scaled, dtype=torch.float64)
    for offset in range(n):
        total += R.values(T.cast(x, amax, sr=(2024, offset, 0))[0]).double()
    err = (total / n - scaled.double()).abs()
    allowed = 5.0 * step.double() / (2.0 * math.sqrt(n)) + step.double() * 2.0 ** -16
    assert bool((err <= allowed).all()), f"worst {float((err / allowed.clamp(min=1e-30)).max()):.2f} x the allowance"
    # and the whole tensor's mean error is centred: |mean of err / step| within 5 sigma of a mean over numel independent elements
    live = step > 0
    z = ((total / n - scaled.double())[live] / step.double()[live]).mean().abs()
    assert float(z) <= 5.0 / (2.0 * math.sqrt(n * int(live.sum()))) + 2.0 ** -16


# ---- the config, the module, the refusals -----------------------------------------------------------------------------------------------------
def test_config_defaults_and_registration():
    c = NVFP4TrainingConfig()
    assert (c.kernel_preference, c.process_group, c.world_size, c.rht_sign_vector) == (KernelPreference.AUTO, None, None, None)
    assert [f.name for f in dataclasses.fields(c)] == ["kernel_preference", "process_group", "world_size", "rht_sign_vector"]
    assert NVFP4TrainingConfig in quant_api._QUANTIZE_CONFIG_HANDLER
    assert DEFAULT_SIGN_VECTOR == T.DEFAULT_SIGN_VECTOR and len(DEFAULT_SIGN_VECTOR) == 16
    v = get_wgrad_sign_vector(16, device="cpu", dtype=torch.int8)
    assert v.dtype == torch.int8 and set(v.tolist()) <= {1, -1}
    assert ops.nvfp4_sign_mask(DEFAULT_SIGN_VECTOR) == sum(1 << i for i, s in enumerate(DEFAULT_SIGN_VECTOR) if s < 0)
    for k in (KernelPreference.AUTO, KernelPreference.TORCH, KernelPreference.TRITON):
        assert NVFP4TrainingConfig(kernel_preference=k).kernel_preference is k


def test_refusals_name_the_cause():
    with pytest.raises(ValueError, match="tensor-parallel"):
        NVFP4TrainingConfig(process_group=object())
    with pytest.raises(ValueError, match="tensor-parallel"):
        NVFP4TrainingConfig(world_size=2)
    with pytest.raises(ValueError, match="tensor-parallel"):
        NVFP4Linear(32, 32, world_size=2)
    for k in (KernelPreference.MSLK, KernelPreference.EMULATED, "cutedsl"):
        with pytest.raises(ValueError, match="AUTO, TORCH or TRITON"):
            NVFP4TrainingConfig(kernel_preference=k)
    for bad in ((1,) * 15, (1,) * 15 + (0,), (1,) * 17, torch.ones(8), 3):
        with pytest.raises(ValueError, match="16 values of \\+1 or -1"):
            NVFP4TrainingConfig(rht_sign_vector=bad)
        with pytest.raises(ValueError, match="16 values of \\+1 or -1"):
            nvfp4_linear(torch.zeros(16, 32, dtype=torch.bfloat16), torch.zeros(16, 32, dtype=torch.bfloat16), sign_vector=bad)
    with pytest.raises(ValueError, match="AUTO, TORCH or TRITON"):
        nvfp4_linear(torch.zeros(16, 32), torch.zeros(16, 32), sign_vector=DEFAULT_SIGN_VECTOR, kernel_preference=KernelPreference.DEEPGEMM)


@pytest.mark.parametrize("m,k,n", [(8, 32, 32), (16, 40, 32), (16, 32, 24), (144, 80, 40)])
def test_shape_errors_raise_before_the_library_is_touched(m, k, n, monkeypatch):
    def touched(*a, **kw):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "lib", touched)
    lin = NVFP4Linear(k, n, rht_sign_vector=DEFAULT_SIGN_VECTOR, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=f"multiples of 16.*M={m}, N={n}, K={k}"):
        lin(torch.zeros(m, k, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="not compatible"):
        nvfp4_linear(torch.zeros(16, 48), torch.zeros(16, 32), sign_vector=DEFAULT_SIGN_VECTOR)


def test_module_buffers_state_dict_and_quantize():
    sv = tuple(-s for s in DEFAULT_SIGN_VECTOR)
    lin = NVFP4Linear(32, 48, bias=True, rht_sign_vector=sv)
    assert lin.rht_sign_vector == sv and lin._rht_sign_vector.dtype == torch.int8 and lin._sr_seed.dtype == torch.int64
    assert {"weight", "bias", "_sr_seed", "_rht_sign_vector"} <= set(lin.state_dict())
    other = NVFP4Linear(32, 48, bias=True)
    other.load_state_dict(lin.state_dict())
    assert other.rht_sign_vector == sv and int(other._sr_seed) == int(lin._sr_seed)   # refreshed after the load
    model = torch.nn.Sequential(torch.nn.Linear(32, 48), torch.nn.ReLU(), torch.nn.Linear(48, 16, bias=False))
    w0 = model[0].weight
    quantize_(model, NVFP4TrainingConfig(rht_sign_vector=sv, kernel_preference="triton"))
    assert type(model[0]) is NVFP4Linear and type(model[2]) is NVFP4Linear and type(model[1]) is torch.nn.ReLU
    assert model[0].weight is w0 and model[0].bias is not None and model[2].bias is None
    assert model[0].rht_sign_vector == sv and model[2].rht_sign_vector == sv and model[0].kernel_preference is KernelPreference.TRITON
    quantize_(model, NVFP4TrainingConfig())  # already swapped: left as they are
    assert model[0].rht_sign_vector == sv
    drawn = NVFP4Linear.from_linear(torch.nn.Linear(16, 16))
    assert set(drawn.rht_sign_vector) <= {1, -1} and len(drawn.rht_sign_vector) == 16


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_new_symbols():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW:
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    for name in ("nvfp4_train_amax", "nvfp4_train_quantize_row_col", "nvfp4_train_quantize_weight_2d", "nvfp4_scaled_mm", "nvfp4_sign_mask"):
        assert name in ops.__all__ and callable(getattr(ops, name))


def test_argument_checks_without_a_gpu():
    lib = _lib.lib()
    one = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    INV, NUL, OK = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_ERR_NULL_POINTER, _lib.AO_OK
    assert lib.ao_nvfp4_train_amax(one, one, 24, 32, 0, 1, None) == INV and "multiples of 16" in _lib.last_error()
    assert lib.ao_nvfp4_train_amax(one, one, 32, 40, 0, 1, None) == INV
    assert lib.ao_nvfp4_train_amax(one, one, 32, 32, 1 << 16, 1, None) == INV and "16-bit mask" in _lib.last_error()
    assert lib.ao_nvfp4_train_amax(one, None, 32, 32, 0, 1, None) == NUL
    assert lib.ao_nvfp4_train_amax(None, one, 32, 32, 0, 1, None) == NUL
    q = lib.ao_nvfp4_train_quantize_row_col
    assert q(one, one, 0, None, None, None, one, one, one, one, 32, 24, None) == INV
    assert q(one, one, 0, None, None, None, None, None, None, None, 32, 32, None) == INV and "both outputs are null" in _lib.last_error()
    assert q(one, one, 0, None, None, None, one, None, one, one, 32, 32, None) == INV and "together" in _lib.last_error()
    assert q(one, None, 0, None, None, None, one, one, one, one, 32, 32, None) == NUL
    assert q(None, one, 0, None, None, None, one, one, one, one, 32, 32, None) == NUL
    assert q(one, one, 0, one, None, one, one, one, one, one, 32, 32, None) == NUL      # SR of the column output without its offset
    assert q(one, one, 0, one, one, None, one, one, one, one, 32, 32, None) == NUL
    assert q(one, one, 0, None, None, None, ctypes.c_void_p(4100), one, one, one, 32, 32, None) == INV and "aligned" in _lib.last_error()
    assert q(None, one, 0, None, None, None, one, one, one, one, 0, 32, None) == OK     # M = 0: nothing launched
    w = lib.ao_nvfp4_train_quantize_weight_2d
    assert w(one, one, one, one, one, one, 40, 32, None) == INV
    assert w(one, one, one, one, None, one, 32, 32, None) == NUL
    assert w(one, None, one, one, one, one, 32, 32, None) == NUL
    mm = lib.ao_nvfp4_scaled_mm
    assert mm(one, one, one, one, one, one, one, 4, 32, 24, None) == INV and "multiple of 16" in _lib.last_error()
    assert mm(one, one, None, one, one, one, one, 4, 32, 32, None) == NUL               # both per-tensor scales are required
    assert mm(one, one, one, one, one, None, one, 4, 32, 32, None) == NUL
    assert mm(one, one, one, one, one, one, None, 4, 32, 32, None) == NUL
    assert mm(None, None, one, one, one, one, None, 0, 32, 32, None) == OK
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nvfp4_train_amax(torch.zeros(16, 32, dtype=torch.bfloat16), DEFAULT_SIGN_VECTOR)
    with pytest.raises(ValueError, match="16 values"):
        ops.nvfp4_sign_mask((1, -1))
