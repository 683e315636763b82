"""Low-bit optimizers on the host: the tables, the numpy restatement against the reference's recording (tests/golden/optim.npz), the
optimizer classes' argument checks, state creation and state dicts, slicing, the C entries, and the stochastic-rounding contract's statistics."""
import json
import math
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from ao_amd import _lib, ops
from ao_amd import optim as O
from ao_amd.optim import quant_utils as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim.npz")


@pytest.fixture(scope="module")
def g():
    return R.load_golden(GOLDEN)


def qmaps_of(g):
    return {k: g[f"qmap_{k}"] for k in ("q8s", "q8u", "q4s", "q4u")}


def cases(g=None):
    return json.loads(str((g if g is not None else np.load(GOLDEN))["cases"]))


CASE_NAMES = [c["name"] for c in cases()]
QUANT_NAMES = [c["name"] for c in json.loads(str(np.load(GOLDEN)["quant_cases"]))]


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["q8s", "q8u", "q4s", "q4u"])
def test_the_tables_are_the_recorded_ones_bit_for_bit(g, kind):
    mine = Q.make_qmap(int(kind[1]), kind[2] == "s").numpy()
    assert mine.dtype == np.float32 and np.array_equal(mine.view(np.uint32), g[f"qmap_{kind}"].view(np.uint32))
    assert np.all(np.diff(mine) > 0) and mine[-1] == 1.0


def test_the_unsigned_4_bit_table_has_no_zero(g):
    assert g["qmap_q4u"][0] == np.float32(1.0 / 16.0)


# ---- the restatement reproduces the fixture -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_reproduces_the_recorded_steps(g, name):
    c = next(c for c in cases(g) if c["name"] == name)
    n = math.prod(c["shape"])
    assert c["quantized"] == (c["family"] != "plain" and n >= 4096 and n % c["block_size"] == 0)
    states = R.new_states(c["family"] if c["quantized"] else "plain", n, c["block_size"], qmaps_of(g), c["bf16"], c["amsgrad"])
    p = g[f"{name}_p0"]
    for t in range(1, c["steps"] + 1):
        p = R.adam_step(p, g[f"{name}_g{t}"], states, dict(zip(R.SCALAR_NAMES, g[f"{name}_scalars{t}"])), c["adamw"], c["bf16"])
        assert np.array_equal(p, g[f"{name}_p{t}"]), (name, t)
        for k, s in enumerate(states):
            for field, v in s.fields().items():
                assert np.array_equal(v, g[f"{name}_s{k}_{field}{t}"]), (name, t, k, field)


@pytest.mark.parametrize("name", QUANT_NAMES)
def test_restatement_reproduces_the_recorded_quantizers(g, name):
    c = next(c for c in json.loads(str(g["quant_cases"])) if c["name"] == name)
    qmap = qmaps_of(g).get(c["kind"])
    codes, scale = R.quantize(c["kind"], g[f"{name}_x"], c["block_size"], qmap)
    assert np.array_equal(codes, g[f"{name}_codes"]) and np.array_equal(scale, g[f"{name}_scale"])
    assert np.array_equal(R.dequantize(c["kind"], codes, scale, c["block_size"], qmap).view(np.uint32), g[f"{name}_deq"].view(np.uint32))
    every = R.dequantize(c["kind"], g[f"{name}_all_codes"], g[f"{name}_all_scale"], c["all_block_size"], qmap)
    assert np.array_equal(every.view(np.uint32), g[f"{name}_all_deq"].view(np.uint32))


def test_the_recorded_scalars_are_what_step_scalars_computes(g):
    for c in cases(g):
        lr = torch.tensor(c["lr"], dtype=torch.float32)
        for t in range(1, c["steps"] + 1):
            got = np.array(O.step_scalars(lr, c["betas"][0], c["betas"][1], c["wd"], c["eps"], torch.tensor(float(t))), dtype=np.float32)
            assert np.array_equal(got.view(np.uint32), g[f"{c['name']}_scalars{t}"].view(np.uint32)), (c["name"], t)


def test_fma32_is_one_rounding():
    rng = np.random.RandomState(5)
    a, b, c = (rng.standard_normal(1 << 16).astype(np.float32) for _ in range(3))
    c = (c * np.float32(1e-3)).astype(np.float32)
    from fractions import Fraction
    got = R.fma32(a, b, c)
    for i in range(0, 1 << 16, 257):  # exact rational arithmetic on a sample
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    assert (R.lerp(a, b, 0.1) != R.lerp_unfused(a, b, 0.1)).sum() > 0
    assert np.array_equal(R.lerp(a, b, 0.25), R.lerp_unfused(a, b, 0.25))


# ---- the optimizer classes ------------------------------------------------------------------------------------------------------------------------
ALL = [O.Adam8bit, O.Adam4bit, O.AdamFp8, O.AdamW8bit, O.AdamW4bit, O.AdamWFp8, O._AdamW]


def test_signatures_and_defaults_are_the_references():
    p = [torch.nn.Parameter(torch.zeros(8))]
    for cls, bs, wd, adamw in ((O.Adam8bit, 256, 0, False), (O.Adam4bit, 128, 0, False), (O.AdamFp8, 256, 0, False), (O.AdamW8bit, 256, 1e-2, True),
                               (O.AdamW4bit, 128, 1e-2, True), (O.AdamWFp8, 256, 1e-2, True), (O._AdamW, None, 1e-2, True)):
        opt = cls(p)
        grp = opt.param_groups[0]
        assert opt.block_size == bs and grp["weight_decay"] == wd and opt.is_adamw is adamw and opt.bf16_stochastic_round is False
        assert grp["betas"] == (0.9, 0.999) and grp["eps"] == 1e-8 and grp["amsgrad"] is False
        assert isinstance(grp["lr"], torch.Tensor) and grp["lr"].dtype == torch.float32 and grp["lr"].device.type == "cpu"
        assert opt.sr_seed == torch.initial_seed() and "sr_seed" not in json.dumps(list(opt.state_dict()["param_groups"][0].keys()))
    assert O.AdamW8bit(p, sr_seed=7).sr_seed == 7


@pytest.mark.parametrize("cls", ALL)
def test_argument_validation(cls):
    p = [torch.nn.Parameter(torch.zeros(8))]
    with pytest.raises(ValueError, match="Invalid learning rate"):
        cls(p, lr=-1.0)
    with pytest.raises(ValueError, match="Invalid epsilon"):
        cls(p, eps=-1.0)
    with pytest.raises(ValueError, match="beta parameter at index 0"):
        cls(p, betas=(1.0, 0.9))
    with pytest.raises(ValueError, match="beta parameter at index 1"):
        cls(p, betas=(0.9, 1.0))
    if cls is not O._AdamW:
        with pytest.raises(ValueError, match="block_size must be a power of two from 64 to 2048"):
            cls(p, block_size=96)
        with pytest.raises(ValueError, match="block_size must be a power of two from 64 to 2048"):
            cls(p, block_size=4096)


def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match="float16 parameters are not supported"):
        O.AdamW8bit([torch.nn.Parameter(torch.zeros(8, dtype=torch.float16))])
    with pytest.raises(NotImplementedError, match="CPUOffloadOptimizer is not supported"):
        O.CPUOffloadOptimizer([], O.AdamW8bit)
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))
    opt = O.AdamW8bit([p])
    p.grad_dtype = None  # (torch itself keeps a gradient to its parameter's dtype unless told otherwise)
    p.grad = torch.zeros(8, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="gradient of dtype torch.float32 for a parameter of dtype torch.bfloat16"):
        opt.step()
    e = torch.nn.Embedding(4, 4, sparse=True)
    e(torch.tensor([1])).sum().backward()
    with pytest.raises(RuntimeError, match="Sparse gradient is not supported"):
        O.Adam8bit(e.parameters()).step()
    q = torch.nn.Parameter(torch.zeros(8))
    opt = O.AdamWFp8([q])
    opt.param_groups[0]["lr"] = 1e-3
    q.grad = torch.zeros(8)
    with pytest.raises(RuntimeError, match="lr was changed to a non-Tensor object"):
        opt.step()
    q.grad = torch.zeros(8)
    with pytest.raises(RuntimeError, match="optim_adam_step: expected all tensors on the GPU"):  # no CPU fallback
        O.AdamWFp8([q]).step()


def test_dtensor_parameters_are_refused_by_name():
    dt = pytest.importorskip("torch.distributed.tensor")

    class Fake(dt.DTensor):  # an instance check is all the refusal makes: no process group is needed to meet it
        @staticmethod
        def __new__(cls):
            return torch.Tensor._make_wrapper_subclass(cls, (8,), dtype=torch.float32, requires_grad=True)

        def __init__(self):
            pass

        __torch_function__ = torch._C._disabled_torch_function_impl

    with pytest.raises(NotImplementedError, match="DTensor / FSDP2 parameters are not supported"):
        O.AdamW8bit([Fake()])


@pytest.mark.parametrize("cls,state_cls", [(O.AdamW8bit, O.OptimState8bit), (O.Adam4bit, O.OptimState4bit), (O.AdamWFp8, O.OptimStateFp8)])
def test_the_state_creation_rule(cls, state_cls):
    opt = cls([torch.nn.Parameter(torch.zeros(8))])
    bs = opt.block_size
    for n, quantized in ((4096, True), (4095, False), (4096 + bs, True), (4097, False), (4096 - bs, False), (2 * bs, False)):
        p = torch.zeros(n, dtype=torch.bfloat16)
        assert opt._quantizes(p) is quantized
        buf = opt._new_buffer(p, True)
        if quantized:
            assert isinstance(buf, state_cls) and buf.block_size == bs and buf.dtype == torch.bfloat16 and tuple(buf.shape) == (n,)
            assert buf.scale.shape == (n // bs,) and buf.scale.dtype == torch.float32
        else:
            assert type(buf) is torch.Tensor and buf.dtype == torch.bfloat16 and buf.shape == p.shape
    p2 = torch.zeros(48, 96)
    buf = opt._new_buffer(p2, False)
    assert isinstance(buf, state_cls) and tuple(buf.shape) == (48, 96) and buf.dtype == torch.float32
    if state_cls is not O.OptimStateFp8:
        assert buf.signed is False and np.array_equal(buf.qmap.numpy(), Q.make_qmap(4 if state_cls is O.OptimState4bit else 8, False).numpy())
    if state_cls is O.OptimState4bit:
        assert buf.codes.shape == (48 * 96 // 2,) and buf._shape == (48, 96)
    assert type(O._AdamW([torch.nn.Parameter(torch.zeros(8))])._new_buffer(torch.zeros(8192), True)) is torch.Tensor


def _with_states(cls, n=4096, amsgrad=True):
    """an optimizer whose states were made the way step() makes them, filled with recognisable bytes (no kernel runs on the host)"""
    p = torch.nn.Parameter(torch.zeros(n, dtype=torch.bfloat16))
    small = torch.nn.Parameter(torch.zeros(7, dtype=torch.bfloat16))
    opt = cls([p, small], amsgrad=amsgrad)
    for q in (p, small):
        st = opt.state[q]
        st["step"] = torch.tensor(3.0)
        st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"] = opt._new_buffer(q, True), opt._new_buffer(q, False), opt._new_buffer(q, False)
    for i, k in enumerate(("exp_avg", "exp_avg_sq", "max_exp_avg_sq")):
        s = opt.state[p][k]
        if isinstance(s, torch.Tensor) and type(s) is not torch.Tensor:
            s.codes.view(torch.uint8).copy_((torch.arange(s.codes.numel()) * (i + 3) % 120).to(torch.uint8).view(s.codes.shape))
            s.scale.copy_(torch.arange(s.scale.numel()) + 0.5 + i)
    return opt, p, small


@pytest.mark.parametrize("cls", [O.AdamW8bit, O.AdamW4bit, O.AdamWFp8, O._AdamW])
def test_state_dict_round_trip(cls, tmp_path):
    opt, p, small = _with_states(cls)
    path = tmp_path / "opt.pt"
    torch.save(opt.state_dict(), path)
    sd = torch.load(path, weights_only=True)  # add_safe_globals: the subclasses unpickle under weights_only
    opt2 = cls([torch.nn.Parameter(torch.zeros(4096, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(7, dtype=torch.bfloat16))], amsgrad=True)
    opt2.load_state_dict(sd)
    for a, b in zip((p, small), opt2.param_groups[0]["params"]):
        sa, sb = opt.state[a], opt2.state[b]
        assert float(sb["step"]) == 3.0 and set(sa) == set(sb)
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert type(sa[k]) is type(sb[k]) and sb[k].dtype == torch.bfloat16
            if type(sa[k]) is torch.Tensor:
                assert torch.equal(sa[k], sb[k])
            else:
                assert torch.equal(sa[k].codes.view(torch.uint8), sb[k].codes.view(torch.uint8)) and torch.equal(sa[k].scale, sb[k].scale)
                assert sa[k].block_size == sb[k].block_size
                if hasattr(sa[k], "qmap"):
                    assert torch.equal(sa[k].qmap, sb[k].qmap) and sa[k].signed == sb[k].signed
    assert isinstance(opt2.param_groups[0]["lr"], torch.Tensor)


@pytest.mark.parametrize("name,cls,state_cls", [("q8_adamw_bf16", O.AdamW8bit, O.OptimState8bit), ("q4_adamw_bf16", O.AdamW4bit, O.OptimState4bit),
                                                ("fp8_adamw_bf16", O.AdamWFp8, O.OptimStateFp8)])
def test_a_state_dict_built_from_the_fixtures_fields_loads(g, name, cls, state_cls):
    """what the reference library writes: its subclasses' fields (codes, scale, qmap, signed[, shape]) -- here from its recorded step 2"""
    c = next(c for c in cases(g) if c["name"] == name)
    kinds = {"q8": ("q8s", "q8u"), "q4": ("q4s", "q4u"), "fp8": (None, None)}[c["family"]]
    states = {}
    for k, key in enumerate(("exp_avg", "exp_avg_sq")):
        codes, scale = torch.from_numpy(g[f"{name}_s{k}_codes2"].copy()), torch.from_numpy(g[f"{name}_s{k}_scale2"].copy())
        if state_cls is O.OptimStateFp8:
            states[key] = state_cls(codes.view(torch.float8_e4m3fn), scale, dtype=torch.bfloat16)
        elif state_cls is O.OptimState4bit:
            states[key] = state_cls(codes, scale, torch.from_numpy(g[f"qmap_{kinds[k]}"].copy()), k == 0, (4096,), dtype=torch.bfloat16)
        else:
            states[key] = state_cls(codes, scale, torch.from_numpy(g[f"qmap_{kinds[k]}"].copy()), k == 0, dtype=torch.bfloat16)
    p = torch.nn.Parameter(torch.zeros(4096, dtype=torch.bfloat16))
    opt = cls([p])
    sd = opt.state_dict()
    sd["state"] = {0: {"step": torch.tensor(2.0), **states}}
    opt.load_state_dict(sd)
    for k, key in enumerate(("exp_avg", "exp_avg_sq")):
        s = opt.state[p][key]
        assert isinstance(s, state_cls) and s.block_size == c["block_size"] and s.dtype == torch.bfloat16
        assert np.array_equal(s.codes.view(torch.uint8).numpy().reshape(-1), g[f"{name}_s{k}_codes2"]) and np.array_equal(s.scale.numpy(), g[f"{name}_s{k}_scale2"])


@pytest.mark.parametrize("state_cls", [O.OptimState8bit, O.OptimState4bit, O.OptimStateFp8])
def test_slice_at_and_off_block_boundaries(state_cls):
    bs = 128
    s = state_cls.zeros((64, 32), block_size=bs, dtype=torch.bfloat16) if state_cls is O.OptimStateFp8 else state_cls.zeros((64, 32), True, bs, dtype=torch.bfloat16)
    s.codes.view(torch.uint8).copy_((torch.arange(s.codes.numel()) % 251).to(torch.uint8).view(s.codes.shape))
    s.scale.copy_(torch.arange(16.0))
    part = s[8:24]  # rows of 32: four rows a block -- 8 and 24 sit on boundaries
    assert isinstance(part, state_cls) and tuple(part.shape) == (16, 32) and part.block_size == bs and part.dtype == torch.bfloat16
    assert torch.equal(part.scale, torch.arange(2.0, 6.0))
    per_row = 16 if state_cls is O.OptimState4bit else 32
    want = s.codes.view(torch.uint8).reshape(-1)[8 * per_row:24 * per_row]
    assert torch.equal(part.codes.view(torch.uint8).reshape(-1), want)
    for start, end in ((2, 24), (8, 22), (1, 3)):
        with pytest.raises(ValueError, match="align with block boundary"):
            s[start:end]
    with pytest.raises(ValueError, match="first dim"):
        s[:, 0:8]
    with pytest.raises(ValueError, match="step=1"):
        s[0:16:2]


@pytest.mark.parametrize("state_cls", [O.OptimState8bit, O.OptimState4bit, O.OptimStateFp8])
def test_structural_ops_rewrap_the_fields(state_cls):
    s = state_cls.zeros((32, 128), block_size=256, dtype=torch.bfloat16) if state_cls is O.OptimStateFp8 else state_cls.zeros((32, 128), False, 256, dtype=torch.bfloat16)
    f = s.float()
    assert isinstance(f, state_cls) and f.dtype == torch.float32 and f.codes.data_ptr() == s.codes.data_ptr()  # the appearance dtype only
    v = s.view(-1)
    assert isinstance(v, state_cls) and tuple(v.shape) == (4096,) and v.scale.data_ptr() == s.scale.data_ptr()
    d = s.detach()
    assert isinstance(d, state_cls) and d.codes.data_ptr() == s.codes.data_ptr() and d.dtype == torch.bfloat16
    other = state_cls.zeros((32, 128), block_size=256) if state_cls is O.OptimStateFp8 else state_cls.zeros((32, 128), False, 256)
    other.scale.fill_(2.0)
    s.copy_(other)  # state <- state: bytes
    assert torch.equal(s.scale, other.scale)
    with pytest.raises(RuntimeError, match="optim_quantize: expected all tensors on the GPU"):  # state <- float: the kernel, never an eager chain
        s.copy_(torch.zeros(32, 128))
    with pytest.raises(RuntimeError, match="optim_dequantize: expected all tensors on the GPU"):
        s.dequantize()


# ---- the C entries -----------------------------------------------------------------------------------------------------------------------------------
def test_c_entries_are_declared_and_resolved():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name, nargs in (("ao_optim_quantize", 9), ("ao_optim_dequantize", 9), ("ao_optim_adam_step", 23), ("ao_optim_grid", 3)):
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES and len(_lib._SIGNATURES[name]) == nargs
    assert [n for n, _ in _lib.OptimScalars._fields_] == list(ops.OPTIM_SCALARS)
    assert ops.OPTIM_FORMATS == {Q.FORMAT_NAMES[v]: v for v in Q.FORMAT_NAMES} and ops.OPTIM_BLOCK_SIZES == Q.BLOCK_SIZES


def test_the_grid_rule():
    r = ops.optim_grid(4096)
    tile = r["tile"]
    assert r == {"tile": tile, "tiles": 1, "workgroups": 1} and all(tile % b == 0 for b in ops.OPTIM_BLOCK_SIZES)
    assert ops.optim_grid(tile + 1) == {"tile": tile, "tiles": 2, "workgroups": 2}
    assert ops.optim_grid(7 * tile + 256, max_workgroups=3) == {"tile": tile, "tiles": 8, "workgroups": 3}
    big = ops.optim_grid(1 << 34)
    assert big["workgroups"] < big["tiles"]  # a capped grid: the loop takes further trips


def test_host_entries_refuse_bad_arguments_by_name():
    lib = _lib.lib()
    s = _lib.OptimScalars()
    import ctypes
    rc = lib.ao_optim_adam_step(None, None, 1, None, None, None, None, None, None, None, None, None, 0, 4096, 96, ctypes.byref(s), 1, 0, 0, 1, 0, 0, None)
    assert rc == _lib.AO_ERR_INVALID_ARGUMENT and "block_size must be a power of two from 64 to 2048" in _lib.last_error()
    rc = lib.ao_optim_adam_step(None, None, 1, None, None, None, None, None, None, None, None, None, 1, 4096, 256, ctypes.byref(s), 1, 0, 0, 1, 0, 0, None)
    assert rc == _lib.AO_ERR_INVALID_ARGUMENT and "the first moment's" in _lib.last_error()
    rc = lib.ao_optim_adam_step(None, None, 0, None, None, None, None, None, None, None, None, None, 5, 4096, 0, ctypes.byref(s), 1, 1, 0, 1, 0, 0, None)
    assert rc == _lib.AO_ERR_INVALID_ARGUMENT and "stochastic rounding is for bf16" in _lib.last_error()
    rc = lib.ao_optim_quantize(None, 0, None, None, None, 4000, 256, 0, None)
    assert rc == _lib.AO_ERR_INVALID_ARGUMENT and "multiple of block_size" in _lib.last_error()
    rc = lib.ao_optim_quantize(None, 0, None, None, None, 4096, 256, 5, None)
    assert rc == _lib.AO_ERR_INVALID_ARGUMENT and "format" in _lib.last_error()
    rc = lib.ao_optim_dequantize(None, None, None, None, 0, 4096, 256, 0, None)
    assert rc == _lib.AO_ERR_NULL_POINTER


# ---- stochastic rounding ----------------------------------------------------------------------------------------------------------------------------
def test_sr_restatement_shares_over_65536_counters():
    n = 1 << 16
    r16 = R.sr_random16(n, seed=0x1234_5678_9ABC_DEF0, step=3, param_index=1)
    assert r16.shape == (n,) and r16.max() < 65536
    hi = np.uint32(0x3F80_0000)  # 1.0
    for f in (1, 0x4000, 0x8000, 0xFFFF):
        x = np.full(n, hi | np.uint32(f), dtype=np.uint32).view(np.float32)
        out = R.sr_bf16(x, r16)
        assert set(np.unique(out).tolist()) <= {0x3F80, 0x3F81}
        share = float((out == 0x3F81).mean())
        print(f"f = {f:#06x}: share rounded away {share:.6f}, f / 65536 = {f / 65536:.6f}")
        assert abs(share - f / 65536) <= 2.0 ** -7
    x = np.full(n, hi, dtype=np.uint32).view(np.float32)
    assert np.all(R.sr_bf16(x, r16) == 0x3F80)                       # f = 0 never rounds
    neg = np.full(n, np.uint32(0xBF80_8000), dtype=np.uint32).view(np.float32)
    assert set(np.unique(R.sr_bf16(neg, r16)).tolist()) == {0xBF80, 0xBF81}  # away from zero, on either side
    assert not np.array_equal(r16, R.sr_random16(n, 0x1234_5678_9ABC_DEF0, 4, 1)) and not np.array_equal(r16, R.sr_random16(n, 0x1234_5678_9ABC_DEF0, 3, 2))
