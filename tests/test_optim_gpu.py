"""Low-bit optimizers on the GPU: the cast kernels and the fused Adam step against the reference's recording (tests/golden/optim.npz) and
against the numpy restatement (tests/optim_ref.py), byte for byte; the optimizer classes on a small MLP; stochastic rounding; the dispatcher op."""
import json
import math
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from ao_amd import ops
from ao_amd import optim as O
from ao_amd.optim import quant_utils as Q

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim.npz")
_raw = np.load(GOLDEN)
CASES = json.loads(str(_raw["cases"]))
QUANT_CASES = json.loads(str(_raw["quant_cases"]))
FORMAT = {"q8s": 0, "q8u": 1, "q4s": 2, "q4u": 3, "fp8": 4, "plain": 5}
FAMILY_FORMAT = {"q8": 0, "q4": 2, "fp8": 4, "plain": 5}


@pytest.fixture(scope="module")
def g():
    return R.load_golden(GOLDEN)


def qmaps_of(g):
    return {k: g[f"qmap_{k}"] for k in ("q8s", "q8u", "q4s", "q4u")}


def project_qmaps():
    return {k: Q.make_qmap(int(k[1]), k[2] == "s").numpy() for k in ("q8s", "q8u", "q4s", "q4u")}


def dev(a, bf16=False):
    """numpy -> GPU tensor; uint16 holding bf16 bits -> bfloat16"""
    a = np.ascontiguousarray(a)
    if bf16:
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).cuda()
    return torch.from_numpy(a.copy()).cuda()


def host(t):
    """GPU tensor -> numpy; bf16 as uint16 bits, fp8 as bytes"""
    t = t.detach().contiguous().reshape(-1)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.float8_e4m3fn:
        return t.view(torch.uint8).cpu().numpy()
    return t.cpu().numpy()


class DevStates:
    """the restatement's states (optim_ref.State) on the GPU, in the flat argument form of ops.optim_adam_step"""

    def __init__(self, states):
        self.kinds = [s.kind for s in states]
        self.fields = []
        for s in states:
            if s.kind == "plain":
                self.fields.append([dev(s.data, s.bf16), None, None])
            else:
                codes = dev(s.codes)
                self.fields.append([codes.view(torch.float8_e4m3fn) if s.kind == "fp8" else codes, dev(s.scale), None if s.qmap is None else dev(s.qmap)])
        if len(states) == 2:
            self.fields.append([None, None, None])

    def args(self):
        return [f for triple in self.fields for f in triple]

    def same_as(self, states, what):
        for k, s in enumerate(states):
            for name, want in s.fields().items():
                got = host(self.fields[k][0 if name in ("data", "codes") else 1])
                assert got.dtype == want.dtype and np.array_equal(got, want), (what, k, name, int((got != want).sum()))


def kernel_step(p, grad, ds, fmt, block_size, scalars, adamw, **kw):
    ops.optim_adam_step(p, grad, *ds.args(), fmt, block_size, [float(x) for x in scalars], adamw, **kw)


# ---- the casts ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", QUANT_CASES, ids=[c["name"] for c in QUANT_CASES])
def test_casts_on_the_planted_fixture(g, c):
    name, kind, bs = c["name"], c["kind"], c["block_size"]
    qmap = None if kind == "fp8" else dev(g[f"qmap_{kind}"])
    codes, scale = ops.optim_quantize(dev(g[f"{name}_x"]), FORMAT[kind], bs, qmap)
    assert np.array_equal(host(codes), g[f"{name}_codes"]) and np.array_equal(host(scale), g[f"{name}_scale"])
    deq = ops.optim_dequantize(codes, scale, FORMAT[kind], bs, qmap)
    assert deq.dtype == torch.float32 and np.array_equal(host(deq).view(np.uint32), g[f"{name}_deq"].view(np.uint32))
    every = dev(g[f"{name}_all_codes"])
    every = every.view(torch.float8_e4m3fn) if kind == "fp8" else every
    # every code under one scale: a block of 256 (or 128 for the 16 codes, each eight times)
    deq = ops.optim_dequantize(every, dev(g[f"{name}_all_scale"]), FORMAT[kind], c["all_block_size"], qmap)
    assert np.array_equal(host(deq).view(np.uint32), g[f"{name}_all_deq"].view(np.uint32))


@pytest.mark.parametrize("kind", ["q8s", "q8u", "q4s", "q4u", "fp8"])
@pytest.mark.parametrize("bs", [64, 128, 256, 512, 1024, 2048])
def test_casts_against_the_restatement_at_every_block_size(kind, bs):
    """bf16 and fp32 sources over two trips of the loop and a tail: every block size takes its own reduction width"""
    tile = ops.optim_grid(0)["tile"]
    n = 2 * tile + bs if bs < tile else 3 * bs
    rng = np.random.RandomState(bs + len(kind))
    x = (rng.standard_normal(n) * np.exp(rng.standard_normal(n // 64).repeat(64))).astype(np.float32)
    x = np.abs(x) if kind.endswith("u") else x
    qm = project_qmaps().get(kind)
    qmap = None if qm is None else dev(qm)
    for bf16 in (False, True):
        src = dev(R.f32_to_bf16(x), True) if bf16 else dev(x)
        xs = R.bf16_to_f32(R.f32_to_bf16(x)) if bf16 else x
        want_codes, want_scale = R.quantize(kind, xs, bs, qm)
        codes, scale = ops.optim_quantize(src, FORMAT[kind], bs, qmap)
        assert np.array_equal(host(codes), want_codes) and np.array_equal(host(scale), want_scale), (kind, bs, bf16)
        want = R.dequantize(kind, want_codes, want_scale, bs, qm)
        assert np.array_equal(host(ops.optim_dequantize(codes, scale, FORMAT[kind], bs, qmap)).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(host(ops.optim_dequantize(codes, scale, FORMAT[kind], bs, qmap, torch.bfloat16)), R.f32_to_bf16(want))


# ---- the step against the recording ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_adam_step_on_the_fixture_step_by_step(g, c):
    name, n = c["name"], math.prod(c["shape"])
    kind = c["family"] if c["quantized"] else "plain"
    ref_states = R.new_states(kind, n, c["block_size"], qmaps_of(g), c["bf16"], c["amsgrad"])
    ds = DevStates(ref_states)
    p = dev(g[f"{name}_p0"], c["bf16"])
    for t in range(1, c["steps"] + 1):
        kernel_step(p, dev(g[f"{name}_g{t}"], c["bf16"]), ds, FAMILY_FORMAT[kind], c["block_size"], g[f"{name}_scalars{t}"], c["adamw"])
        got = host(p)
        want = g[f"{name}_p{t}"]
        assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, want.view(np.uint32) if want.dtype == np.float32 else want), (name, t)
        for k, s in enumerate(ref_states):  # the recorded fields of step t into the restatement's holders, then compare
            for field in s.fields():
                setattr(s, field, g[f"{name}_s{k}_{field}{t}"])
        ds.same_as(ref_states, (name, t))


# ---- the step against the restatement where the loop takes further trips -------------------------------------------------------------------------
def _scalars(lr, betas, wd, eps, t):
    return O.step_scalars(torch.tensor(lr, dtype=torch.float32), betas[0], betas[1], wd, eps, torch.tensor(float(t)))


@pytest.mark.parametrize("family,bs", [("q8", 256), ("q4", 128), ("fp8", 256), ("q8", 2048), ("q4", 64), ("plain", 0)])
@pytest.mark.parametrize("bf16", [True, False])
def test_adam_step_against_the_restatement_over_loop_trips_and_a_tail(family, bs, bf16):
    """3 workgroups over 8 tiles: every workgroup takes a second trip, two a third, and the last tile is a tail of one block (plain: of 5 elements,
    which ends inside a lane's run of 16)"""
    wg = 3
    tile = ops.optim_grid(0)["tile"]
    n = 7 * tile + (max(bs, 64) if family != "plain" else 5)
    assert ops.optim_grid(n, wg) == {"tile": tile, "tiles": 8, "workgroups": wg}
    rng = np.random.RandomState(n % 1000 + bs)
    qm = project_qmaps()
    to_store = (lambda a: R.f32_to_bf16(a)) if bf16 else (lambda a: a.astype(np.float32))
    p_ref = to_store((rng.standard_normal(n) * 0.1).astype(np.float32))
    ref_states = R.new_states(family, n, bs, qm, bf16, True)
    ds = DevStates(ref_states)
    p = dev(p_ref, bf16)
    for t in (1, 2):
        grad = to_store((rng.standard_normal(n) * 0.02 * np.exp(rng.standard_normal(n // 8 + 1).repeat(8)[:n])).astype(np.float32))
        sc = _scalars(1e-3, (0.9, 0.999), 1e-2, 1e-8, t)
        p_ref = R.adam_step(p_ref, grad, ref_states, dict(zip(R.SCALAR_NAMES, sc)), True, bf16)
        kernel_step(p, dev(grad, bf16), ds, FAMILY_FORMAT[family], bs, sc, True, max_workgroups=wg)
        got = host(p)
        assert np.array_equal(got.view(np.uint32) if not bf16 else got, p_ref.view(np.uint32) if not bf16 else p_ref), (family, bs, bf16, t)
        ds.same_as(ref_states, (family, bs, bf16, t))


def test_the_bytes_do_not_depend_on_the_grid_or_the_run():
    tile = ops.optim_grid(0)["tile"]
    n = 5 * tile + 256
    rng = np.random.RandomState(11)
    p0, grad = R.f32_to_bf16(rng.standard_normal(n).astype(np.float32)), R.f32_to_bf16((rng.standard_normal(n) * 0.01).astype(np.float32))
    sc = _scalars(1e-3, (0.9, 0.999), 1e-2, 1e-8, 1)
    outs = []
    for wg in (0, 0, 1, 2, 6):
        ds = DevStates(R.new_states("q8", n, 256, project_qmaps(), True, True))
        p = dev(p0, True)
        kernel_step(p, dev(grad, True), ds, 0, 256, sc, True, sr=True, seed=5, step=1, param_index=0, max_workgroups=wg)
        outs.append([host(p)] + [host(f) for f in ds.args() if f is not None])
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], o))


# ---- stochastic rounding --------------------------------------------------------------------------------------------------------------------------------
def test_stochastic_rounding_is_the_restatements_bytes():
    tile = ops.optim_grid(0)["tile"]
    n = tile + 4096 + 13  # plain states: the count need not be whole groups of 8
    rng = np.random.RandomState(3)
    p0, grad = R.f32_to_bf16(rng.standard_normal(n).astype(np.float32)), R.f32_to_bf16((rng.standard_normal(n) * 0.01).astype(np.float32))
    sc = _scalars(1e-2, (0.9, 0.999), 0.0, 1e-8, 1)
    seed = 0xF123_4567_89AB_CDEF  # the top bit set: torch.initial_seed() is unsigned

    def run(family, nn, **kw):
        ds = DevStates(R.new_states(family, nn, 256, project_qmaps(), True, False))
        p = dev(p0[:nn], True)
        kernel_step(p, dev(grad[:nn], True), ds, FAMILY_FORMAT[family], 256 if family != "plain" else 0, sc, True, **kw)
        return host(p)

    def want(family, nn, sr):
        return R.adam_step(p0[:nn], grad[:nn], R.new_states(family, nn, 256, project_qmaps(), True, False), dict(zip(R.SCALAR_NAMES, sc)), True, True, sr=sr)

    for family, nn in (("plain", n), ("q8", tile + 4096)):
        a = run(family, nn, sr=True, seed=seed, step=7, param_index=2)
        assert np.array_equal(a, want(family, nn, (seed, 7, 2)))
        rtne = run(family, nn, sr=False, seed=seed, step=7, param_index=2)
        assert np.array_equal(rtne, want(family, nn, None)) and not np.array_equal(a, rtne)
        assert not np.array_equal(a, run(family, nn, sr=True, seed=seed, step=8, param_index=2))
        assert not np.array_equal(a, run(family, nn, sr=True, seed=seed, step=7, param_index=3))
        assert not np.array_equal(a, run(family, nn, sr=True, seed=seed ^ 1, step=7, param_index=2))
    with pytest.raises(RuntimeError, match="stochastic rounding is for bfloat16"):
        ops.optim_adam_step(torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), None, None,
                            torch.zeros(8, device="cuda"), None, None, None, None, None, 5, 0, sc, True, sr=True)


# ---- the optimizer classes on a small MLP ---------------------------------------------------------------------------------------------------------------
def _mlp(device):
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.GELU(), torch.nn.Linear(128, 64)).to(torch.bfloat16)
    return m.to(device)


def _batch(device):
    gen = torch.Generator().manual_seed(1)
    return torch.randn(32, 64, generator=gen).to(torch.bfloat16).to(device), torch.randn(32, 64, generator=gen).to(torch.bfloat16).to(device)


class RestatedOptimizer:
    """the numpy restatement driven like an optimizer over torch parameters on any device: the creation rule, one step count, param_index in order"""

    def __init__(self, params, family, block_size, adamw, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0, amsgrad=False, sr_seed=None):
        self.params, self.adamw, self.hyper, self.t, self.sr_seed = list(params), adamw, (lr, betas, wd, eps), 0, sr_seed
        qm = project_qmaps()
        self.states = []
        for p in self.params:
            n = p.numel()
            quantized = family != "plain" and n >= 4096 and n % block_size == 0
            self.states.append(R.new_states(family if quantized else "plain", n, block_size, qm, True, amsgrad))

    def step(self):
        self.t += 1
        lr, betas, wd, eps = self.hyper
        sc = dict(zip(R.SCALAR_NAMES, _scalars(lr, betas, wd, eps, self.t)))
        for i, p in enumerate(self.params):
            new = R.adam_step(host(p.data) if p.is_cuda else _bits_cpu(p.data), host(p.grad) if p.is_cuda else _bits_cpu(p.grad), self.states[i], sc,
                              self.adamw, True, sr=None if self.sr_seed is None else (self.sr_seed, self.t, i))
            p.data.copy_(torch.from_numpy(new.view(np.int16).copy()).view(torch.bfloat16).view(p.shape))


def _bits_cpu(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1).copy()


OPTIMIZERS = [(O.Adam8bit, "q8", 256, False, 0.0), (O.Adam4bit, "q4", 128, False, 0.0), (O.AdamFp8, "fp8", 256, False, 0.0),
              (O.AdamW8bit, "q8", 256, True, 1e-2), (O.AdamW4bit, "q4", 128, True, 1e-2), (O.AdamWFp8, "fp8", 256, True, 1e-2),
              (O._AdamW, "plain", 0, True, 1e-2)]


@pytest.mark.parametrize("cls,family,bs,adamw,wd", OPTIMIZERS, ids=[o[0].__name__ for o in OPTIMIZERS])
@pytest.mark.parametrize("amsgrad,sr", [(False, False), (True, True)])
def test_optimizer_classes_on_an_mlp_are_the_restatement_bit_for_bit(cls, family, bs, adamw, wd, amsgrad, sr):
    model = _mlp("cuda")
    x, y = _batch("cuda")
    opt = cls(model.parameters(), lr=1e-3, amsgrad=amsgrad, bf16_stochastic_round=sr, sr_seed=99)
    shadow = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    ref = RestatedOptimizer(shadow, family, bs, adamw, wd=wd, amsgrad=amsgrad, sr_seed=99 if sr else None)
    for step in range(3):
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(x), y).backward()
        for s, p in zip(shadow, model.parameters()):
            s.grad = p.grad.detach().clone()
        opt.step()
        ref.step()
        for i, (s, p) in enumerate(zip(shadow, model.parameters())):
            assert np.array_equal(host(p.data), host(s.data)), (step, i)
            st = opt.state[p]
            assert float(st["step"]) == step + 1 and st["step"].device.type == "cpu"
            keys = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if amsgrad else [])
            for k, key in enumerate(keys):
                want = ref.states[i][k]
                quantized = family != "plain" and p.numel() >= 4096
                assert (type(st[key]) is not torch.Tensor) == quantized
                if quantized:
                    assert np.array_equal(host(st[key].codes), want.codes) and np.array_equal(host(st[key].scale), want.scale), (step, i, key)
                else:
                    assert np.array_equal(host(st[key]), want.data), (step, i, key)
    w = opt.state[next(iter(model.parameters()))]["exp_avg"]
    if family != "plain":  # dequantize() and the float <- state copy are the dequantize kernel
        want = R.dequantize(ref.states[0][0].kind, ref.states[0][0].codes, ref.states[0][0].scale, bs, ref.states[0][0].qmap)
        assert np.array_equal(host(w.dequantize()).view(np.uint32), want.view(np.uint32)) and w.dequantize().shape == (128, 64)
        out = torch.empty(128, 64, device="cuda")
        out.copy_(w)
        assert np.array_equal(host(out).view(np.uint32), want.view(np.uint32))
        w2 = type(w).zeros((128, 64), block_size=bs, device="cuda") if family == "fp8" else type(w).zeros((128, 64), True, bs, device="cuda")
        w2.copy_(out)  # state <- float: the quantize kernel
        c2, s2 = R.quantize(ref.states[0][0].kind, want, bs, ref.states[0][0].qmap)
        assert np.array_equal(host(w2.codes), c2) and np.array_equal(host(w2.scale), s2)


def test_two_runs_give_the_same_bytes():
    outs = []
    for _ in range(2):
        model = _mlp("cuda")
        x, y = _batch("cuda")
        opt = O.AdamW4bit(model.parameters(), bf16_stochastic_round=True, sr_seed=4)
        for _ in range(3):
            opt.zero_grad()
            torch.nn.functional.mse_loss(model(x), y).backward()
            opt.step()
        outs.append([host(p.data) for p in model.parameters()] + [host(opt.state[p]["exp_avg_sq"].codes) for p in list(model.parameters())[::2]])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_the_loss_falls_over_20_adamw8bit_steps():
    def train(device, make_opt):
        model = _mlp(device)
        x, y = _batch(device)
        opt = make_opt(model)
        losses = []
        for _ in range(20):
            for p in model.parameters():
                p.grad = None
            loss = torch.nn.functional.mse_loss(model(x), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        losses.append(float(torch.nn.functional.mse_loss(model(x), y).detach()))
        return losses

    restated = train("cpu", lambda m: RestatedOptimizer(m.parameters(), "q8", 256, True, lr=1e-3, wd=1e-2))
    print("restatement: loss", restated[0], "->", restated[-1])
    assert restated[-1] < restated[0]  # the contract trains; then the kernels
    fused = train("cuda", lambda m: O.AdamW8bit(m.parameters(), lr=1e-3))
    print("AdamW8bit:   loss", fused[0], "->", fused[-1])
    assert fused[-1] < fused[0]


# ---- the dispatcher op -------------------------------------------------------------------------------------------------------------------------------------
def test_the_dispatcher_ops_equal_the_direct_calls():
    import ao_amd.torch_ops  # noqa: F401  (registers ao_mi355::optim_*)

    n = 8192
    rng = np.random.RandomState(8)
    p0, grad = R.f32_to_bf16(rng.standard_normal(n).astype(np.float32)), R.f32_to_bf16((rng.standard_normal(n) * 0.01).astype(np.float32))
    sc = _scalars(1e-3, (0.9, 0.999), 1e-2, 1e-8, 1)
    res = []
    for call in (ops.optim_adam_step, torch.ops.ao_mi355.optim_adam_step):
        ds = DevStates(R.new_states("q8", n, 256, project_qmaps(), True, True))
        p = dev(p0, True)
        out = call(p, dev(grad, True), *ds.args(), 0, 256, [float(v) for v in sc], True, True, 17, 1, 0, 0)
        assert out is None
        res.append([host(p)] + [host(f) for f in ds.args() if f is not None])
    assert all(np.array_equal(a, b) for a, b in zip(*res)) and not np.array_equal(res[0][0], p0)
    x = dev(rng.standard_normal(n).astype(np.float32))
    qmap = dev(project_qmaps()["q4s"])
    a, b = ops.optim_quantize(x, 2, 128, qmap), torch.ops.ao_mi355.optim_quantize(x, 2, 128, qmap)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.optim_dequantize(a[0], a[1], 2, 128, qmap), torch.ops.ao_mi355.optim_dequantize(a[0], a[1], 2, 128, qmap, torch.float32))
