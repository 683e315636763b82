"""GPU: SmoothQuant's kernels against tests/smoothquant_ref.py byte for byte, the fused routing of the Int8Tensor linear against the parent
route, the observers against the fixture recorded from the reference, and SmoothQuantConfig end to end.

Layers.  (A) ops.sq_col_absmax_update and (B) ops.sq_smoothed_amax_update: the restatement's bytes at one row, at the seams of the four-wave
row walk (63, 64, 65), at more rows than one workgroup takes (257, 1031) and at column counts of one slice, just under, at and over one
512-column tile and over eight; folding over batches; a second update with smaller values; two launches.  (C) the three pre-scaled casts
through the C ABI into poisoned buffers: the existing cast on `x * pre` computed on the device, and the restatement, at the register form's
depths 1, 2 and 8 and the first K of the two-sweep form.  (routing) every supported base config: output bytes of the parent route, and no
elementwise multiply on the fused routes.  (observers) the fixture's x_abs_max exactly, the smoothing factor within one bf16 ulp (an fp32
pow that differs in its last places can move the bf16 rounding by at most one step), everything downstream equal to the restatement applied
to the device's own factor.  (end to end) the reference's accuracy test on its toy model, the two-pass flow, prepare_for_loading, save / load.
"""
import io
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _parity
import smoothquant_cases as C
import smoothquant_ref as R
from oracle import bf16

pytestmark = pytest.mark.gpu

from ao_amd import _lib, ops  # noqa: E402
from ao_amd.prototype.smoothquant import (  # noqa: E402
    RunningAbsMaxSmoothQuantObserver,
    SmoothQuantConfig,
    SmoothQuantObservedLinear,
    SmoothQuantObserver,
)
from ao_amd.quantization import quantize_  # noqa: E402
from ao_amd.quantization.config import Int8DynamicActivationInt8WeightConfig, Int8StaticActivationInt8WeightConfig  # noqa: E402
from ao_amd.quantization.granularity import PerRow, PerTensor  # noqa: E402
from ao_amd.quantization.int8_tensor import Int8Tensor  # noqa: E402
from ao_amd.quantization.quant_primitives import MappingType  # noqa: E402

DEV = torch.device("cuda", 0)
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smoothquant.npz"))
META = json.loads(str(GOLDEN["meta"]))
MS = (1, 2, 63, 64, 65, 257, 1031)
KS = (8, 504, 512, 520, 4104)
CAST_MS = (1, 3, 64, 65)
CAST_KS = (8, 264, 2048, 2056, 16384, 16392)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_bf16(a):
    assert bf16.is_bf16(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(DEV).contiguous()


def bits32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same32(got, want):
    want = np.asarray(want, np.float32)
    return tuple(got.shape) == want.shape and np.array_equal(bits32(got).reshape(-1), want.reshape(-1).view(np.uint32))


class Out:
    """`count` elements of a numpy dtype in a poisoned, guarded buffer of bytes (16-byte aligned)"""

    def __init__(self, count, dtype):
        self.count, self.dtype = count, np.dtype(dtype)
        self.nbytes = count * self.dtype.itemsize
        self.g = _parity.Guarded(1, (self.nbytes + 1) // 2, torch.bfloat16, DEV)
        self.ptr = self.g.out.data_ptr()

    def get(self):
        assert not self.g.guard_problems(), self.g.guard_problems()
        raw = self.g.bits().contiguous().view(torch.uint8).reshape(-1).cpu().numpy()
        return raw[:self.nbytes].view(self.dtype).copy()


# ---- A: the running per-column absmax ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_col_absmax_equals_the_restatement_byte_for_byte(K):
    for M in MS:
        x = C.activation(M, K, 7 * M + K)
        xd = dev_bf16(x)
        state = torch.zeros(K, dtype=torch.float32, device=DEV)
        assert ops.sq_col_absmax_update(xd, state) is state
        again = ops.sq_col_absmax_update(xd, torch.zeros(K, dtype=torch.float32, device=DEV))
        want = R.col_absmax(x)
        assert same32(state, want), (M, K, int((bits32(state) != want.view(np.uint32)).sum()))
        assert torch.equal(state, again), "two launches gave different bytes"
        assert torch.equal(state, xd.float().abs().amax(0))


def test_col_absmax_folds_batches_like_the_concatenation_and_keeps_larger_state():
    K = 520
    xs = [C.activation(m, K, 40 + i, scale=s) for i, (m, s) in enumerate(((65, 1.0), (3, 8.0), (257, 0.25)))]
    state = torch.zeros(K, dtype=torch.float32, device=DEV)
    for x in xs:
        ops.sq_col_absmax_update(dev_bf16(x), state)
    cat = ops.sq_col_absmax_update(dev_bf16(np.concatenate(xs)), torch.zeros(K, dtype=torch.float32, device=DEV))
    assert torch.equal(state, cat) and same32(state, R.col_absmax(np.concatenate(xs)))
    before = state.clone()
    ops.sq_col_absmax_update(dev_bf16(bf16.bf16_round(xs[0] * np.float32(0.5))), state)  # nothing in it is larger
    assert torch.equal(state, before)
    # a state that is not bf16-representable and larger than the input stays as it is, bit for bit
    big = torch.full((K,), 3.0000002e38, dtype=torch.float32, device=DEV)
    ops.sq_col_absmax_update(dev_bf16(xs[1]), big)
    assert torch.all(big == 3.0000002e38)
    # a 0-row update is no update; a strided input is made contiguous
    ops.sq_col_absmax_update(torch.empty(0, K, dtype=torch.bfloat16, device=DEV), state)
    wide = dev_bf16(C.activation(5, 2 * K, 9))
    got = ops.sq_col_absmax_update(wide[:, :K], torch.zeros(K, dtype=torch.float32, device=DEV))
    assert torch.equal(state, before) and torch.equal(got, wide[:, :K].float().abs().amax(0))


# ---- B: the running amax of the smoothed activation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_smoothed_amax_equals_the_restatement_byte_for_byte(K):
    for M in MS:
        x, s = C.activation(M, K, 11 * M + K), C.smoothing_vector(K, M + K)
        xd, sd = dev_bf16(x), dev_bf16(s)
        amax = torch.zeros(1, dtype=torch.float32, device=DEV)
        assert ops.sq_smoothed_amax_update(xd, sd, amax) is amax
        again = ops.sq_smoothed_amax_update(xd, sd, torch.zeros(1, dtype=torch.float32, device=DEV))
        want = R.smoothed_amax(x, s)
        assert np.isfinite(want) and same32(amax, [want]), (M, K, float(amax), float(want))
        assert torch.equal(amax, again)
        assert torch.equal(amax, (xd / sd).abs().amax().float().reshape(1))  # the reference's tensor ops on the device


def test_smoothed_amax_folds_batches_and_keeps_larger_state():
    K = 4104
    s = C.smoothing_vector(K, 3)
    xs = [C.activation(m, K, 60 + i, big=False, scale=sc) for i, (m, sc) in enumerate(((5, 1.0), (200, 4.0), (7, 0.5)))]
    amax = torch.zeros(1, dtype=torch.float32, device=DEV)
    want, seen = np.float32(0), []
    for x in xs:
        ops.sq_smoothed_amax_update(dev_bf16(x), dev_bf16(s), amax)
        want = R.smoothed_amax(x, s, want)
        seen.append(float(amax))
        assert same32(amax, [want])
    assert seen[0] < seen[1] == seen[2]  # the second batch raised it, the third left it
    assert want == R.smoothed_amax(np.concatenate(xs), s)


# ---- C: the pre-scaled casts -----------------------------------------------------------------------------------------------------------------------
def cast_inputs(M, K):
    x, pre = C.activation(M, K, 13 * M + K), C.pre_scale(K, M + K)
    xd, pd = dev_bf16(x), dev_bf16(pre)
    td = xd * pd  # the parent route's multiply, on the device
    assert np.array_equal(td.float().cpu().numpy().view(np.uint32), R.prescaled(x, pre).view(np.uint32)), "x * pre differs from the restatement"
    return x, pre, xd, pd, td


@pytest.mark.parametrize("K", CAST_KS)
def test_rowwise_prescaled_cast_equals_its_twin_and_the_restatement(K):
    lib = _lib.lib()
    for M in CAST_MS:
        x, pre, xd, pd, td = cast_inputs(M, K)
        q, s = Out(M * K, np.int8), Out(M, np.float32)
        _lib.check(lib.ao_int8_quantize_rowwise_prescaled(xd.data_ptr(), pd.data_ptr(), q.ptr, s.ptr, M, K, stream()))
        tq, ts = ops.int8_quantize_rowwise(td)
        torch.cuda.synchronize()
        gq, gs = q.get().reshape(M, K), s.get()
        assert np.array_equal(gq, tq.cpu().numpy()) and np.array_equal(gs.view(np.uint32), bits32(ts).reshape(-1)), ("twin", M, K)
        wq, ws = R.quantize_rowwise_prescaled(x, pre)
        assert np.array_equal(gq, wq) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), ("restatement", M, K)
        oq, os_ = ops.int8_quantize_rowwise_prescaled(xd, pd)
        assert torch.equal(oq, tq) and torch.equal(os_, ts) and os_.shape == (M, 1)


@pytest.mark.parametrize("K", CAST_KS)
def test_tensorwise_prescaled_cast_equals_its_twin_and_the_restatement(K):
    lib = _lib.lib()
    for M in CAST_MS:
        x, pre, xd, pd, td = cast_inputs(M, K)
        q, s, amax = Out(M * K, np.int8), Out(M, np.float32), Out(1, np.float32)
        _lib.check(lib.ao_int8_quantize_tensorwise_prescaled(xd.data_ptr(), pd.data_ptr(), amax.ptr, q.ptr, s.ptr, M, K, stream()))
        tq, ts = ops.int8_quantize_tensorwise(td)
        torch.cuda.synchronize()
        gq, gs, ga = q.get().reshape(M, K), s.get(), amax.get()
        assert ga[0] == np.abs(R.prescaled(x, pre)).max()
        assert np.array_equal(gq, tq.cpu().numpy()) and np.all(gs.view(np.uint32) == bits32(ts).reshape(-1)[0]), ("twin", M, K)
        wq, ws = R.quantize_tensorwise_prescaled(x, pre)
        assert np.array_equal(gq, wq) and np.all(gs == np.float32(ws)), ("restatement", M, K)
        oq, os_ = ops.int8_quantize_tensorwise_prescaled(xd, pd)
        assert torch.equal(oq, tq) and torch.equal(os_, ts) and os_.shape == (1, 1)


@pytest.mark.parametrize("with_zp", [False, True])
@pytest.mark.parametrize("K", CAST_KS)
def test_static_prescaled_cast_equals_its_twin_and_the_restatement(K, with_zp):
    lib = _lib.lib()
    for M in CAST_MS:
        for per_row in (0, 1):
            x, pre, xd, pd, td = cast_inputs(M, K)
            rng = np.random.default_rng(K + M + per_row)
            n = M if per_row else 1
            scale = np.exp(rng.uniform(-4.0, 1.0, size=n)).astype(np.float32)
            scale[0] = 0.25  # a power of two: half-integers of t / scale land on ties
            zp = rng.integers(-128, 128, size=n).astype(np.int8) if with_zp else None
            sd = torch.from_numpy(scale).to(DEV)
            zd = torch.from_numpy(zp).to(DEV) if with_zp else None
            q = Out(M * K, np.int8)
            _lib.check(lib.ao_int8_quantize_static_prescaled(xd.data_ptr(), pd.data_ptr(), sd.data_ptr(), zd.data_ptr() if with_zp else None,
                                                             per_row, q.ptr, M, K, stream()))
            tq = ops.int8_quantize_static(td, sd, zd)
            torch.cuda.synchronize()
            gq = q.get().reshape(M, K)
            assert np.array_equal(gq, tq.cpu().numpy()), ("twin", M, K, per_row)
            assert np.array_equal(gq, R.quantize_static_prescaled(x, pre, scale, zp)), ("restatement", M, K, per_row)
            assert torch.equal(ops.int8_quantize_static_prescaled(xd, pd, sd, zd), tq)


# ---- routing: the converted linear against the parent route -----------------------------------------------------------------------------------
ROUTED = {
    "dyn-row": Int8DynamicActivationInt8WeightConfig(),
    "dyn-tensor": Int8DynamicActivationInt8WeightConfig(granularity=PerTensor()),
    "dyn-row-wtensor": Int8DynamicActivationInt8WeightConfig(granularity=[PerRow(), PerTensor()]),
    "dyn-tensor-wrow": Int8DynamicActivationInt8WeightConfig(granularity=[PerTensor(), PerRow()]),
    "dyn-asym": Int8DynamicActivationInt8WeightConfig(act_mapping_type=MappingType.ASYMMETRIC),
    "static-tensor": Int8StaticActivationInt8WeightConfig(granularity=PerTensor()),
    "static-tensor-wrow": Int8StaticActivationInt8WeightConfig(granularity=[PerTensor(), PerRow()]),
}
ROUTE_N, ROUTE_K = 256, 512


class MulSpy:
    """Counts the elementwise multiplies Python code asks torch for: Tensor.__mul__ / __rmul__ and torch.mul"""

    def __enter__(self):
        self.count = 0
        self.saved = (torch.Tensor.__mul__, torch.Tensor.__rmul__, torch.mul)

        def wrap(fn):
            def counted(*a, **k):
                self.count += 1
                return fn(*a, **k)
            return counted

        torch.Tensor.__mul__, torch.Tensor.__rmul__, torch.mul = wrap(self.saved[0]), wrap(self.saved[1]), wrap(self.saved[2])
        return self

    def __exit__(self, *exc):
        torch.Tensor.__mul__, torch.Tensor.__rmul__, torch.mul = self.saved
        return False


def converted_linear(base, seed=0, bias=True):
    W = dev_bf16(C.weight(ROUTE_N, ROUTE_K, seed))
    lin = nn.Linear(ROUTE_K, ROUTE_N, bias=bias, device=DEV, dtype=torch.bfloat16)
    lin.weight = nn.Parameter(W, requires_grad=False)
    m = nn.Sequential(lin)
    quantize_(m, SmoothQuantConfig(base, step="prepare", alpha=0.5))
    for i, rows in enumerate((5, 130)):
        m(dev_bf16(C.activation(rows, ROUTE_K, 70 + i, big=False)))
    quantize_(m, SmoothQuantConfig(base, step="convert", alpha=0.5))
    return m[0]


@pytest.mark.parametrize("kind", list(ROUTED))
def test_converted_linear_equals_the_parent_route_and_launches_no_multiply(kind):
    lin = converted_linear(ROUTED[kind])
    w = lin.weight
    assert isinstance(w, Int8Tensor) and w.act_pre_scale.dtype == torch.bfloat16 and w.act_pre_scale.shape == (ROUTE_K,)
    parent_w = Int8Tensor(w.qdata, w.scale, w.block_size, w.dtype_, w.act_quant_kwargs, None, w.zero_point, w.w_row_sums, w.act_quant_scale,
                          w.act_quant_zero_point)  # the same weight without the pre-scale: the parent route multiplies first
    for M in (1, 2, 17, 130):
        x = dev_bf16(C.activation(M, ROUTE_K, 90 + M, big=False))
        with MulSpy() as parent_spy:
            want = F.linear(x * w.act_pre_scale, parent_w, lin.bias)
        with MulSpy() as spy:
            got = lin(x)
        assert parent_spy.count >= 1  # the spy sees the parent's multiply
        assert got.dtype == torch.bfloat16 and got.shape == (M, ROUTE_N) and torch.equal(got.view(torch.int16), want.view(torch.int16)), (kind, M)
        keeps_multiply = kind == "dyn-asym" or (kind in ("dyn-row", "dyn-row-wtensor") and M == 1)  # (one row: DESIGN.md 4.29)
        assert spy.count == (1 if keeps_multiply else 0), (kind, M, spy.count)
        if M == 17:  # a 3-D activation takes the same route
            assert torch.equal(lin(x.reshape(1, M, ROUTE_K)).reshape(M, ROUTE_N), got)


def test_other_pre_scales_and_dtypes_keep_the_multiply():
    lin = converted_linear(ROUTED["dyn-row"], bias=False)
    w = lin.weight
    x = dev_bf16(C.activation(17, ROUTE_K, 5, big=False))
    want = lin(x)
    w2 = Int8Tensor(w.qdata, w.scale, w.block_size, w.dtype_, w.act_quant_kwargs, w.act_pre_scale.reshape(1, ROUTE_K))  # a broadcast shape
    with MulSpy() as spy:
        assert torch.equal(F.linear(x, w2), want)
    assert spy.count == 1
    w3 = Int8Tensor(w.qdata, w.scale, w.block_size, w.dtype_, w.act_quant_kwargs, w.act_pre_scale.float())  # fp32: the product is fp32
    with MulSpy() as spy:
        y = F.linear(x, w3)
    assert spy.count >= 1 and y.dtype == torch.bfloat16 and y.shape == want.shape
    with MulSpy() as spy:  # fp32 activations: the reference-dtype path, after the multiply
        y = lin(x.float())
    assert spy.count >= 1 and y.dtype == torch.float32


def test_fused_routes_trace_through_their_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    for kind in ("dyn-row", "dyn-tensor", "static-tensor"):
        w = converted_linear(ROUTED[kind], bias=False).weight
        pre, scale = w.act_pre_scale, w._row_scale()
        with FakeTensorMode(allow_non_fake_inputs=True) as mode:
            x = mode.from_tensor(torch.empty(17, ROUTE_K, dtype=torch.bfloat16, device=DEV))
            if kind == "dyn-row":
                y = torch.ops.ao_mi355.int8_linear_prescaled(x, pre, w.qdata, scale, None)
            elif kind == "dyn-tensor":
                y = torch.ops.ao_mi355.int8_linear_tensorwise_prescaled(x, pre, w.qdata, scale, None)
            else:
                y = torch.ops.ao_mi355.int8_linear_static_prescaled(x, pre, w.qdata, scale, w.act_quant_scale, None, None, None)
        assert y.shape == (17, ROUTE_N) and y.dtype == torch.bfloat16


# ---- the observers against the fixture ---------------------------------------------------------------------------------------------------------
def golden_inputs():
    return [GOLDEN[f"x{i}"] for i in range(len(META["batches"]))]


def ulps_apart(a_bits, b_bits):
    return np.abs(a_bits.astype(np.int64) - b_bits.astype(np.int64)).max()


@pytest.mark.parametrize("i", range(len(META["alphas"])), ids=[f"alpha={a}" for a in META["alphas"]])
def test_observers_and_convert_against_the_fixture(i):
    alpha, p = META["alphas"][i], f"a{i}_"
    Wn, xs = GOLDEN["W"], golden_inputs()
    W = dev_bf16(Wn)
    obs, run = SmoothQuantObserver(W, alpha), RunningAbsMaxSmoothQuantObserver(W, alpha)
    for x in xs:
        xd = dev_bf16(x)
        assert obs(xd) is xd and run(xd) is xd
    for o in (obs, run):
        assert o.x_abs_max.is_cuda and np.array_equal(bf16.to_bits(o.x_abs_max.cpu().numpy()), GOLDEN["x_abs_max"])
    assert np.array_equal(bf16.to_bits(obs.w_abs_max().float().cpu().numpy()), GOLDEN["w_abs_max"])
    kwargs = Int8StaticActivationInt8WeightConfig(granularity=PerTensor()).get_act_quant_kwargs()
    sf, act_scale, zp = obs.calculate_qparams(kwargs)
    s = sf.float().cpu().numpy()
    # positive bf16 values: adjacent bit patterns are adjacent values
    assert sf.dtype == torch.bfloat16 and ulps_apart(bf16.to_bits(s), GOLDEN[p + "sf_bits"]) <= 1 and zp is None
    if alpha is None:
        assert np.all(s == 1)
    # downstream of the device's own factor: the restatement's bytes
    amax = np.float32(0)
    for x in xs:
        amax = R.smoothed_amax(x, s, amax)
    assert act_scale.shape == (1, 1) and same32(act_scale, np.full((1, 1), R.static_scale(amax), np.float32))
    assert torch.equal(run.compute_smoothing_factor(), sf)
    for x in xs:
        run(dev_bf16(x))
    sf_r, scale_r, zp_r = run.calculate_qparams(kwargs)
    assert torch.equal(sf_r, sf) and zp_r is None and scale_r.shape == () and same32(scale_r, np.float32(R.running_scale(amax)))
    if np.array_equal(bf16.to_bits(s), GOLDEN[p + "sf_bits"]):  # the same factor: the reference's own recorded scales
        assert act_scale.item() == GOLDEN[p + "static_act_scale"].item() and scale_r.item() == GOLDEN[p + "running_act_scale"].item()

    # convert through quantize_: act_pre_scale, qdata and the weight scale
    Ws = R.smoothed_weight(Wn, s)
    for base, per_tensor, running in ((Int8DynamicActivationInt8WeightConfig(), False, False),
                                      (Int8StaticActivationInt8WeightConfig(granularity=PerTensor()), True, False),
                                      (Int8StaticActivationInt8WeightConfig(granularity=PerTensor()), True, True)):
        lin = nn.Linear(META["K"], META["N"], bias=False, device=DEV, dtype=torch.bfloat16)
        lin.weight = nn.Parameter(W.clone(), requires_grad=False)
        m = nn.Sequential(lin)
        quantize_(m, SmoothQuantConfig(base, step="prepare", alpha=alpha, use_running_absmax=running))
        assert isinstance(m[0], SmoothQuantObservedLinear)
        for x in xs:
            m(dev_bf16(x))
        if running:
            quantize_(m, SmoothQuantConfig(base, step="prepare_for_smoothquant_smoothing_factor", alpha=alpha, use_running_absmax=True))
            for x in xs:
                m(dev_bf16(x))
        quantize_(m, SmoothQuantConfig(base, step="convert", alpha=alpha, use_running_absmax=running))
        w = m[0].weight
        assert type(m[0]) is nn.Linear and isinstance(w, Int8Tensor)
        assert np.array_equal(bf16.to_bits(w.act_pre_scale.float().cpu().numpy()), bf16.to_bits(R.pre_scale(s)))
        q, sc = R.quantize_weight(Ws, per_tensor=per_tensor)
        assert np.array_equal(w.qdata.cpu().numpy(), q) and same32(w.scale.reshape(-1), np.asarray(sc, np.float32).reshape(-1))
        if per_tensor:
            want = R.running_scale(amax) if running else R.static_scale(amax)
            assert w.act_quant_zero_point is None and same32(w.act_quant_scale.reshape(-1), np.asarray([want], np.float32))
            assert w.act_quant_scale.shape == (() if running else (1, 1))
        else:
            assert w.act_quant_scale is None
        if np.array_equal(bf16.to_bits(s), GOLDEN[p + "sf_bits"]):
            key = "static" if per_tensor else "dyn"
            assert np.array_equal(w.qdata.cpu().numpy(), GOLDEN[p + key + "_qdata"])
            assert np.array_equal(w.scale.cpu().numpy().reshape(-1), GOLDEN[p + key + "_scale"].reshape(-1))


def test_observers_take_other_dtypes_through_torch_ops_onto_the_same_state():
    W = dev_bf16(GOLDEN["W"])
    obs = SmoothQuantObserver(W, 0.5, keep_inputs=False)
    xs = golden_inputs()
    obs(dev_bf16(xs[0]))
    obs(torch.from_numpy(xs[1]).to(DEV))           # fp32 on the device
    obs(torch.from_numpy(xs[2]).to(torch.bfloat16))  # bf16 on the CPU: moved to the weight's device
    assert np.array_equal(bf16.to_bits(obs.x_abs_max.cpu().numpy()), GOLDEN["x_abs_max"]) and obs.calibration_count == 3


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
class Toy(nn.Module):
    """the reference test's ToyLinearModel (test/prototype/test_smoothquant.py:33-65)"""

    def __init__(self, weights):
        super().__init__()
        for i, w in enumerate(weights):
            lin = nn.Linear(w.shape[1], w.shape[0], bias=False, device=DEV, dtype=torch.bfloat16)
            lin.weight = nn.Parameter(w.to(DEV), requires_grad=False)
            setattr(self, f"linear{i + 1}", lin)

    def forward(self, x):
        return self.linear3(self.linear2(self.linear1(x)))


def sqnr(ref, y):
    ref, y = ref.float(), y.float()
    return (20 * torch.log10(torch.linalg.norm(ref) / torch.linalg.norm(ref - y))).item()


ACCURACY_BASES = {k: ROUTED[k] for k in ("dyn-row", "dyn-tensor", "dyn-row-wtensor", "dyn-tensor-wrow", "static-tensor", "static-tensor-wrow")}


@pytest.mark.parametrize("kind", list(ACCURACY_BASES))
def test_accuracy_on_the_toy_model(kind):
    """the reference's test_smoothquant_accuracy: loss_smoothquant < loss_base and SQNR > 20 dB, seeds 0 - 3, alpha 0.5 and 0.75"""
    base = ACCURACY_BASES[kind]
    for seed in range(4):
        x = C.toy_inputs(seed).to(DEV)
        weights = C.toy_weights(seed)
        ref = Toy(weights).eval()
        out_ref = ref(x)
        basic = Toy(weights).eval()
        if isinstance(base, Int8StaticActivationInt8WeightConfig):
            quantize_(basic, Int8DynamicActivationInt8WeightConfig(granularity=base.granularity))
        else:
            quantize_(basic, base)
        loss_base = F.mse_loss(basic(x), out_ref).item()
        for alpha in (0.5, 0.75):
            model = Toy(weights).eval()
            config = SmoothQuantConfig(base_config=base, step="prepare", alpha=alpha)
            quantize_(model, config)
            model(x)
            config.step = "convert"
            quantize_(model, config)
            assert model.linear1.weight.act_pre_scale is not None and model.linear2.weight.act_pre_scale is not None
            out = model(x)
            loss, db = F.mse_loss(out, out_ref).item(), sqnr(out_ref, out)
            print(f"{kind} seed {seed} alpha {alpha}: loss_smoothquant / loss_base = {loss / loss_base:.3f}, SQNR {db:.1f} dB")
            assert loss < loss_base, f"SmoothQuant loss ({loss:.6f}) should not be higher than basic loss ({loss_base:.6f})"
            assert db > 20.0


def two_pass_model(base, weights, x, alpha=0.5):
    model = Toy(weights).eval()
    quantize_(model, SmoothQuantConfig(base, step="prepare", alpha=alpha, use_running_absmax=True))
    model(x)
    quantize_(model, SmoothQuantConfig(base, step="prepare_for_smoothquant_smoothing_factor", alpha=alpha, use_running_absmax=True))
    quantize_(model, SmoothQuantConfig(base, step="prepare_for_smoothquant_activation_scales", alpha=alpha, use_running_absmax=True))
    model(x)
    assert model.linear1.obs._second_pass_count == 1 and model.linear1.obs.calibration_count == 1
    quantize_(model, SmoothQuantConfig(base, step="convert", alpha=alpha, use_running_absmax=True))
    return model


def test_two_pass_running_flow_through_quantize_steps():
    x, weights = C.toy_inputs(0).to(DEV), C.toy_weights(0)
    out_ref = Toy(weights).eval()(x)
    for kind in ("dyn-row", "static-tensor"):
        base = ROUTED[kind]
        model = two_pass_model(base, weights, x)
        one = Toy(weights).eval()
        quantize_(one, SmoothQuantConfig(base, step="prepare", alpha=0.5))
        one(x)
        quantize_(one, SmoothQuantConfig(base, step="convert", alpha=0.5))
        for name in ("linear1", "linear2", "linear3"):
            a, b = getattr(model, name).weight, getattr(one, name).weight
            assert torch.equal(a.qdata, b.qdata) and torch.equal(a.act_pre_scale, b.act_pre_scale) and torch.equal(a.scale, b.scale)
            if kind == "static-tensor":  # on bf16 activations both observers' scale is max(bf16(amax / 127.5), eps)
                assert a.act_quant_scale.shape == () and torch.equal(a.act_quant_scale.reshape(1, 1), b.act_quant_scale)
        assert sqnr(out_ref, model(x)) > 20.0
    # convert before the second pass: a static scale does not exist yet
    model = Toy(weights).eval()
    quantize_(model, SmoothQuantConfig(ROUTED["static-tensor"], step="prepare", use_running_absmax=True))
    model(x)
    with pytest.raises(RuntimeError, match="second calibration pass"):
        quantize_(model, SmoothQuantConfig(ROUTED["static-tensor"], step="convert", use_running_absmax=True))


@pytest.mark.parametrize("kind,running", [("dyn-row", False), ("static-tensor", False), ("static-tensor-wrow", True)])
def test_prepare_for_loading_then_load_state_dict_and_save_load(kind, running):
    base = ROUTED[kind]
    x, weights = C.toy_inputs(1).to(DEV), C.toy_weights(1)
    if running:
        model = two_pass_model(base, weights, x)
    else:
        model = Toy(weights).eval()
        quantize_(model, SmoothQuantConfig(base, step="prepare", alpha=0.5))
        model(x)
        quantize_(model, SmoothQuantConfig(base, step="convert", alpha=0.5))
    want = model(x)
    fresh = Toy([torch.zeros_like(w) for w in weights]).eval()
    quantize_(fresh, SmoothQuantConfig(base, step="prepare_for_loading", alpha=0.5, use_running_absmax=running))
    sd, fd = model.state_dict(), fresh.state_dict()
    assert list(sd) == list(fd)
    for k in sd:
        a, b = sd[k], fd[k]
        assert type(a) is type(b) and a.shape == b.shape and a.dtype == b.dtype
        for n in Int8Tensor.tensor_data_names + Int8Tensor.optional_tensor_data_names:
            ta, tb = getattr(a, n), getattr(b, n)
            assert (ta is None) == (tb is None), (k, n)
            if ta is not None:
                assert ta.shape == tb.shape and ta.dtype == tb.dtype, (k, n, ta.shape, tb.shape)
    assert torch.all(fresh.linear1.weight.act_pre_scale == 1)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh(x).view(torch.int16), want.view(torch.int16))
    buf = io.BytesIO()
    torch.save(model.state_dict(), buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=True)
    again = Toy([torch.zeros_like(w) for w in weights]).eval()
    quantize_(again, SmoothQuantConfig(base, step="prepare_for_loading", alpha=0.5, use_running_absmax=running))
    again.load_state_dict(loaded, assign=True)
    assert torch.equal(again(x).view(torch.int16), want.view(torch.int16))
