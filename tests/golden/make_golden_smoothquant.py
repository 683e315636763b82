"""Generate tests/golden/smoothquant.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_smoothquant.py

Everything runs on the CPU.  For one bias-free linear (N = 16, K = 64, bf16), three calibration batches of 5, 7 and 200 rows and every alpha
of ALPHAS, the reference's own SmoothQuantConfig steps are driven through its quantize_ as they are:

  dyn      Int8DynamicActivationInt8WeightConfig()                          prepare, calibrate, convert (SmoothQuantObserver)
  static   Int8StaticActivationInt8WeightConfig(granularity=PerTensor())    prepare, calibrate, convert (SmoothQuantObserver)
  running  the same static config with use_running_absmax=True: prepare, calibrate, prepare_for_smoothquant_smoothing_factor, calibrate again.
           The reference's convert cannot finish this flow as it is: it hands the config's QuantizeTensorToInt8Kwargs to
           RunningAbsMaxSmoothQuantObserver.calculate_qparams, which reads it as a dict (core.py:287).  So the maker calls the observer's
           calculate_qparams with the dict of the reference's own test (test/prototype/test_smoothquant.py:529-533) and records its scale; the
           weight is the static flow's (the smoothing factor is asserted equal).
  The reference's symmetric static flows come with a zero-point of zeros (int8 [1, 1], int64 [1] from the running observer); the maker asserts
  that they are zero and records none: this backend stores a symmetric scale without a zero-point.

Per alpha a (key prefix a{i}_) the file holds sf_bits (the smoothing factor, bf16 bits), pre_bits (act_pre_scale), dyn_qdata / dyn_scale and
static_qdata / static_scale (the converted weights), static_act_scale and running_act_scale (fp32); once: W and the three inputs x0, x1, x2
(bf16 values as fp32), x_abs_max and w_abs_max (bf16 bits; the reference's expressions core.py:53-54 on the concatenated inputs), meta (JSON).

The maker asserts that tests/smoothquant_ref.py reproduces every recorded array byte for byte.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import smoothquant_cases as C  # noqa: E402
import smoothquant_ref as R  # noqa: E402
from oracle import bf16  # noqa: E402

from torchao.prototype.smoothquant import SmoothQuantConfig  # noqa: E402
from torchao.prototype.smoothquant.core import RunningAbsMaxSmoothQuantObserver, SmoothQuantObserver  # noqa: E402
from torchao.quantization import Int8DynamicActivationInt8WeightConfig, Int8StaticActivationInt8WeightConfig, quantize_  # noqa: E402
from torchao.quantization.granularity import PerTensor  # noqa: E402
from torchao.quantization.quantize_.common.quantization_step import QuantizationStep  # noqa: E402

N, K = 16, 64
BATCHES = (5, 7, 200)
ALPHAS = (None, 0.0, 0.25, 0.5, 0.75, 1.0)
RUNNING_KWARGS = {"quant_min": -128, "quant_max": 127, "qscheme": torch.per_tensor_symmetric}


def t16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)


def f32(t):
    return t.detach().to(torch.float32).contiguous().numpy().copy()


def bits(t):
    assert t.dtype == torch.bfloat16
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def model(W):
    m = torch.nn.Sequential(torch.nn.Linear(K, N, bias=False)).to(torch.bfloat16).eval()
    m[0].weight = torch.nn.Parameter(W.clone(), requires_grad=False)
    return m


def flow(W, xs, base_config, alpha, running=False):
    m = model(W)
    quantize_(m, SmoothQuantConfig(base_config=base_config, step=QuantizationStep.PREPARE, alpha=alpha, use_running_absmax=running))
    obs = m[0].obs
    assert isinstance(obs, RunningAbsMaxSmoothQuantObserver if running else SmoothQuantObserver)
    for x in xs:
        m(x)
    if running:
        quantize_(m, SmoothQuantConfig(base_config=base_config, step=QuantizationStep.PREPARE_FOR_SMOOTHQUANT_SMOOTHING_FACTOR, alpha=alpha,
                                       use_running_absmax=True))
        for x in xs:
            m(x)
        assert obs._second_pass_count == len(xs)
        return obs.calculate_qparams(RUNNING_KWARGS)
    sf = obs.calculate_qparams()[0]
    quantize_(m, SmoothQuantConfig(base_config=base_config, step=QuantizationStep.CONVERT, alpha=alpha))
    return sf, m[0].weight


def main():
    W = t16(C.weight(N, K, 20261021))
    xs = [t16(C.activation(b, K, 100 + i, scale=4.0, big=False)) for i, b in enumerate(BATCHES)]
    X = torch.cat(xs, dim=0)
    x_abs_max = torch.max(torch.abs(X), dim=0)[0]
    w_abs_max = torch.max(torch.abs(W), dim=0)[0]
    Wn, Xn = f32(W), [f32(x) for x in xs]
    want_x = R.col_absmax(Xn[2], R.col_absmax(Xn[1], R.col_absmax(Xn[0])))
    assert np.array_equal(bf16.to_bits(want_x), bits(x_abs_max)) and np.array_equal(bf16.to_bits(R.col_absmax(Wn)), bits(w_abs_max))
    assert (f32(w_abs_max) == 0).any(), "the fixture wants a weight column whose absmax is 0"

    out = dict(W=Wn, x0=Xn[0], x1=Xn[1], x2=Xn[2], x_abs_max=bits(x_abs_max), w_abs_max=bits(w_abs_max))
    for i, alpha in enumerate(ALPHAS):
        sf, qw = flow(W, xs, Int8DynamicActivationInt8WeightConfig(), alpha)
        sf_s, qw_s = flow(W, xs, Int8StaticActivationInt8WeightConfig(granularity=PerTensor()), alpha)
        sf_r, scale_r, zp_r = flow(W, xs, Int8StaticActivationInt8WeightConfig(granularity=PerTensor()), alpha, running=True)
        assert sf.dtype == torch.bfloat16 and torch.equal(sf, sf_s) and torch.equal(sf, sf_r)
        assert qw.act_quant_scale is None and torch.all(qw_s.act_quant_zero_point == 0) and torch.all(zp_r == 0)
        print(f"alpha {alpha}: static act scale {qw_s.act_quant_scale.dtype} {tuple(qw_s.act_quant_scale.shape)} "
              f"{qw_s.act_quant_scale.flatten().tolist()}, running {scale_r.dtype} {tuple(scale_r.shape)} {scale_r.flatten().tolist()}, "
              f"weight scale {qw.scale.dtype} {tuple(qw.scale.shape)}")

        # the restatement reproduces every one of them
        s = R.smoothing_factor(f32(x_abs_max), f32(w_abs_max), alpha)
        assert np.array_equal(bf16.to_bits(s), bits(sf)), f"alpha {alpha}: smoothing factor differs"
        pre = R.pre_scale(s)
        assert np.array_equal(bf16.to_bits(pre), bits(qw.act_pre_scale)) and torch.equal(qw.act_pre_scale, qw_s.act_pre_scale)
        q, sc = R.quantize_weight(R.smoothed_weight(Wn, s))
        assert np.array_equal(q, qw.qdata.numpy()) and np.array_equal(sc, f32(qw.scale).reshape(-1)), f"alpha {alpha}: weight differs"
        q, sc = R.quantize_weight(R.smoothed_weight(Wn, s), per_tensor=True)  # (the static config's PerTensor() is the weight's too)
        assert np.array_equal(q, qw_s.qdata.numpy()) and sc == f32(qw_s.scale).reshape(()), f"alpha {alpha}: PerTensor weight differs"
        amax = np.float32(0)
        for x in Xn:
            amax = R.smoothed_amax(x, s, amax)
        assert R.static_scale(amax) == f32(qw_s.act_quant_scale).reshape(()), f"alpha {alpha}: static activation scale differs"
        assert R.running_scale(amax) == f32(scale_r).reshape(()), f"alpha {alpha}: running activation scale differs"

        p = f"a{i}_"
        out.update({p + "sf_bits": bits(sf), p + "pre_bits": bits(qw.act_pre_scale), p + "dyn_qdata": qw.qdata.numpy().copy(),
                    p + "dyn_scale": f32(qw.scale), p + "static_qdata": qw_s.qdata.numpy().copy(), p + "static_scale": f32(qw_s.scale),
                    p + "static_act_scale": f32(qw_s.act_quant_scale), p + "running_act_scale": f32(scale_r)})
    out["meta"] = np.array(json.dumps({"N": N, "K": K, "batches": list(BATCHES), "alphas": list(ALPHAS)}))
    path = os.path.join(HERE, "smoothquant.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; tests/smoothquant_ref.py reproduces every byte")


if __name__ == "__main__":
    main()
