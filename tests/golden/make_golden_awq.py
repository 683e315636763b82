"""Generate tests/golden/awq.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_awq.py

Everything runs on the CPU.  The reference's AWQObserver (prototype/awq/core.py) is driven as it is: forward() on a few batches, then
calculate_qparams().  Its base config's handler cannot run here -- Int4WeightOnlyConfig's needs the un-vendored mslk package and a GPU -- so
this maker registers a stand-in config with the reference's handler registry.  Its handler applies the PLAIN int4 formula that
include/ao_mi355.h states for ao_int4_plain_quantize (the one make_golden_gptq.py uses for the group qparams), in fp32 torch ops, stores the
qparams as bf16 and returns the dequantized bf16 weight q.to(bf16) * scale + zero_point (PARITY UNPINNED, as in oracle/int4_plain_ref.py);
and it records what it is handed and what it returns.

The file holds, for one linear (N = 8, K = 128, g = 32, R = 20, 200 calibration rows in three batches):
  W, X              the weight and the concatenated inputs (bf16 values as fp32)
  x_mean            the reference's get_act_scale of the concatenated inputs (bf16 as fp32)
  S                 [R, K]: the scale table, made from x_mean with the tensor ops of core.py:71-76 as the issue of this feature states them;
                    pinned to the reference by the two assertions below
  ws_bits, dq_bits  [R, N, K] uint16: the bf16 bits of every scaled weight the handler received and of every weight it returned
  best_scales       what the reference's calculate_qparams returned;  best_index: the row of S it equals
  meta              JSON: N, K, g, R, the batch sizes

The maker asserts that bf16(W * S[r]) is the r-th weight the reference handed over, that the reference's best_scales is a row of S, and
that tests/awq_ref.py reproduces every recorded scaled weight and dequantized weight byte for byte.
"""
import json
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import awq_ref as R  # noqa: E402
from oracle import bf16  # noqa: E402

from torchao.core.config import AOBaseConfig  # noqa: E402
from torchao.prototype.awq.core import AWQObserver, get_act_scale  # noqa: E402
from torchao.quantization.transform_module import register_quantize_module_handler  # noqa: E402

N, K, G, NR = 8, 128, 32, 20
BATCHES = (64, 100, 36)
RECORD = {"ws": [], "dq": []}


@dataclass
class PlainInt4StandIn(AOBaseConfig):
    group_size: int = G


@register_quantize_module_handler(PlainInt4StandIn)
def _plain_int4_stand_in(module, config):
    w = module.weight.detach()
    assert w.dtype == torch.bfloat16
    g = config.group_size
    x = w.to(torch.float32).reshape(w.shape[0], -1, g)
    mx, mn = x.amax(dim=2, keepdim=True), x.amin(dim=2, keepdim=True)
    scale = torch.clamp(mx - mn, min=1e-6) / 15
    zero = mn + scale * 8
    q = torch.clamp(torch.round((x - mn) / scale), 0, 15) - 8
    dq = (q.to(torch.bfloat16) * scale.to(torch.bfloat16) + zero.to(torch.bfloat16)).reshape(w.shape)
    assert dq.dtype == torch.bfloat16
    RECORD["ws"].append(w.clone())
    RECORD["dq"].append(dq.clone())
    module.weight = torch.nn.Parameter(dq, requires_grad=False)
    return module


def f32(t):
    return t.detach().to(torch.float32).contiguous().numpy().copy()


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def main():
    gen = torch.Generator().manual_seed(20261021)
    W = (torch.randn(N, K, generator=gen) * 0.05).to(torch.bfloat16)
    W[2, 32:64] = 0.0        # an all-zero group
    W[3, 64:96] = 0.03125    # an all-equal group: the 1e-6 clamp
    mag = torch.exp(torch.randn(K, generator=gen))
    xs = [(torch.randn(b, K, generator=gen) * mag).to(torch.bfloat16) for b in BATCHES]

    obs = AWQObserver(W, None, PlainInt4StandIn(), NR)
    for x in xs:
        obs(x, None)
    best = obs.calculate_qparams()
    assert len(RECORD["ws"]) == NR

    X = torch.cat(xs, dim=-2)
    x_mean = get_act_scale(X)
    rows = []
    for i in range(NR):
        s = x_mean.pow(i / NR).to(torch.bfloat16).clamp(min=1e-4)
        rows.append(s / (s.max() * s.min()).sqrt())
    S = torch.stack(rows)
    assert S.dtype == torch.bfloat16 and torch.all(S[0] == 1)
    for r in range(NR):
        assert torch.equal(W * S[r], RECORD["ws"][r]), r
    hits = [r for r in range(NR) if torch.equal(S[r], best)]
    assert hits, "the reference's best_scales is not a row of the table"

    ws_bits, dq_bits = np.stack([bits(t) for t in RECORD["ws"]]), np.stack([bits(t) for t in RECORD["dq"]])
    got = R.chain(f32(W), f32(S), G)
    assert np.array_equal(bf16.to_bits(got["ws"]), ws_bits), "tests/awq_ref.py: scaled weights differ"
    assert np.array_equal(bf16.to_bits(got["dq"]), dq_bits), "tests/awq_ref.py: dequantized weights differ"
    assert (got["scale"] == np.float32(1e-6) / np.float32(15)).sum() == NR + 1  # the clamp: the zero group under every ratio, the all-equal group under ratio 0

    out = dict(W=f32(W), X=f32(X), x_mean=f32(x_mean), S=f32(S), ws_bits=ws_bits, dq_bits=dq_bits, best_scales=f32(best),
               best_index=np.array(hits[0]), meta=np.array(json.dumps({"N": N, "K": K, "g": G, "R": NR, "batches": list(BATCHES)})))
    path = os.path.join(HERE, "awq.npz")
    np.savez_compressed(path, **out)
    l64 = R.losses64(f32(W), f32(S), G, f32(X))
    print(f"wrote {path}: {os.path.getsize(path)} bytes; the reference picked ratio {hits[0]} / {NR}, float64 argmin {int(np.argmin(l64))}; "
          "tests/awq_ref.py reproduces every byte")


if __name__ == "__main__":
    main()
