"""Generate tests/golden/nvfp4_training.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_nvfp4_training.py

Everything runs on the CPU, from the reference's own test/prototype/moe_training/nvfp4_training/nvfp4_reference.py (loaded by its path next
to the imported torchao package) with layout="plain": reference_rht_amax, reference_rht_quantize_row_col, reference_weight_quantize_2d.
bf16 tensors are stored as uint16 bit patterns, codes and e4m3 scales as uint8, amaxes as fp32.

  act_*    a seeded 144 x 80 activation whose 16-row runs sit on per-run magnitudes 2^-6 .. 2^6 (8-bit integers times the run's power of
           two): amaxes, column and row codes and scales, both directions of the 16 x 16 cast
  edge_*   16-element blocks, each replicated down a run of 16 rows (so a column run holds one magnitude): zeros, -0.0, every e2m1 tie
           and its bf16 neighbours under an encode scale of exactly 1, block amaxes around the points where the e4m3 scale rounds, a block
           whose scale underflows to byte 0, the block that holds the tensor's amax (scale 448).  The tensor's amax is 42 = 2688 / 64.
  zero_*   an all-zero 16 x 32 tensor (amax 0: S_enc = 1)
  w_*      a seeded 48 x 80 weight: both directions of the 16 x 16 cast
  lin*_*   the operands of the linear tests -- lin0: the activation and the weight above, a seeded gradient and bias; lin1: seeded
           (M, K, N) = (256, 128, 128) -- and, measured on the CPU restatement (tests/nvfp4_train_ref.py) under the stored seed and
           offsets, the SQNR in dB of out, grad_input and grad_weight against the fp32 matmuls
The fp32 Hadamard sums of act and edge are asserted exact (float64 against fp32), so bitwise parity is fair for any summation order.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
# the offsets are the two torch.randint(0, 2 ** 32) draws of an MI355X's default generator after torch.manual_seed(11), which is what the
# backward of the GPU test draws: the stored SQNR and the measured one then round with the same bits
SR_SEED, COL_OFFSET, ROW_OFFSET = 0x5EED5EED12345678, 4117957564, 2978150339


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def bf(v):
    return torch.tensor(v, dtype=torch.float32).to(torch.bfloat16)


def nextafter_bf16(t, up):
    b = t.view(torch.int16).to(torch.int32)
    step = torch.where((t.float() >= 0) == up, 1, -1)
    return (b + step).to(torch.int16).view(torch.bfloat16)


def load_reference():
    import torchao

    root = os.path.dirname(os.path.dirname(os.path.abspath(torchao.__file__)))
    path = os.path.join(root, "test", "prototype", "moe_training", "nvfp4_training", "nvfp4_reference.py")
    spec = importlib.util.spec_from_file_location("nvfp4_reference", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["nvfp4_reference"] = mod
    spec.loader.exec_module(mod)
    return mod


def activation(g):
    ints = torch.randint(-127, 128, (144, 80), generator=g).to(torch.float32)
    exps = torch.tensor([-6, -4, -3, -1, 0, 1, 3, 4, 6], dtype=torch.float32) - 7  # |x| < 2^e of the run
    return (ints * torch.exp2(exps).repeat_interleave(16).reshape(144, 1)).to(torch.bfloat16)


def edge_matrix():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    t = bf([v for x in ties for v in (x, -x)] + [6.0, -6.0])  # block amax 6 under S_enc = 64: scale 64, enc = 1
    blocks = [torch.zeros(16, dtype=torch.bfloat16), -torch.zeros(16, dtype=torch.bfloat16), t]
    for up in (False, True):
        n = nextafter_bf16(t, up)
        n[14], n[15] = 6.0, -6.0
        blocks.append(n)
    filler = bf([0.5, -1.0, 1.5, -2.0, 3.0, -0.25, 0.75, 0.0, -0.0, 1.25, -1.75, 2.5, -3.5, 4.0, 5.0])
    # scale = amax (64 f32(1/6)) around the e4m3 ties 1.0625 (to even 1) and 1.1875 (to even 1.25), the subnormal tie 2^-9 1.5 and the
    # underflow point 2^-10; 42 is the tensor's amax (scale 448); 2^-20 underflows to byte 0
    for amax in (0.099609375, 0.111328125, 0.00027465820, 0.0000915527):
        for v in (nextafter_bf16(bf([amax]), False), bf([amax]), nextafter_bf16(bf([amax]), True)):
            blocks.append(torch.cat([v, (filler * (float(v) / 8)).to(torch.bfloat16)]))
    for amax in (42.0, 41.75, 2.0 ** -20, 3.0):
        blocks.append(torch.cat([bf([amax]), (filler * (amax / 8)).to(torch.bfloat16)]))
    rows = torch.stack(blocks)                       # [B, 16]
    sign = torch.where(torch.arange(16) % 3 == 0, -1.0, 1.0).reshape(1, 16, 1)
    return (rows.float().reshape(-1, 1, 16) * sign).to(torch.bfloat16).reshape(-1, 16)   # [16 B, 16]: a run = one block, signs varied


def assert_exact_hadamard(ref, name, x):
    from torchao.prototype.moe_training.nvfp4_training.hadamard_utils import get_rht_matrix

    m, n = x.shape
    B = get_rht_matrix(tuple(ref.DEFAULT_SIGN_VECTOR), "cpu", torch.bfloat16, 16)
    runs = x.t().reshape(-1, 16)
    s64 = runs.double() @ B.double()
    s32 = runs.float() @ B.float()
    assert torch.equal(s32.double(), s64), f"{name}: the fp32 Hadamard sums are not exact"
    assert torch.equal(ref.reference_rht(x).view(torch.int16), s64.float().to(torch.bfloat16).reshape(n, m).view(torch.int16)), name


def record_casts(ref, out, name, x):
    col_amax, row_amax = ref.reference_rht_amax(x)
    out[f"{name}_x"] = bits(x)
    out[f"{name}_amax2"] = torch.stack([col_amax, row_amax]).to(torch.float32).numpy().copy()
    col, row = ref.reference_rht_quantize_row_col(x, col_amax, row_amax, layout="plain")
    for tag, o in (("col", col), ("row", row)):
        out[f"{name}_{tag}_q"] = o.codes.view(torch.uint8).numpy().copy()
        out[f"{name}_{tag}_s"] = o.scales.view(torch.uint8).numpy().copy()


def record_weight(ref, out, name, w):
    amax = w.float().abs().max()
    out[f"{name}_x"] = bits(w)
    out[f"{name}_amax"] = amax.to(torch.float32).numpy().copy()
    rowwise, colwise = ref.reference_weight_quantize_2d(w, amax, layout="plain")
    for tag, o in (("w2d", rowwise), ("w2dt", colwise)):
        out[f"{name}_{tag}_q"] = o.codes.view(torch.uint8).numpy().copy()
        out[f"{name}_{tag}_s"] = o.scales.view(torch.uint8).numpy().copy()


def main():
    ref = load_reference()
    import nvfp4_train_ref as T

    assert tuple(ref.DEFAULT_SIGN_VECTOR) == T.DEFAULT_SIGN_VECTOR
    g = torch.Generator().manual_seed(0)
    out = {"sr_seed": np.int64(np.uint64(SR_SEED).astype(np.int64)), "col_offset": np.int64(COL_OFFSET), "row_offset": np.int64(ROW_OFFSET)}
    act, edge, zero = activation(g), edge_matrix(), torch.zeros(16, 32, dtype=torch.bfloat16)
    w = (torch.randn(48, 80, generator=g) * 0.05).to(torch.bfloat16)
    for name, x in (("act", act), ("edge", edge), ("zero", zero)):
        assert_exact_hadamard(ref, name, x)
        record_casts(ref, out, name, x)
        record_weight(ref, out, name, x)
    record_weight(ref, out, "w", w)
    # the linears: operands and the restatement's SQNR against the fp32 matmuls
    lins = {"lin0": (act, w, (torch.randn(144, 48, generator=g) * 0.02).to(torch.bfloat16)),
            "lin1": ((torch.randn(256, 128, generator=g)).to(torch.bfloat16), (torch.randn(128, 128, generator=g) * 0.05).to(torch.bfloat16),
                     (torch.randn(256, 128, generator=g) * 0.02).to(torch.bfloat16))}
    for name, (x, wt, dy) in lins.items():
        out[f"{name}_x"], out[f"{name}_w"], out[f"{name}_dy"] = bits(x), bits(wt), bits(dy)
        bias = (torch.randn(wt.shape[0], generator=g) * 0.1).to(torch.bfloat16)
        out[f"{name}_bias"] = bits(bias)
        sums = T.linear_sums(x, wt, dy, T.DEFAULT_SIGN_VECTOR, SR_SEED, COL_OFFSET, ROW_OFFSET)
        want = T.fp32_linear(x, wt, dy)
        got = {k: sums[k][0].float().to(torch.bfloat16) for k in sums}
        # [out, grad_input, grad_weight, out with the bias added in bf16 after the GEMM]
        out[f"{name}_sqnr"] = np.array([T.sqnr_db(got[k], want[k]) for k in ("out", "grad_input", "grad_weight")]
                                       + [T.sqnr_db(got["out"] + bias, want["out"] + bias.float())], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "nvfp4_training.npz"), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})
    print({k: out[k] for k in out if k.endswith("_sqnr")})


if __name__ == "__main__":
    main()
