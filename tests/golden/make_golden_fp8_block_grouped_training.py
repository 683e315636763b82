"""Generate tests/golden/fp8_block_grouped_training.npz by importing the REFERENCE (torchao) in the build container.  Run once, commit
the file:

    PYTHONPATH=<reference torchao tree> python tests/golden/make_golden_fp8_block_grouped_training.py

Everything runs on the CPU.  The reference's Function (prototype/moe_training/blockwise_fp8/grouped_mm.py:98-265) calls Triton casts, which
do not run there, so the recorder composes the reference's own torch functions in the Function's order, under KernelPreference.EMULATED:
  torch_pad_token_groups / torch_unpad_token_groups (moe_training/kernels/mxfp8/quant.py:368-490), alignment 128
  torch_blockwise_scale_act_quant_lhs on A and grad_out, torch_blockwise_scale_act_quant_rhs on both (the wgrad's operands)
  torch_blockwise_scale_weight_quant per expert on w[e] and on w[e].t() (the forward's and the dgrad's B)
  _emulated_blockwise_scaled_grouped_mm_impl (blockwise_fp8_training/grouped_kernels.py:78-93) for all three GEMMs, with the operand
  layouts of _EmulatedGroupedMMBackend (grouped_mm_backend.py:93-194): it rounds both dequantized operands to bf16 and calls
  torch._grouped_mm
on the reference test's two cases (test/prototype/moe_training/test_fp8_blockwise_grouped_mm.py:37-43), K = N = 256:
  aligned   offs = [256, 512], no padding          padded   offs = [129, 384, 500], groups padded to 128 tokens

At these shapes the tensors of one case alone (three operands, eight casts, three results) are several MiB of incompressible bytes, far
more than a committed file may hold.  So the file records what cannot be made again without the reference, and pins the rest:
  <c>_offs
  <c>_<t>_sha             SHA-256 of the bf16 bits of t in a, w, go -- the operands, which tests/fp8_block_grouped_training_ref.operands
                          generates (numpy's frozen legacy generator)
  <c>_<cast>_q_sha        SHA-256 of the codes of every cast the Function makes: a_row, go_row [Mp, C]; a_col, go_col stored transposed
                          [C, Mp]; w [E, N, K]; w_t [E, K, N]
  <c>_<cast>_inv          its reciprocal scales, in full (fp32)
  <c>_<r>_ref_sqnr        r in out, grad_a, grad_w: SQNR (dB) of the reference's result against the float64 product of the recorded
                          dequantized casts (the helper's function_f64), over the whole tensor
  <c>_<r>_energy          the sum of squares of that float64 product (so that a test can tell its own product is the recorder's)
  <c>_<r>_sample          every 8th row of the reference's result (bf16 bits; grad_w: every 8th row of every expert)
The recorder asserts that the helper's numpy casts and padding reproduce the reference's bytes, that cast(w[e].t()) is the transposed
cast of w[e], and that all codes are finite.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fp8_block_grouped_training.npz")
CASTS = ("a_row", "go_row", "a_col", "go_col", "w", "w_t")
RESULTS = ("out", "grad_a", "grad_w")


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def from_bits(b):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).view(torch.bfloat16)


def load(path=PATH):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import fp8_block_grouped_training_ref as G
    from torchao.prototype.blockwise_fp8_training.grouped_kernels import _emulated_blockwise_scaled_grouped_mm_impl as emulated
    from torchao.prototype.blockwise_fp8_training.kernels import (
        BLOCKWISE_1X128_SCALING_TYPE,
        BLOCKWISE_128X128_SCALING_TYPE,
        _scaling_type_value,
        torch_blockwise_scale_act_quant_lhs,
        torch_blockwise_scale_act_quant_rhs,
        torch_blockwise_scale_weight_quant,
    )
    from torchao.prototype.moe_training.kernels.mxfp8.quant import torch_pad_token_groups, torch_unpad_token_groups

    r1, r128 = _scaling_type_value(BLOCKWISE_1X128_SCALING_TYPE), _scaling_type_value(BLOCKWISE_128X128_SCALING_TYPE)
    bf = torch.bfloat16
    out = {}
    for case, spec in G.CASES.items():
        ab, wb, gob = G.operands(case)
        a, w, go = from_bits(ab), from_bits(wb), from_bits(gob)
        offs = torch.tensor(spec["offs"], dtype=torch.int32)
        M, E = a.shape[0], w.shape[0]
        if spec["pad"]:
            a_p, starts, ends = torch_pad_token_groups(a, offs, 128)
            go_p, _, _ = torch_pad_token_groups(go, offs, 128)
        else:
            a_p, go_p, starts, ends = a, go, None, offs
        want, w_starts, w_ends = G.function_casts(ab, wb, gob, spec["offs"], spec["pad"])
        assert np.array_equal(ends.numpy(), w_ends) and (starts is None or np.array_equal(starts.numpy(), w_starts))
        assert a_p.shape[0] % 128 == 0 and (not spec["pad"] or np.array_equal(bits(a_p), G.pad_groups(ab, spec["offs"])[0]))

        # the casts, in the Function's order
        a_q, a_inv = torch_blockwise_scale_act_quant_lhs(a_p.contiguous())
        wq = [torch_blockwise_scale_weight_quant(w[e].contiguous()) for e in range(E)]
        w_q, w_inv = torch.stack([q for q, _ in wq]), torch.stack([s for _, s in wq])                    # [E, N, K], [E, N/128, K/128]
        go_q, go_inv = torch_blockwise_scale_act_quant_lhs(go_p.contiguous())
        wtq = [torch_blockwise_scale_weight_quant(w[e].t().contiguous()) for e in range(E)]
        wt_q, wt_inv = torch.stack([q for q, _ in wtq]), torch.stack([s for _, s in wtq])                # [E, K, N], [E, K/128, N/128]
        goc_q, goc_inv = torch_blockwise_scale_act_quant_rhs(go_p.contiguous())                          # [Mp, N], [Mp/128, N]
        ac_q, ac_inv = torch_blockwise_scale_act_quant_rhs(a_p.contiguous())                             # [Mp, K], [Mp/128, K]
        got = {"a_row": (a_q, a_inv), "go_row": (go_q, go_inv), "a_col": (ac_q.t(), ac_inv), "go_col": (goc_q.t(), goc_inv),
               "w": (w_q, w_inv), "w_t": (wt_q, wt_inv)}
        for name in CASTS:
            q = got[name][0].contiguous().view(torch.uint8).numpy()
            inv = got[name][1].contiguous().to(torch.float32).numpy()
            assert not np.any((q & 0x7F) == 0x7F), "a non-finite code in " + name
            assert np.array_equal(q, want[name][0]), "the numpy restatement misses the reference's codes of " + name
            assert np.array_equal(inv.view(np.uint32), want[name][1].view(np.uint32)), "... the reciprocal scales of " + name
            out["%s_%s_q_sha" % (case, name)], out["%s_%s_inv" % (case, name)] = G.sha(q), inv.copy()

        # the three GEMMs, with the layouts of _EmulatedGroupedMMBackend
        y = emulated(a_q, w_q.transpose(-2, -1), a_inv, r1, w_inv.transpose(-2, -1), r128, ends, bf, 128)          # [Mp, N]
        ga = emulated(go_q, wt_q.transpose(-2, -1), go_inv, r1, wt_inv.transpose(-2, -1), r128, ends, bf, 128)      # [Mp, K]
        gw = emulated(goc_q.t().contiguous(), ac_q, goc_inv.t(), r1, ac_inv, r1, ends, bf, 128)                     # [E, N, K]
        if spec["pad"]:
            y = torch_unpad_token_groups(y, offs, starts, M, 128)
            ga = torch_unpad_token_groups(ga, offs, starts, M, 128)
        assert tuple(y.shape) == (M, G.N_FIX) and tuple(ga.shape) == (M, G.K_FIX) and tuple(gw.shape) == (E, G.N_FIX, G.K_FIX)
        ref64 = G.function_f64(want, spec["offs"], w_starts, w_ends, M)
        out[case + "_offs"] = offs.numpy().copy()
        for t, b in (("a", ab), ("w", wb), ("go", gob)):
            out["%s_%s_sha" % (case, t)] = G.sha(b)
        for name, t, r in zip(RESULTS, (y, ga, gw), ref64):
            s = G.sqnr(t.double().numpy(), r)
            out["%s_%s_ref_sqnr" % (case, name)] = np.float64(s)
            out["%s_%s_energy" % (case, name)] = np.float64(np.sum(r ** 2))
            out["%s_%s_sample" % (case, name)] = G.sample(bits(t))
            print("%s %s: the reference's emulation against the float64 product of its casts: %.2f dB" % (case, name, s))
    np.savez_compressed(PATH, **out)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
