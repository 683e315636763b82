"""Disassembly guard for the balanced grid of the one-row int4 kernel (no GPU).  The balanced build must leave a block's work alone:
its whole-tile path still holds the 16 block-level v_mfma_f32_16x16x32_bf16 (4 blocks x 4 words) in one straight run -- no branch, no
barrier -- with the same instruction mix of the dequant and no more s_waitcnt than the build it replaces on those shapes."""
import re

import pytest

from test_isa_structure import _device_disassembly

MFMA = "v_mfma_f32_16x16x32_bf16"
SYMBOL = "_ZN2ao12_GLOBAL__N_114int4_mm_kernelILi{g}ELi1ELi4ELb1ELb{bal}ELb0EEE"  # <G, 1 row, 4 blocks, straight-line, BAL, no stamps>


def _function(asm, prefix):
    m = re.search(r"^[0-9a-f]+ <(" + re.escape(prefix) + r"[^>]*)>:$", asm, flags=re.M)
    assert m, f"{prefix} not found in the library's disassembly"
    end = re.compile(r"^[0-9a-f]+ <[^>]*>:$", flags=re.M).search(asm, m.end())
    ops = []
    for line in asm[m.end(): end.start() if end else len(asm)].split("\n"):
        line = line.split("//")[0].strip()
        if line and not line.endswith(":"):
            ops.append(line)
    return ops


def _body(ops):
    """From the first block-level MFMA to the last."""
    at = [i for i, l in enumerate(ops) if l.startswith(MFMA)]
    return ops[at[0]: at[-1] + 1], len(at)


@pytest.mark.parametrize("g", [32, 64, 128, 256])
def test_balanced_build_keeps_the_block_body(tmp_path, g):
    asm = _device_disassembly(tmp_path)
    whole_fn, bal_fn = _function(asm, SYMBOL.format(g=g, bal=0)), _function(asm, SYMBOL.format(g=g, bal=1))
    whole, n_whole = _body(whole_fn)
    bal, n_bal = _body(bal_fn)
    assert n_whole == 16 and n_bal == 16, (n_whole, n_bal)
    for name, body in (("whole-tile build", whole), ("balanced build", bal)):
        flow = [l for l in body if l.startswith(("s_cbranch", "s_branch", "s_barrier", "s_endpgm"))]
        assert not flow, f"{name}: control flow inside the four blocks: {flow}"
    count = lambda body, op: sum(1 for l in body if l.split()[0].startswith(op))  # noqa: E731
    assert count(bal, "s_waitcnt") <= count(whole, "s_waitcnt"), "the balanced build waits more often inside the blocks"
    # the dequant's conversions, its matrix-pipe adds and the operand reads belong to the blocks alone (the scheduler may lift the first
    # word's ahead of the first MFMA, so they are counted over the kernel): the same counts in both builds.  (The compiler splits one
    # packed multiply-add into scalar ones in some builds and not in others: v_pk_fma_f32 is not pinned.)
    for op in ("v_mfma_f32_4x4x4", "v_cvt_scalef32_pk_f32_fp8", "ds_read_b128", "buffer_load_dwordx4"):
        assert count(bal_fn, op) == count(whole_fn, op), f"{op}: {count(bal_fn, op)} in the balanced build, {count(whole_fn, op)} in the whole-tile build"
    assert count(bal_fn, "v_cvt_pk_bf16_f32") == count(whole_fn, "v_cvt_pk_bf16_f32") + 1, "the two roundings per weight pair, and one more epilogue"
    assert len(bal) <= len(whole) + 4, (len(bal), len(whole))
