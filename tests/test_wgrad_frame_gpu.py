"""GPU: the weight-gradient frame (ao_amd/csrc/wgrad_frame.h) means the same under every scaling policy.

One set of e4m3 codes drawn from {0, +-1, +-2, +-4}, every scale equal to one (E8M0 byte 127, reciprocal 1.0f): every fp32 partial sum is
an integer of at most 130 * 16, exact in any order and under any policy's chain.  So the MXFP8, the rowwise and the blockwise entries
must return the SAME bits, and those bits are the float64 sum over the group's tokens rounded once to bf16 -- the group range from offs,
the k steps on the global 128-token grid and the masks of a step's foreign tokens are the frame's, not a recipe's.

The shape is the hard case of test_mxfp8_grouped_bwd_gpu.py at the smallest shape the blockwise entries accept: M = 256, N = K = 128,
groups [1, 130, 125] -- a one-token group, boundaries off the 16-, 32- and 128-token grids, two groups sharing a k step.  Outputs go into
guarded, poisoned buffers (tests/_parity.py).
"""
import functools

import numpy as np
import pytest
import torch

import _parity
from ao_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
M, N, K = 256, 128, 128
SIZES = [1, 130, 125]
CODES = [0x00, 0x38, 0x40, 0x48, 0xB8, 0xC0, 0xC8]  # the table of test_mxfp8_grouped_bwd_gpu.py
VALUES = [0.0, 1.0, 2.0, 4.0, -1.0, -2.0, -4.0]


@functools.lru_cache(maxsize=None)
def case():
    """The operands on the device and the reference bits: grouped [E * N, K] and dense [N, K]."""
    g = torch.Generator().manual_seed(8128)
    ig, ix = torch.randint(0, 7, (N, M), generator=g), torch.randint(0, 7, (K, M), generator=g)
    codes, values = torch.tensor(CODES, dtype=torch.uint8), torch.tensor(VALUES, dtype=torch.float64)
    G, X = values[ig], values[ix]  # [N, M], [K, M]
    ends = np.cumsum(SIZES)
    # (+ 0.0: a sum starts from +0, so it is never -0; a one-token "matmul" is a bare product, and 0 x -1 is)
    ref = torch.cat([G[:, lo:hi] @ X[:, lo:hi].t() + 0.0 for lo, hi in zip([0, *ends[:-1]], ends)])
    assert float(ref.abs().max()) <= 130 * 16 and float((G @ X.t()).abs().max()) < 2 ** 24  # exact in fp32
    bits = lambda r: _parity.oracle_round(r, torch.bfloat16).view(torch.int16).to(DEV)  # noqa: E731
    dev = lambda t: t.to(DEV)  # noqa: E731
    return dict(g=dev(codes[ig]), x=dev(codes[ix]), offs=dev(torch.tensor(ends, dtype=torch.int32)),
                e8m0_n=dev(torch.full((M // 32, N), 127, dtype=torch.uint8)), e8m0_k=dev(torch.full((M // 32, K), 127, dtype=torch.uint8)),
                ones=dev(torch.ones(max(len(SIZES), M // 128) * max(N, K))),  # any [E][N], [E][K], [M/128][N] or [M/128][K] of 1.0f
                grouped=bits(ref), dense=bits(G @ X.t()))


def _run(entry, scales, E):
    """entry(g, g_scale, x, x_scale, [offs,] out, M, N, K, [E,] stream) into a guarded [E * N, K] buffer; offs and E only where E > 0."""
    c = case()
    buf = _parity.Guarded(max(E, 1) * N, K, torch.bfloat16, torch.device(DEV, 0))
    p = lambda t: t.data_ptr()  # noqa: E731
    head = (p(c["g"]), p(c[scales[0]]), p(c["x"]), p(c[scales[1]]))
    stream = torch.cuda.current_stream().cuda_stream
    fn = getattr(_lib.lib(), entry)
    if E > 0:
        _lib.check(fn(*head, p(c["offs"]), p(buf.out), M, N, K, E, stream))
    elif entry == "ao_fp8_grouped_mm_wgrad":  # the grouped entry without offs
        _lib.check(fn(*head, None, p(buf.out), M, N, K, 1, stream))
    else:
        _lib.check(fn(*head, p(buf.out), M, N, K, stream))
    torch.cuda.synchronize()
    assert not buf.guard_problems(), "%s: %s" % (entry, buf.guard_problems())
    return buf.bits()


GROUPED = {"ao_mxfp8_grouped_mm_wgrad": ("e8m0_n", "e8m0_k"), "ao_fp8_grouped_mm_wgrad": ("ones", "ones"),
           "ao_fp8_block_grouped_mm_wgrad": ("ones", "ones")}
DENSE = {"ao_mxfp8_mm_wgrad": ("e8m0_n", "e8m0_k"), "ao_fp8_block_mm_wgrad": ("ones", "ones"), "ao_fp8_grouped_mm_wgrad": ("ones", "ones")}


def _compare(got, want, what):
    for entry, bits in got.items():
        bad = torch.nonzero(bits != want)
        assert not len(bad), "%s (%s): %d elements differ from the float64 sum rounded once, the first at %s" % (entry, what, len(bad),
                                                                                                               bad[0].tolist())
    first = next(iter(got))
    for entry, bits in got.items():
        assert torch.equal(bits, got[first]), "%s and %s disagree (%s)" % (entry, first, what)


def test_the_three_grouped_entries_return_the_bits_of_the_float64_group_sums():
    got = {entry: _run(entry, scales, len(SIZES)) for entry, scales in GROUPED.items()}
    _compare(got, case()["grouped"], "groups %s" % SIZES)
    assert bool(got["ao_fp8_grouped_mm_wgrad"][:N].any()), "the one-token group's gradient is not all zero"


def test_without_offs_the_three_entries_return_the_bits_of_the_float64_sum_over_every_token():
    got = {entry: _run(entry, scales, 0) for entry, scales in DENSE.items()}
    _compare(got, case()["dense"], "one group of every token")
