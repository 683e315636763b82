"""The four lookup tables of the low-bit optimizer states (csrc/quant_math.h "low-bit optimizer states").

  8-bit signed / unsigned  bitsandbytes' dynamic map (arXiv 1511.04561, 2110.02861): for exponent step i of E the decade 10^(i - E + 1) holds
                           the midpoints of a linspace(0.1, 1, .) with 2^i (signed: both signs) or 2^(i + 1) (unsigned) intervals; 0 and 1 close it
  4-bit signed             the same construction with E = 3 over 4 bits
  4-bit unsigned           linspace(0, 1, 17)[1:]: no zero, so a zero second moment decodes to 1/16 of its block's scale (arXiv 2309.01507)

The values are fp32 and their BITS are part of the state-dict format: tests/golden/optim.npz holds the reference's, and
tests/test_optim_host.py compares.  Every step is taken in the precision the published construction takes it in (fp32 linspace and
midpoints, the decade as a Python float times the fp32 midpoints), because a table built in float64 differs in the last bit of some entries.
The kernels hold no table: they read the `qmap` field of the state they are given.
"""
from functools import lru_cache

import torch

Q8_SIGNED, Q8_UNSIGNED, Q4_SIGNED, Q4_UNSIGNED, FP8, PLAIN = 0, 1, 2, 3, 4, 5
FORMAT_NAMES = {Q8_SIGNED: "Q8_SIGNED", Q8_UNSIGNED: "Q8_UNSIGNED", Q4_SIGNED: "Q4_SIGNED", Q4_UNSIGNED: "Q4_UNSIGNED", FP8: "FP8", PLAIN: "PLAIN"}
BLOCK_SIZES = (64, 128, 256, 512, 1024, 2048)


def _dynamic_map(signed: bool, exponent_steps: int, total_bits: int):
    """sorted Python floats, 2^total_bits of them (only the sizes whose every code is an exponent-step code: 8 bits / 7 steps, 4 bits / 3)"""
    width = total_bits - 1
    if width != exponent_steps:
        raise ValueError("the dynamic map is built here only where total_bits - 1 == exponent_steps")
    values = [0.0, 1.0]
    for i in range(exponent_steps):
        intervals = 2 ** i if signed else 2 ** (i + 1)
        edges = torch.linspace(0.1, 1, intervals + 1)
        mids = (edges[:-1] + edges[1:]) / 2.0
        decade = 10 ** (i - exponent_steps + 1)
        values += (decade * mids).tolist()
        if signed:
            values += (-decade * mids).tolist()
    if len(values) != 2 ** total_bits:
        raise AssertionError(f"{len(values)} table entries for {total_bits} bits")
    return sorted(values)


@lru_cache(maxsize=None)
def qmap_values(bits: int, signed: bool):
    """The table of one state format as a tuple of Python floats (each exactly an fp32)."""
    if bits == 8:
        return tuple(_dynamic_map(signed, 7, 8))
    if bits == 4:
        return tuple(_dynamic_map(True, 3, 4)) if signed else tuple(torch.linspace(0, 1, 17)[1:].tolist())
    raise ValueError(f"qmap_values: bits must be 8 or 4, got {bits}")


def make_qmap(bits: int, signed: bool, device=None) -> torch.Tensor:
    return torch.tensor(qmap_values(bits, signed), dtype=torch.float32, device=device)


def table_format(bits: int, signed: bool) -> int:
    return {(8, True): Q8_SIGNED, (8, False): Q8_UNSIGNED, (4, True): Q4_SIGNED, (4, False): Q4_UNSIGNED}[(bits, bool(signed))]
