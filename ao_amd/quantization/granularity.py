"""Quantization granularities (reference: torchao/quantization/granularity.py)."""
from dataclasses import dataclass


@dataclass(frozen=True)
class Granularity:
    pass


@dataclass(frozen=True)
class PerTensor(Granularity):
    pass


@dataclass(frozen=True)
class PerRow(Granularity):
    """One scale per row of the last-but-one... i.e. per output feature / per token."""
    dim: int = -1


@dataclass(frozen=True)
class PerGroup(Granularity):
    group_size: int = 128


@dataclass(frozen=True, eq=False)
class PerBlock(Granularity):
    """Multidimensional blocks (reference granularity.py:116-142): block_size [X, Y] on a tensor [A, B] gives scales [A // X, B // Y];
    tensors of higher rank keep one scale per leading index (get_block_size pads block_size with 1s on the left).  block_size may be
    given as a list or a tuple; the two compare and hash alike (by tuple(block_size)).  JSON writes it as a list -- upstream's own
    serialisation only works for lists (reference :138-141) -- see config._encode."""
    block_size: tuple = ()

    def __post_init__(self):
        bs = tuple(int(b) for b in self.block_size)
        if not bs or any(b < 1 for b in bs):
            raise ValueError(f"PerBlock: block_size must be a non-empty list of positive ints, got {self.block_size}")
        object.__setattr__(self, "block_size", bs)

    def __eq__(self, other):
        return isinstance(other, PerBlock) and tuple(self.block_size) == tuple(other.block_size)

    def __hash__(self):
        return hash(("PerBlock", tuple(self.block_size)))


def get_block_size(shape, granularity):
    """Block size for a granularity (reference: torchao/quantization/utils.py:589)."""
    if isinstance(granularity, PerTensor):
        return tuple(shape)
    if isinstance(granularity, PerRow):
        bs = [1] * len(shape)
        bs[granularity.dim] = shape[granularity.dim]
        return tuple(bs)
    if isinstance(granularity, PerGroup):
        assert shape[-1] % granularity.group_size == 0
        return tuple([1] * (len(shape) - 1) + [granularity.group_size])
    if isinstance(granularity, PerBlock):  # reference utils.py:603-621
        bs = (1,) * (len(shape) - len(granularity.block_size)) + tuple(granularity.block_size)
        assert len(bs) == len(shape), f"Block size {bs} must have the same number of dimensions as input shape {tuple(shape)}"
        for i in range(len(bs)):
            assert shape[i] % bs[i] == 0, f"Not all shapes in input shape {tuple(shape)} are divisible by block size {bs}"
        return bs
    raise ValueError(f"Unsupported Granularity: {granularity}")


import torch as _torch  # noqa: E402

# granularities ride along in the quantized tensors' attributes: allow them under torch.load(weights_only=True)
_torch.serialization.add_safe_globals([Granularity, PerTensor, PerRow, PerGroup, PerBlock])
