"""AWQ (torchao/prototype/awq): Gram-matrix observer, fused scale search, AWQConfig."""
from .api import AWQConfig  # noqa: F401
from .core import AWQObservedLinear, AWQObserver  # noqa: F401

__all__ = ["AWQConfig", "AWQObserver", "AWQObservedLinear"]
