"""The monkey-patch wrapper (mirrors torchao/prototype/attention/shared_utils/wrapper.py)."""
from typing import Callable

import torch.nn as nn
import torch.nn.functional as F


class _LowPrecisionAttentionWrapper(nn.Module):
    """Base wrapper.  Proxies attribute access to the original module."""

    def __init__(self, orig_mod: nn.Module):
        super().__init__()
        self._orig_mod = orig_mod

    def __getattr__(self, name: str):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self._orig_mod, name)


class _FP8AttentionMonkeyPatchWrapper(_LowPrecisionAttentionWrapper):
    """Replaces F.scaled_dot_product_attention by the FP8 path for the duration of each forward call, and restores it whatever happens."""

    def __init__(self, orig_mod: nn.Module, sdpa_patch_fn: Callable):
        super().__init__(orig_mod)
        self._sdpa_patch_fn = sdpa_patch_fn

    def forward(self, *args, **kwargs):
        original_sdpa = F.scaled_dot_product_attention
        F.scaled_dot_product_attention = self._sdpa_patch_fn
        try:
            return self._orig_mod(*args, **kwargs)
        finally:
            F.scaled_dot_product_attention = original_sdpa
