"""Model conversion for float8 training: the host mirror of torchao/float8/float8_linear_utils.py:20-130."""
from typing import Callable, Optional

import torch.nn as nn

from .config import Float8LinearConfig
from .float8_linear import Float8Linear, check_config

__all__ = ["swap_linear_layers", "convert_to_float8_training"]


def swap_linear_layers(module: nn.Module, from_float_func: Callable[[nn.Linear], nn.Linear], *,
                       module_filter_fn: Optional[Callable[[nn.Module, str], bool]] = None) -> nn.Module:
    """Replace every nn.Linear under `module` that `module_filter_fn(mod, fqn)` passes (None: all of them) by `from_float_func(mod)`
    (float8_linear_utils.py:20-83).  Children are visited before their parent.  A root-level nn.Linear cannot be replaced in place: its
    replacement is returned and `module` left as it was."""
    passes = lambda mod, fqn: isinstance(mod, nn.Linear) and (module_filter_fn is None or module_filter_fn(mod, fqn))  # noqa: E731
    if passes(module, ""):
        if len(list(module.children())) > 0:
            raise AssertionError(f"Does not support a root nn.Linear with children: {module}")
        return from_float_func(module)

    def visit(mod: nn.Module, fqn: str, parent: Optional[nn.Module]):
        for name, child in mod.named_children():
            visit(child, name if fqn == "" else f"{fqn}.{name}", mod)
        if passes(mod, fqn):
            assert parent is not None, f"Linear root module should return early: {mod}"
            setattr(parent, fqn.split(".")[-1], from_float_func(mod))

    visit(module, "", None)
    return module


def convert_to_float8_training(module: nn.Module, *, module_filter_fn: Optional[Callable[[nn.Module, str], bool]] = None,
                               config: Optional[Float8LinearConfig] = None) -> nn.Module:
    """Swap the nn.Linear modules of `module` for Float8Linear (float8_linear_utils.py:86-133); `module_filter_fn(mod, fqn)` chooses
    which, `config` how they train (None: Float8LinearConfig(), which this backend refuses for its e5m2 grad_output -- see
    float8_linear.check_config for the working alternatives).  Returns the converted module."""
    if config is None:
        config = Float8LinearConfig()
    check_config(config)
    return swap_linear_layers(module, lambda m: Float8Linear.from_float(m, config=config), module_filter_fn=module_filter_fn)
