"""Adam / AdamW with block-quantized moments: the classes, signatures and defaults of torchao/optim/adam.py, the step of one parameter in
ONE launch (ops.optim_adam_step, csrc/optim_kernels.hip) where the reference compiles single_param_adam through Triton.  The bytes are those
of the reference's eager CPU run (csrc/quant_math.h "low-bit optimizer states"); stochastic rounding is this library's own Philox stream.

Not built, refused by name: DTensor / FSDP2 parameters, CPUOffloadOptimizer, fp16 parameters, a gradient dtype other than the parameter's,
sparse gradients, and step() under hipGraph capture (the step's scalars go to the kernel by value and change every step).
"""
import torch
from torch import Tensor
from torch.optim import Optimizer

from .. import ops
from .quant_utils import FP8, PLAIN, Q4_SIGNED, Q8_SIGNED
from .subclass_4bit import OptimState4bit
from .subclass_8bit import OptimState8bit
from .subclass_fp8 import OptimStateFp8

__all__ = ["Adam8bit", "Adam4bit", "AdamFp8", "AdamW8bit", "AdamW4bit", "AdamWFp8", "_AdamW", "step_scalars"]


def step_scalars(lr: Tensor, beta1: float, beta2: float, weight_decay: float, eps: float, step: Tensor):
    """The eight fp32 scalars of one step (ops.OPTIM_SCALARS) as Python floats, by the torch CPU operations single_param_adam runs on its
    0-dim tensors (adam.py:182-204): lr and step are 0-dim CPU fp32 tensors, the rest Python numbers -- pow and the roundings of the
    Python doubles are torch's own, so the bits are the reference's by construction.  The one sqrt is taken in float64 and rounded to fp32,
    which is the correctly rounded fp32 root on any machine (ATen's CPU sqrt is MKL's and need not be: quant_math.h)."""
    lr = lr.detach().to(device="cpu", dtype=torch.float32).reshape(())
    step = step.detach().to(device="cpu", dtype=torch.float32).reshape(())
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    vals = (lr, lr * weight_decay, f32(weight_decay), f32(1 - beta1), f32(1 - beta2), bias_correction1, bias_correction2.double().sqrt().float(), f32(eps))
    return [float(v) for v in vals]


def _is_dtensor(t) -> bool:
    try:
        from torch.distributed.tensor import DTensor
    except ImportError:  # a torch built without distributed
        return False
    return isinstance(t, DTensor)


class _AdamBase(Optimizer):
    def __init__(self, params, lr, betas, eps, weight_decay, amsgrad, *, block_size, bf16_stochastic_round, is_adamw, sr_seed=None) -> None:
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if block_size is not None and block_size not in ops.OPTIM_BLOCK_SIZES:
            raise ValueError(f"{type(self).__name__}: block_size must be a power of two from 64 to 2048, got {block_size}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults)
        self.block_size = block_size
        self.bf16_stochastic_round = bf16_stochastic_round
        self.is_adamw = is_adamw
        self.sr_seed = torch.initial_seed() if sr_seed is None else int(sr_seed)  # (an attribute: not part of state_dict)

    def add_param_group(self, param_group: dict) -> None:
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        for p in group["params"]:
            if _is_dtensor(p):
                raise NotImplementedError(f"{type(self).__name__}: DTensor / FSDP2 parameters are not supported")
            if p.dtype == torch.float16:
                raise NotImplementedError(f"{type(self).__name__}: float16 parameters are not supported (bfloat16 and float32 are)")
        # lr lives as a CPU fp32 tensor
        if not isinstance(group["lr"], Tensor):
            group["lr"] = torch.tensor(group["lr"], dtype=torch.float32)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)

    # a zero-filled state subclass for p
    @staticmethod
    def _subclass_zeros(p: Tensor, signed: bool, block_size: int):
        raise NotImplementedError

    _FORMAT = PLAIN

    def _quantizes(self, p: Tensor) -> bool:
        """bitsandbytes' rule, the reference's: at least 4096 values, and whole blocks"""
        return self.block_size is not None and p.numel() >= 4096 and p.numel() % self.block_size == 0

    def _new_buffer(self, p: Tensor, signed: bool):
        if self._quantizes(p):
            return self._subclass_zeros(p, signed, self.block_size)
        return torch.zeros_like(p, memory_format=torch.contiguous_format)

    @staticmethod
    def _kernel_fields(state):
        if state is None:
            return None, None, None
        if isinstance(state, (OptimState8bit, OptimState4bit)):
            return state.codes, state.scale, state.qmap
        if isinstance(state, OptimStateFp8):
            return state.codes, state.scale, None
        return state, None, None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.step() cannot be captured in a hipGraph: the step's scalars go to the kernel by value and "
                               "change every step")

        param_index = -1
        for group in self.param_groups:
            scalars_of = {}  # step count -> the eight scalars: the parameters of a group usually share it
            for p in group["params"]:
                param_index += 1
                if p.grad is None:
                    continue
                grad = p.grad
                if grad.is_sparse:
                    raise RuntimeError("Sparse gradient is not supported")
                if grad.dtype != p.dtype:
                    raise RuntimeError(f"{type(self).__name__}: a gradient of dtype {grad.dtype} for a parameter of dtype {p.dtype} is not supported")

                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0)
                    state["exp_avg"] = self._new_buffer(p, True)
                    state["exp_avg_sq"] = self._new_buffer(p, False)
                    if group["amsgrad"]:
                        state["max_exp_avg_sq"] = self._new_buffer(p, False)
                state["step"] += 1

                if not isinstance(group["lr"], Tensor):
                    raise RuntimeError(
                        "lr was changed to a non-Tensor object. If you want to update lr, please use "
                        "optim.param_groups[0]['lr'].fill_(new_lr)"
                    )
                t = float(state["step"])
                key = (t, float(group["lr"]))
                if key not in scalars_of:
                    scalars_of[key] = step_scalars(group["lr"], group["betas"][0], group["betas"][1], group["weight_decay"], group["eps"], state["step"])

                quantized = isinstance(state["exp_avg"], (OptimState8bit, OptimState4bit, OptimStateFp8))
                ops.optim_adam_step(
                    p.detach(), grad,
                    *self._kernel_fields(state["exp_avg"]), *self._kernel_fields(state["exp_avg_sq"]),
                    *self._kernel_fields(state.get("max_exp_avg_sq", None)),
                    self._FORMAT if quantized else PLAIN,
                    state["exp_avg"].block_size if quantized else 0,
                    scalars_of[key], self.is_adamw,
                    sr=self.bf16_stochastic_round and p.dtype is torch.bfloat16, seed=self.sr_seed, step=int(t), param_index=param_index)
        return loss


def _make(name, fmt, zeros, default_block, is_adamw, default_wd):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=default_wd, amsgrad=False, *, block_size=default_block,
                 bf16_stochastic_round=False, sr_seed=None) -> None:
        _AdamBase.__init__(self, params, lr, betas, eps, weight_decay, amsgrad, block_size=block_size, bf16_stochastic_round=bf16_stochastic_round,
                           is_adamw=is_adamw, sr_seed=sr_seed)

    return type(name, (_AdamBase,), {"__init__": __init__, "_subclass_zeros": staticmethod(zeros), "_FORMAT": fmt, "__module__": __name__,
                                     "__doc__": f"torchao.optim.{name}: the same signature and defaults, plus sr_seed (the Philox seed of "
                                                "bf16_stochastic_round; default torch.initial_seed() at construction)."})


def _zeros8(p, signed, block_size):
    return OptimState8bit.zeros(p.shape, signed, block_size, p.device, dtype=p.dtype)


def _zeros4(p, signed, block_size):
    return OptimState4bit.zeros(p.shape, signed, block_size, p.device, dtype=p.dtype)


def _zeros_fp8(p, signed, block_size):
    return OptimStateFp8.zeros(p.shape, block_size, p.device, dtype=p.dtype)


Adam8bit = _make("Adam8bit", Q8_SIGNED, _zeros8, 256, False, 0)
Adam4bit = _make("Adam4bit", Q4_SIGNED, _zeros4, 128, False, 0)
AdamFp8 = _make("AdamFp8", FP8, _zeros_fp8, 256, False, 0)
AdamW8bit = _make("AdamW8bit", Q8_SIGNED, _zeros8, 256, True, 1e-2)
AdamW4bit = _make("AdamW4bit", Q4_SIGNED, _zeros4, 128, True, 1e-2)
AdamWFp8 = _make("AdamWFp8", FP8, _zeros_fp8, 256, True, 1e-2)


class _AdamW(_AdamBase):
    """AdamW with plain moments in the parameter's dtype (torchao.optim._AdamW): every parameter takes the PLAIN form of the one launch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, bf16_stochastic_round=False,
                 sr_seed=None) -> None:
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, block_size=None, bf16_stochastic_round=bf16_stochastic_round,
                         is_adamw=True, sr_seed=sr_seed)
