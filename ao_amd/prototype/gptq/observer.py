"""GPTQObserverTensor: the weight wrapper of GPTQConfig(step="observe").

Host-side mirror of torchao/prototype/gptq/observer.py (same fields: hp_data, total_batches, hessian; from_hp, update_2d).  F.linear on the
wrapper folds the activation into the running mean of the Hessian and then runs the plain linear on hp_data.

  H <- H tb / (tb + n) + (2 / (tb + n)) X^T X      (observer.py:67-89; n = 1 for a 2-D input, else its leading dimension)

in fp32 on the weight's device, as ONE torch addmm_ (plumbing, not a kernel of this library; the reference scales X by sqrt(2 / tb) first
and adds a separate matmul: the same mean up to fp32 rounding).  The batch count is kept on the host as well, so a forward never reads the
device count back (the reference's two .item() calls a forward); a tensor rebuilt from its fields reads it once, at its first update.

3-D expert weights and their bmm / _grouped_mm hooks (update_3d, update_3d_with_offs) are not implemented.
"""
import torch
import torch.nn.functional as F

from ...quantization.base_tensor import LowBitTensorBase, aten

__all__ = ["GPTQObserverTensor"]

_NO_3D = ("GPTQ on MI355X observes 2-D linear weights: 3-D expert weights and the bmm / _grouped_mm observer hooks (gptq_quantize_3d) are "
          "not implemented")


class GPTQObserverTensor(LowBitTensorBase):
    tensor_data_names = ["hp_data", "total_batches"]
    optional_tensor_data_names = ["hessian"]
    tensor_attribute_names = []
    _quantized_weight = False  # quantize_'s default filter still selects a linear whose weight is being observed

    def __new__(cls, hp_data: torch.Tensor, total_batches, hessian=None):
        return torch.Tensor._make_wrapper_subclass(cls, hp_data.shape, device=hp_data.device, dtype=hp_data.dtype, requires_grad=False)

    def __init__(self, hp_data: torch.Tensor, total_batches, hessian=None):
        if hp_data.dim() != 2:
            raise NotImplementedError(f"{_NO_3D}, got a weight of shape {tuple(hp_data.shape)}")
        self.hp_data = hp_data
        if isinstance(total_batches, torch.Tensor):
            self.total_batches = total_batches
            self._host_batches = [None]  # unknown until the first update reads it, once
        else:
            self.total_batches = torch.full((1,), int(total_batches), dtype=torch.int64, device=hp_data.device)
            self._host_batches = [int(total_batches)]
        if hessian is None:
            assert hp_data.is_contiguous()
            k = hp_data.shape[-1]
            hessian = torch.zeros(k, k, dtype=torch.float32, device=hp_data.device)
        self.hessian = hessian

    def _quantization_type(self):
        return f"shape={tuple(self.shape)}, device={self.device}, batches={self._host_batches[0]}"

    def _apply_fn_to_data(self, fn):
        out = GPTQObserverTensor(fn(self.hp_data), fn(self.total_batches), fn(self.hessian))
        out._host_batches = self._host_batches  # views of one observer (detach, the nn.Parameter wrapper) share its count
        return out

    @property
    def batches(self) -> int:
        """The batch count, from the host copy (read back from the device once if this tensor was rebuilt from its fields)."""
        if self._host_batches[0] is None:
            self._host_batches[0] = int(self.total_batches[0].item())
        return self._host_batches[0]

    def update_2d(self, input: torch.Tensor):
        shape = input.shape
        n = 1 if len(shape) == 2 else shape[0]
        x = input.detach().reshape(-1, shape[-1]).to(device=self.hp_data.device, dtype=torch.float32)
        tb = self.batches
        self.hessian.addmm_(x.t(), x, beta=tb / (tb + n), alpha=2.0 / (tb + n))
        self.total_batches += n
        self._host_batches[0] = tb + n

    def update_3d(self, input: torch.Tensor):
        raise NotImplementedError(_NO_3D)

    def update_3d_with_offs(self, input: torch.Tensor, offs: torch.Tensor):
        raise NotImplementedError(_NO_3D)

    @classmethod
    def from_hp(cls, hp_tensor):
        return GPTQObserverTensor(hp_tensor, 0, None)


implements = GPTQObserverTensor.implements
implements_torch_function = GPTQObserverTensor.implements_torch_function


@implements(aten.linear.default)
@implements_torch_function(F.linear)
def _(func, types, args, kwargs):
    input_tensor, weight_tensor = args[0], args[1]
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    if not isinstance(weight_tensor, GPTQObserverTensor):
        raise ValueError(f"Expected weight_tensor to be GPTQObserverTensor, got: {type(weight_tensor)}")
    weight_tensor.update_2d(input_tensor.detach())
    return F.linear(input_tensor, weight_tensor.hp_data, bias)


@implements([aten.bmm.default] + ([aten._grouped_mm.default] if hasattr(aten, "_grouped_mm") else []))
@implements_torch_function([torch.bmm] + ([torch._grouped_mm] if hasattr(torch, "_grouped_mm") else []))
def _(func, types, args, kwargs):
    raise NotImplementedError(_NO_3D)
