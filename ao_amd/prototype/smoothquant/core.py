"""SmoothQuantObserver, RunningAbsMaxSmoothQuantObserver and SmoothQuantObservedLinear: the calibration side of SmoothQuantConfig.

Host-side mirror of torchao/prototype/smoothquant/core.py (same names, constructors, forward(input) -> input and
calculate_qparams(weight_quant_kwargs=None) -> (smoothing_factor, activation_scale, activation_zero_point)).

The reference's default observer copies every calibration input to the CPU, concatenates them at convert and reduces the concatenation
(core.py:37-53); its running observer copies an absmax to the CPU on every forward (:168-195).  What either needs of the inputs is a maximum,
and max is exact, so both observers here keep RUNNING maxima on the weight's device and a forward never reads the device back:

  x_abs_max  fp32 [K]   max |x| per input channel, folded by ops.sq_col_absmax_update (csrc/smoothquant_kernels.hip, kernel A): equal to the
                        reference's max(abs(cat(inputs))) bit for bit, O(K) memory instead of every input
  w_abs_max             kernel A on the weight
  smoothing_factor      the reference's own tensor ops on [K] vectors in the weight's dtype (core.py:53-63):
                        pow(x_abs_max + eps, alpha) / pow(w_abs_max + eps, 1 - alpha), eps = finfo(float32).eps; ones when alpha is None
  smoothed amax         fp32 scalar: max |bf16(x / smoothing_factor)|, folded by ops.sq_smoothed_amax_update (kernel B) one input at a time,
                        the quotient never written: the amax that the reference's from_hp(example_input / smoothing_factor) (:66-68) and its
                        second pass (:192-195, min and max of which only max(|min|, |max|) is used) reduce

A static base config needs the amax of the SMOOTHED activation, which depends on the final factor.  The default observer therefore keeps
the inputs when (and only when) a static scale is wanted (`keep_inputs`; on the device, not concatenated); the running observer has the
reference's two-pass protocol and keeps nothing.

Activation scale of the static case, fp32 [1, 1] resp. 0-dim, zero-point None (symmetric):
  default observer   max(bf16(amax / 127.5), fp32 eps): Int8Tensor.from_hp(., PerTensor())'s formula (csrc/quant_math.h int8_row_scale)
  running observer   amax / 127.5 clamped at fp32 eps (core.py:295-300), computed in the activation's dtype like the reference's tensors

Deviations, on purpose: the reference's _first_pass_min / _first_pass_max are never read by its calculate_qparams and are
not kept; a symmetric running scale comes with zero-point None, not the reference's int64 zero; inputs that are not bfloat16 on the GPU take
a torch-op path onto the same state.
"""
from typing import Optional

import torch
import torch.nn.functional as F

from ... import ops

__all__ = ["SmoothQuantObserver", "RunningAbsMaxSmoothQuantObserver", "SmoothQuantObservedLinear"]

_NOT_CALIBRATED = "calibrate observer first by running model on exemplar data"


def _uses_kernels(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0 and x.shape[-1] > 0


def _flat(input: torch.Tensor) -> torch.Tensor:
    return input.detach().reshape(-1, input.shape[-1])


@torch.no_grad()
def _col_absmax_update(x: torch.Tensor, state: torch.Tensor) -> None:
    """state[k] = max(state[k], max_m |x[m, k]|); x is [M, K] on the state's device"""
    if x.shape[0] == 0:
        return
    if _uses_kernels(x):
        ops.sq_col_absmax_update(x, state)
    else:
        torch.maximum(state, x.abs().amax(0).to(torch.float32), out=state)


@torch.no_grad()
def _smoothed_amax_update(x: torch.Tensor, s: torch.Tensor, amax: torch.Tensor) -> None:
    """amax = max(amax, max |x / s|), the quotient rounded to x's dtype as the reference's tensor division rounds it"""
    if x.shape[0] == 0:
        return
    if _uses_kernels(x) and s.dtype == torch.bfloat16:
        ops.sq_smoothed_amax_update(x, s, amax)
    else:
        torch.maximum(amax, (x / s).abs().amax().to(torch.float32).reshape(amax.shape), out=amax)


class _ObserverBase(torch.nn.Module):
    def __init__(self, weight: torch.Tensor, alpha: Optional[float] = 0.5):
        super().__init__()
        assert weight.ndim == 2
        self.weight = weight
        self.alpha = alpha
        self.device = weight.device

    def _to_state_device(self, input: torch.Tensor) -> torch.Tensor:
        x = _flat(input)
        return x if x.device == self.device else x.to(self.device)

    @torch.no_grad()
    def w_abs_max(self) -> torch.Tensor:
        """max |W| per input channel, in the weight's dtype (core.py:54)"""
        w = self.weight.detach()
        state = torch.zeros(w.shape[1], dtype=torch.float32, device=w.device)
        _col_absmax_update(w, state)
        return state.to(w.dtype)

    @torch.no_grad()
    def _factor_from(self, x_abs_max: torch.Tensor) -> torch.Tensor:
        """core.py:57-63 on [K] vectors in the weight's dtype"""
        x_abs_max = x_abs_max.to(self.weight.dtype)
        if self.alpha is None:
            return torch.ones_like(x_abs_max)
        eps = torch.finfo(torch.float32).eps
        return torch.pow(x_abs_max + eps, self.alpha) / torch.pow(self.w_abs_max() + eps, 1 - self.alpha)


def _symmetric_per_tensor(weight_quant_kwargs) -> None:
    """The static activation quantization this backend calibrates: one symmetric scale for the tensor.  `weight_quant_kwargs` is the base
    config's QuantizeTensorToInt8Kwargs, or the reference's dict form (quant_min / quant_max / is_symmetric / qscheme, core.py:287-293)."""
    from ...quantization.granularity import PerTensor
    from ...quantization.int8_tensor import _mapping
    from ...quantization.quant_primitives import MappingType

    if isinstance(weight_quant_kwargs, dict):
        symmetric = weight_quant_kwargs.get("is_symmetric", weight_quant_kwargs.get("qscheme", None) in (torch.per_tensor_symmetric,
                                                                                                         torch.per_channel_symmetric))
        if (weight_quant_kwargs.get("quant_min", -128), weight_quant_kwargs.get("quant_max", 127)) != (-128, 127) or not symmetric:
            raise NotImplementedError("SmoothQuant on MI355X calibrates a symmetric int8 (-128 .. 127) activation scale, got "
                                      f"{weight_quant_kwargs}")
        return
    if not isinstance(weight_quant_kwargs.granularity, PerTensor) or _mapping(weight_quant_kwargs.mapping_type) != MappingType.SYMMETRIC:
        raise NotImplementedError("SmoothQuant on MI355X calibrates a PerTensor symmetric static activation scale, got "
                                  f"{weight_quant_kwargs}")


class SmoothQuantObserver(_ObserverBase):
    """reference core.py:16-75.  weight: [N, K]; alpha: the exponent of the smoothing factor, None for ones.

    keep_inputs: keep the calibration inputs (on the weight's device, as they come) so that calculate_qparams(weight_quant_kwargs) can
    measure the smoothed activation's amax.  SmoothQuantConfig's prepare sets it for static base configs only; without it the observer's
    memory is the fp32 [K] running maximum.

    State: x_abs_max fp32 [K] on the weight's device, calibration_count (a host int), inputs (a list, empty unless keep_inputs)."""

    def __init__(self, weight: torch.Tensor, alpha: Optional[float] = 0.5, *, keep_inputs: bool = True):
        super().__init__(weight, alpha)
        self.keep_inputs = bool(keep_inputs)
        self.inputs = []
        self.calibration_count = 0
        self.register_buffer("x_abs_max", torch.zeros(weight.shape[1], dtype=torch.float32, device=weight.device), persistent=False)

    @torch.no_grad()
    def forward(self, input: torch.Tensor):
        x = self._to_state_device(input)
        _col_absmax_update(x, self.x_abs_max)
        if self.keep_inputs:
            self.inputs.append(x)
        self.calibration_count += 1
        return input

    @torch.no_grad()
    def calculate_qparams(self, weight_quant_kwargs=None):
        assert self.calibration_count > 0, _NOT_CALIBRATED
        smoothing_factor = self._factor_from(self.x_abs_max)
        if weight_quant_kwargs is None:
            return smoothing_factor, None, None
        _symmetric_per_tensor(weight_quant_kwargs)
        assert self.inputs, "SmoothQuantObserver(keep_inputs=False) kept no inputs to measure a static activation scale on"
        amax = torch.zeros(1, dtype=torch.float32, device=self.device)
        for x in self.inputs:
            _smoothed_amax_update(x, smoothing_factor, amax)
        # Int8Tensor.from_hp(x / s, PerTensor()): scale = max(bf16(amax / 127.5), eps) in the activation's dtype (a tensor divisor: the
        # correctly rounded quotient, then one rounding to the dtype), kept as fp32 like every Int8Tensor scale here
        dtype = self.inputs[0].dtype
        eps = torch.finfo(torch.float32).eps
        q = amax.to(dtype) / torch.tensor(127.5, dtype=torch.float32, device=self.device)
        scale = torch.clamp(q.to(dtype).to(torch.float32), min=eps).reshape(1, 1)
        return smoothing_factor, scale, None

    def release(self):
        """Drop the kept inputs (convert does, once the scale is measured)."""
        self.inputs = []


class RunningAbsMaxSmoothQuantObserver(_ObserverBase):
    """reference core.py:78-310: the two-pass protocol.

        for batch in calibration: model(batch)      # first pass: x_abs_max
        observer.compute_smoothing_factor()          # finalises the factor, switches to the second pass
        for batch in calibration: model(batch)      # second pass: the amax of batch / smoothing_factor
        observer.calculate_qparams(weight_quant_kwargs)

    State: x_abs_max (None before the first forward, then fp32 [K] on the weight's device), calibration_count, _smoothing_factor,
    _in_second_pass, _second_pass_count, _smooth_amax (fp32 [1]: max(|min|, |max|) of the smoothed activations, all the reference's
    symmetric scale takes of its _smooth_input_min / _smooth_input_max)."""

    def __init__(self, weight: torch.Tensor, alpha: Optional[float] = 0.5):
        super().__init__(weight, alpha)
        self.x_abs_max: Optional[torch.Tensor] = None
        self.calibration_count: int = 0
        self._smoothing_factor: Optional[torch.Tensor] = None
        self._in_second_pass: bool = False
        self._smooth_amax: Optional[torch.Tensor] = None
        self._smooth_dtype = None
        self._second_pass_count: int = 0

    @torch.no_grad()
    def forward(self, input: torch.Tensor):
        x = self._to_state_device(input)
        if not self._in_second_pass:
            if self.x_abs_max is None:
                self.x_abs_max = torch.zeros(self.weight.shape[1], dtype=torch.float32, device=self.device)
            _col_absmax_update(x, self.x_abs_max)
            self.calibration_count += 1
        else:
            assert self._smoothing_factor is not None
            if self._smooth_amax is None:
                self._smooth_amax = torch.zeros(1, dtype=torch.float32, device=self.device)
            _smoothed_amax_update(x, self._smoothing_factor, self._smooth_amax)
            self._smooth_dtype = x.dtype
            self._second_pass_count += 1
        return input

    @torch.no_grad()
    def compute_smoothing_factor(self) -> torch.Tensor:
        """Finalise the smoothing factor after the first pass and switch to the second (core.py:208-240)."""
        assert self.x_abs_max is not None and self.calibration_count > 0, _NOT_CALIBRATED
        self._smoothing_factor = self._factor_from(self.x_abs_max)
        self._in_second_pass = True
        self._smooth_amax = None
        self._second_pass_count = 0
        return self._smoothing_factor

    @torch.no_grad()
    def calculate_qparams(self, weight_quant_kwargs=None):
        assert self.x_abs_max is not None and self.calibration_count > 0, _NOT_CALIBRATED
        smoothing_factor = self._smoothing_factor if self._smoothing_factor is not None else self._factor_from(self.x_abs_max)
        if weight_quant_kwargs is None:
            return smoothing_factor, None, None
        if not (self._in_second_pass and self._second_pass_count > 0):
            return smoothing_factor, None, None  # second pass not completed (core.py:308-310)
        _symmetric_per_tensor(weight_quant_kwargs)
        # core.py:295-300: abs_max / ((qmax - qmin) / 2), clamped at fp32 eps, in the smoothed activation's dtype
        dtype = self._smooth_dtype
        q = self._smooth_amax.to(dtype) / torch.tensor(127.5, dtype=torch.float32, device=self.device)
        scale = torch.clamp(q.to(dtype).to(torch.float32), min=torch.finfo(torch.float32).eps).reshape(())
        return smoothing_factor, scale, None

    def release(self):
        pass


class SmoothQuantObservedLinear(torch.nn.Linear):
    """reference core.py:313-349: the observer sees the input, then the plain linear."""

    def __init__(self, in_features: int, out_features: int, obs, has_bias: bool = False, device=None, dtype=None):
        super().__init__(in_features, out_features, bias=has_bias, device=device, dtype=dtype)
        self.obs = obs

    def forward(self, input: torch.Tensor):
        input = self.obs(input)
        return F.linear(input, self.weight, self.bias)

    @classmethod
    def from_float(cls, float_linear: torch.nn.Linear, obs):
        observed_linear = cls(float_linear.in_features, float_linear.out_features, obs, has_bias=float_linear.bias is not None, device="meta",
                              dtype=float_linear.weight.dtype)  # (meta: the placeholder weight is replaced on the next line)
        observed_linear.weight = float_linear.weight
        observed_linear.bias = float_linear.bias
        return observed_linear
