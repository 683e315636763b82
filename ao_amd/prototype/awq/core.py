"""AWQObserver and AWQObservedLinear: the calibration side of AWQConfig.

Host-side mirror of torchao/prototype/awq/core.py (same names, same constructor, forward(input, output) and calculate_qparams()).

The reference keeps every calibration input on the CPU, concatenates them, and for each of its 20 ratios scales the weight, runs the whole
int4 quantize_ handler and two F.linear calls over all the tokens, and reads the loss back with .item() (core.py:59-87).  The loss it
minimises,

    mean((X W^T - (X / s) Wq^T)^2)  =  tr(D G D^T) / (rows N),      D = W - Wq / s  (column k of Wq divided by s[k]),   G = X^T X,

needs of the inputs only the K x K matrix G (the bias cancels in the difference).  So the observer keeps two unnormalised fp32 sums on the
weight's device -- G, one addmm_ per forward like the GPTQ observer's Hessian, and sum |x| per channel -- and the row count on the host:
calibration memory is O(K^2) whatever the token count, and the search never touches the inputs.  Per chunk of ratios the search is ONE
launch over the weight (ops.awq_scaled_error, csrc/awq_kernels.hip, which states the arithmetic: D of every ratio of the chunk, W read
once) and ONE fp32 matmul against G; the winner is picked on the device.  Nothing synchronises.  The matmul is the search's time (2 R N K^2
flops whatever the token count): measured, the search is ahead of the reference's loop only where the rows far exceed K.

Deviations, on purpose:
  * the loss is the exact quadratic form through G in fp32; the reference subtracts two bf16-rounded outputs of its own kernels.  The two
    can pick different ratios when losses are nearly tied; this library's contract is the float64 value of the reference's formula.
  * x_mean is the fp32 running sum divided once and rounded once to the weight's dtype; the reference takes the mean of the concatenated
    bf16 inputs.
  * memory: one fp32 K x K buffer per observed linear (0.82 GB at K = 14336); linears fed by the same activation each keep their own.
"""
from typing import Optional

import torch
import torch.nn.functional as F

from ... import ops
from ...quantization.config import AOBaseConfig

__all__ = ["AWQObserver", "AWQObservedLinear", "AWQ_SEARCH_BYTES"]

# The most bytes the search's two fp32 work buffers of one chunk of ratios -- D [Rc, N, K] and T = D G, the same shape -- may take together;
# Rc = max(1, AWQ_SEARCH_BYTES // (8 N K)).  4 GiB: Llama-3-8B's largest linear (4096 x 14336 or 14336 x 4096, 0.47 GB per ratio for the
# pair) runs its 20 ratios in chunks of 9, 9 and 2; a 4096 x 4096 linear in one chunk.  A weight whose single ratio is larger still runs, one
# ratio at a time.
AWQ_SEARCH_BYTES = 4 << 30


class AWQObserver(torch.nn.Module):
    """reference core.py:23-87.  weight: bf16 [N, K]; base_config: the Int4WeightOnlyConfig (PLAIN) whose quantizer the search judges.

    State, on the weight's device: abs_sum fp32 [K] = sum |x|, gram fp32 [K, K] = sum x^T x, and `rows`, a host int (a forward never reads
    the device back).  After calculate_qparams: scales (the table S, [R, K] in the weight's dtype), losses (fp32 [R]) and best_index
    (a 0-dim int64 tensor), all on the device."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], base_config: AOBaseConfig, scale_search_space_size: int = 20):
        super().__init__()
        if weight.dim() != 2:
            raise NotImplementedError(f"AWQ on MI355X observes 2-D linear weights, got shape {tuple(weight.shape)}")
        if int(scale_search_space_size) < 1:
            raise ValueError(f"scale_search_space_size must be at least 1, got {scale_search_space_size}")
        self.base_config = base_config
        self.weight = weight
        self.bias = bias
        self.scale_options = int(scale_search_space_size)
        k = weight.shape[1]
        self.register_buffer("abs_sum", torch.zeros(k, dtype=torch.float32, device=weight.device), persistent=False)
        self.register_buffer("gram", torch.zeros(k, k, dtype=torch.float32, device=weight.device), persistent=False)
        self.rows = 0
        self.scales = self.losses = self.best_index = None

    @torch.no_grad()
    def forward(self, input: torch.Tensor, output: torch.Tensor):
        x = input.detach().reshape(-1, input.shape[-1]).to(device=self.gram.device, dtype=torch.float32)
        self.abs_sum += x.abs().sum(0)
        self.gram.addmm_(x.t(), x)
        self.rows += x.shape[0]

    @torch.no_grad()
    def get_act_scale(self) -> torch.Tensor:
        """The reference's get_act_scale (core.py:19-20) of everything observed: mean |x| per channel, in the weight's dtype."""
        rows = torch.tensor(float(self.rows), dtype=torch.float32, device=self.abs_sum.device)  # (a tensor: the correctly rounded quotient)
        return (self.abs_sum / rows).to(self.weight.dtype)

    @torch.no_grad()
    def scale_table(self, x_mean: torch.Tensor) -> torch.Tensor:
        """The R candidate scale vectors, the reference's own tensor ops on [K] vectors (core.py:71-76).  Row 0 is all ones."""
        dtype, R = self.weight.dtype, self.scale_options
        rows = []
        for i in range(R):
            ratio = i * 1 / R
            scales = x_mean.pow(ratio).to(dtype).clamp(min=1e-4).view(-1)
            rows.append(scales / (scales.max() * scales.min()).sqrt())
        return torch.stack(rows).contiguous()

    @torch.no_grad()
    def search_losses(self, W: torch.Tensor, S: torch.Tensor, group_size: int) -> torch.Tensor:
        """fp32 [R]: tr(D[r] G D[r]^T) / (rows N), a chunk of ratios per launch and matmul."""
        n, k = W.shape
        chunk = max(1, AWQ_SEARCH_BYTES // (8 * n * k))
        out = []
        for r0 in range(0, S.shape[0], chunk):
            D = ops.awq_scaled_error(W, S[r0:r0 + chunk], group_size)
            T = torch.matmul(D.view(-1, k), self.gram).view_as(D)
            out.append(T.mul_(D).sum((1, 2)))
            del D, T
        return torch.cat(out) / float(self.rows * n)

    @torch.no_grad()
    def calculate_qparams(self) -> torch.Tensor:
        if self.rows == 0 or self.gram is None:
            raise ValueError("calibrate observer first by running model on exemplar data")
        from .api import _group_size_of

        g = _group_size_of(self.base_config)
        W = self.weight.detach().contiguous()
        S = self.scale_table(self.get_act_scale())
        losses = self.search_losses(W, S, g)
        # the first minimum wins, like the reference's strict `<`; a NaN loss never does, and an all-NaN search keeps row 0 (all ones)
        best = torch.argmin(torch.where(torch.isnan(losses), torch.full_like(losses, float("inf")), losses))
        self.scales, self.losses, self.best_index = S, losses, best
        return S.index_select(0, best.reshape(1))[0].detach()

    def release(self):
        """Drop the K x K accumulator and the channel sums (convert does, once the scale is chosen)."""
        self.gram = None
        self.abs_sum = None


class AWQObservedLinear(torch.nn.Linear):
    """reference core.py:90-120: the plain linear, then the observer sees (input, output)."""

    def __init__(self, in_features: int, out_features: int, act_obs: torch.nn.Module, bias: bool = True, device=None, dtype=None):
        super().__init__(in_features, out_features, bias, device, dtype)
        self.act_obs = act_obs

    def forward(self, input: torch.Tensor):
        output = F.linear(input, self.weight, self.bias)
        self.act_obs(input, output)
        return output

    @classmethod
    def from_float(cls, float_linear: torch.nn.Linear, act_obs: AWQObserver):
        observed_linear = cls(float_linear.in_features, float_linear.out_features, act_obs, False, device="meta",
                              dtype=float_linear.weight.dtype)  # (meta: the placeholder weight is replaced on the next line)
        observed_linear.weight = float_linear.weight
        observed_linear.bias = float_linear.bias
        return observed_linear
