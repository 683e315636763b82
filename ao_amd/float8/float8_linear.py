"""Float8Linear and its autograd Function, MI355X-native: the host mirror of torchao/float8/float8_linear.py:28-335.

The three GEMMs of a linear with W [N, K] all run through ops.fp8_scaled_mm (e4m3 x e4m3, one fp32 scale per row of each operand,
both operands contiguous along the contraction), so every operand is cast along the dimension its GEMM contracts and stored with that
dimension innermost:

  GEMM                 A (per-row scale)                              B (per-row scale)
  out         [M, N]   x cast along K                                 W cast along K
  grad_input  [M, K]   grad_out cast along N                          W cast along dim 0, stored transposed [K][N], one scale per k
  grad_weight [N, K]   grad_out cast along dim 0, transposed [N][M]   x cast along dim 0, transposed [K][M]

The casts are the HIP training casts of ops.fp8_train_* (csrc/fp8_train_kernels.hip): the reference's arithmetic
(float8_utils.py:31-53, :244-246; float8_training_tensor.py:153-154), which is not the inference cast's.  A TENSORWISE cast uses the
whole tensor's amax, its one scale filled into the vector the GEMM takes (float8_ops.py:356-359); a DISABLED pair runs torch.mm in
bf16 (ROWWISE_WITH_GW_HP's grad_weight).  The Function saves the high-precision input and weight and casts again in backward, as the
reference does.  DESIGN.md 4.18.

Left out:
  * an e5m2 GEMM operand, and with it the default config and the "tensorwise" recipe, whose grad_output is e5m2: the GEMM family here
    multiplies e4m3 x e4m3 (a bf8 MFMA form of it is the natural follow-up).  `check_config` refuses with the working alternative;
  * Float8TrainingTensor as a public tensor subclass (the Function calls the casts and the GEMM directly);
  * the FSDP2 and DTensor hooks (enable_fsdp_float8_all_gather is refused);
  * torch.compile of the Function;
  * pad_inner_dim (refused: K, N, and M where it is contracted, must be multiples of 16).
"""
import enum
from typing import NamedTuple, Optional

import torch

from .. import ops
from .config import CastConfig, Float8LinearConfig, ScalingGranularity, ScalingType, e4m3_dtype

__all__ = ["matmul_with_hp_or_float8_args", "Float8Linear", "ScaledMMConfig", "LinearMMConfig", "GemmInputRole", "check_config"]

_FP8_TYPES = (torch.float8_e4m3fn, torch.float8_e5m2, torch.float8_e4m3fnuz, torch.float8_e5m2fnuz)


class ScaledMMConfig(NamedTuple):
    """float8_training_tensor.py:46-61.  emulate and use_fast_accum are carried and select nothing: see matmul_with_hp_or_float8_args."""

    emulate: bool = False
    use_fast_accum: bool = False
    fp8_output: bool = False
    pad_inner_dim: bool = False


class LinearMMConfig(NamedTuple):
    """One ScaledMMConfig per GEMM (float8_training_tensor.py:64-80)."""

    output: ScaledMMConfig = ScaledMMConfig(False, True, False, False)
    grad_input: ScaledMMConfig = ScaledMMConfig(False, False, False, False)
    grad_weight: ScaledMMConfig = ScaledMMConfig(False, False, False, False)


class GemmInputRole(enum.Enum):
    """float8_training_tensor.py:83-93."""

    INPUT = "input"
    WEIGHT = "weight"
    GRAD_OUTPUT = "grad_output"


def check_config(config: Float8LinearConfig) -> None:
    """Refuse, with the reason, what this backend does not run of a Float8LinearConfig.  Called where a config is used (Float8Linear,
    convert_to_float8_training), not in the config's constructor, which stays the reference's; needs no GPU."""
    assert isinstance(config, Float8LinearConfig), f"expected a Float8LinearConfig, got {type(config).__name__}"
    for name in ("cast_config_input", "cast_config_input_for_grad_weight", "cast_config_weight", "cast_config_weight_for_grad_input",
                 "cast_config_grad_output", "cast_config_grad_output_for_grad_weight"):
        cc = getattr(config, name)
        if cc.scaling_type is not ScalingType.DISABLED and cc.target_dtype != e4m3_dtype:
            raise ValueError(
                f"{name}.target_dtype is {cc.target_dtype}: the float8 GEMMs on MI355X multiply float8_e4m3fn operands only (the default "
                "config and the 'tensorwise' recipe cast grad_output to e5m2).  For tensorwise scaling use "
                "Float8LinearConfig(cast_config_grad_output=CastConfig(target_dtype=e4m3_dtype)), or the 'rowwise' / "
                "'rowwise_with_gw_hp' recipes")
    if config.enable_fsdp_float8_all_gather:
        raise ValueError("enable_fsdp_float8_all_gather is not supported: the FSDP2 float8 all-gather hooks are left out of this backend")
    if config.pad_inner_dim:
        raise ValueError("pad_inner_dim is not supported: K and N (and M, where grad_weight is computed in float8) must be multiples of 16")


def _gemm_is_fp8(a: CastConfig, b: CastConfig) -> bool:
    return a.scaling_type is not ScalingType.DISABLED and b.scaling_type is not ScalingType.DISABLED


def _cast(t: torch.Tensor, row_cc: Optional[CastConfig], col_cc: Optional[CastConfig], pow2: bool):
    """The casts of t [R, C] that its GEMMs need, in as few passes over t as they allow: row_cc -> (q [R, C], scale, inv_scale) cast
    along dim -1, col_cc -> (q_t [C, R], scale, inv_scale) cast along dim 0 and stored transposed; None skips a direction.  AXISWISE
    takes the amax along the axis, TENSORWISE the whole tensor's for either layout."""
    axis = ScalingGranularity.AXISWISE
    row_ax = row_cc is not None and row_cc.scaling_granularity is axis
    col_ax = col_cc is not None and col_cc.scaling_granularity is axis
    tensorwise = (row_cc is not None and not row_ax) or (col_cc is not None and not col_ax)
    if row_ax and col_cc is None:
        return ops.fp8_train_quantize_rowwise(t, pow2), None
    if row_ax and col_ax:
        return ops.fp8_train_quantize_both(t, pow2)
    ra, ca = ops.fp8_train_amax(t, rows=row_ax or tensorwise, cols=col_ax)
    ta = ra.amax() if tensorwise else None
    return ops.fp8_train_cast(t, None if row_cc is None else (ra if row_ax else ta), None if col_cc is None else (ca if col_ax else ta), pow2)


class matmul_with_hp_or_float8_args(torch.autograd.Function):
    """input_hp [..., K] @ weight_hp_t [K, N] with each of the three GEMMs in float8 or in high precision as `config` says: the
    reference's Function (float8_linear.py:28-204), its argument order included.  weight_hp_t is the `.t()` view of the [N, K] weight.

    linear_mm_config carries `emulate` and `use_fast_accum` per GEMM.  Both are accepted and select nothing: the e4m3 MFMA accumulates
    in fp32 whatever they say, which is what the reference's emulated path computes (the precedent is KernelPreference.EMULATED in
    prototype/mx_training.py).

    Refused with a reason, before any launch: operands that are not bfloat16, or already cast to float8; K or N that is no multiple of
    16; a token count M that is no multiple of 16 while grad_weight is computed in float8 (M is that GEMM's contraction) -- use the
    ROWWISE_WITH_GW_HP recipe or freeze the weight."""

    @classmethod
    def apply(cls, input_hp: torch.Tensor, weight_hp_t: torch.Tensor, linear_mm_config: LinearMMConfig, config: Float8LinearConfig):
        # the refusals, where the grad mode of the call is still visible (inside forward it is always off)
        c = config
        check_config(c)
        for name, t in (("input", input_hp), ("weight", weight_hp_t)):
            assert t.dtype not in _FP8_TYPES and not hasattr(t, "_scale"), (
                f"{name} is already cast to float8: this backend casts inside the Function (Float8TrainingTensor operands are left out)")
            assert t.dtype == torch.bfloat16, f"{name} must be bfloat16, got {t.dtype}"
        assert weight_hp_t.ndim == 2 and input_hp.ndim >= 1 and input_hp.shape[-1] == weight_hp_t.shape[0], (
            f"shapes {tuple(input_hp.shape)} and {tuple(weight_hp_t.shape)} are not compatible (input [..., K], weight_t [K, N])")
        k, n = weight_hp_t.shape
        assert k % 16 == 0 and n % 16 == 0, f"K and N must be multiples of 16 (pad_inner_dim is not supported), got K={k} N={n}"
        m = input_hp.numel() // k
        fp8_gw = _gemm_is_fp8(c.cast_config_input_for_grad_weight, c.cast_config_grad_output_for_grad_weight)
        needs_gw = torch.is_grad_enabled() and weight_hp_t.requires_grad
        assert not (fp8_gw and needs_gw) or m % 16 == 0, (
            f"M={m} tokens must be a multiple of 16 while grad_weight is computed in float8 (M is that GEMM's contraction): use the "
            "ROWWISE_WITH_GW_HP recipe, which keeps grad_weight in bfloat16, or freeze the weight")
        return super().apply(input_hp, weight_hp_t, linear_mm_config, c)

    @staticmethod
    def forward(ctx, input_hp: torch.Tensor, weight_hp_t: torch.Tensor, linear_mm_config: LinearMMConfig, config: Float8LinearConfig):
        c = config
        k, n = weight_hp_t.shape
        ctx.save_for_backward(input_hp, weight_hp_t)
        ctx.linear_mm_config = linear_mm_config
        ctx.config = c
        pow2 = c.round_scales_to_power_of_2
        x = input_hp.reshape(-1, k)
        if _gemm_is_fp8(c.cast_config_input, c.cast_config_weight):
            (x_q, _, x_inv), _ = _cast(x, c.cast_config_input, None, pow2)
            (w_q, _, w_inv), _ = _cast(weight_hp_t.t(), c.cast_config_weight, None, pow2)  # W [N, K] along K
            out = ops.fp8_scaled_mm(x_q, w_q.t(), x_inv, w_inv)
        else:
            out = torch.mm(x, weight_hp_t)
        return out.reshape(*input_hp.shape[:-1], n)

    @staticmethod
    def backward(ctx, grad_output):
        input_hp, weight_hp_t = ctx.saved_tensors
        c = ctx.config
        pow2 = c.round_scales_to_power_of_2
        assert grad_output.dtype == torch.bfloat16, f"grad_output must be bfloat16, got {grad_output.dtype}"
        k, n = weight_hp_t.shape
        go = grad_output.contiguous().reshape(-1, n)  # (a transposed or strided grad_output: the casts take contiguous rows)
        x = input_hp.reshape(-1, k)
        need_input, need_weight = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        fp8_gi = need_input and _gemm_is_fp8(c.cast_config_grad_output, c.cast_config_weight_for_grad_input)
        fp8_gw = need_weight and _gemm_is_fp8(c.cast_config_grad_output_for_grad_weight, c.cast_config_input_for_grad_weight)

        # grad_output is read for both of its casts together: two passes over it where both gradients are float8 GEMMs
        go_rows = go_cols = None
        if fp8_gi or fp8_gw:
            go_rows, go_cols = _cast(go, c.cast_config_grad_output if fp8_gi else None,
                                     c.cast_config_grad_output_for_grad_weight if fp8_gw else None, pow2)

        grad_input = grad_weight_t = None
        if need_input:
            # grad_output [M, N] @ W [N, K], contracting N: W cast along dim 0 leaves transposed, [K][N], the operand as the GEMM stores it
            if fp8_gi:
                _, (w_t, _, w_inv) = _cast(weight_hp_t.t(), None, c.cast_config_weight_for_grad_input, pow2)
                grad_input = ops.fp8_scaled_mm(go_rows[0], w_t.t(), go_rows[2], w_inv)
            else:
                grad_input = torch.mm(go, weight_hp_t.t())
            grad_input = grad_input.reshape(*grad_output.shape[:-1], k)
        if need_weight:
            # grad_output^T [N, M] @ x [M, K], contracting the tokens: both operands cast along dim 0 and stored transposed
            if fp8_gw:
                _, (x_t, _, x_inv) = _cast(x, None, c.cast_config_input_for_grad_weight, pow2)
                grad_weight = ops.fp8_scaled_mm(go_cols[0], x_t.t(), go_cols[2], x_inv)
            else:
                grad_weight = torch.mm(go.t(), x)
            grad_weight_t = grad_weight.t()  # the gradient of weight_hp_t [K, N]
        return grad_input, grad_weight_t, None, None


class Float8Linear(torch.nn.Linear):
    """An nn.Linear whose GEMMs run in float8 as its Float8LinearConfig says (float8_linear.py:207-335).  Takes nn.Linear's arguments and
    `config=`; build it from an existing linear with `from_float`.  The bias is added outside the GEMM, in the output's dtype."""

    def __init__(self, *args, **kwargs):
        config = kwargs.pop("config")
        check_config(config)
        super().__init__(*args, **kwargs)
        self.scaling_type_input = config.cast_config_input.scaling_type
        self.scaling_type_weight = config.cast_config_weight.scaling_type
        self.scaling_type_grad_output = config.cast_config_grad_output.scaling_type
        self.config = config
        self.linear_mm_config = LinearMMConfig(
            ScaledMMConfig(config.emulate, config.gemm_config_output.use_fast_accum, False, config.pad_inner_dim),
            ScaledMMConfig(config.emulate, config.gemm_config_grad_input.use_fast_accum, False, config.pad_inner_dim),
            ScaledMMConfig(config.emulate, config.gemm_config_grad_weight.use_fast_accum, False, config.pad_inner_dim),
        )

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        # F.linear's autocast, so that the module's output has the dtype the plain linear's would (float8_linear.py:255-262)
        if torch.is_autocast_enabled():
            input = input.to(torch.get_autocast_gpu_dtype())
        output = matmul_with_hp_or_float8_args.apply(input, self.weight.t(), self.linear_mm_config, self.config)
        if self.bias is not None:
            output = output + self.bias.to(output.dtype)
        return output

    def extra_repr(self):
        c = self.config
        parts = [f"i:{c.cast_config_input.short_str()}", f"w:{c.cast_config_weight.short_str()}", f"go:{c.cast_config_grad_output.short_str()}"]
        if c.cast_config_input_for_grad_weight != c.cast_config_input:
            parts.append(f"i_gw:{c.cast_config_input_for_grad_weight.short_str()}")
        if c.cast_config_weight_for_grad_input != c.cast_config_weight:
            parts.append(f"w_gi:{c.cast_config_weight_for_grad_input.short_str()}")
        if c.cast_config_grad_output_for_grad_weight != c.cast_config_grad_output:
            parts.append(f"go_gw:{c.cast_config_grad_output_for_grad_weight.short_str()}")
        return f'{super().extra_repr()}, cast_configs={",".join(parts)}"'  # (the closing quote is the reference's)

    @classmethod
    def from_float(cls, mod, config: Optional[Float8LinearConfig] = None):
        """A Float8Linear that shares `mod`'s weight and bias Parameters (float8_linear.py:293-335)."""
        if config is None:
            config = Float8LinearConfig()
        check_config(config)
        with torch.device("meta"):
            new_mod = cls(mod.in_features, mod.out_features, bias=False, config=config)
        new_mod.weight = mod.weight
        new_mod.bias = mod.bias
        return new_mod
