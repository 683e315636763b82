"""NVFP4 MoE grouped GEMM, inference forward: e2m1 codes, one float8_e4m3fn scale per 1 x 16 block, an optional fp32 scale per expert --
the routed experts of an NVFP4-quantized MoE model, MI355X-native (ao_nvfp4_grouped_mm).

The reference has the operation on NVFP4Tensor itself: aten._grouped_mm on a 3-D NVFP4Tensor with a per-expert [E, 1, 1] scale
(prototype/mx_formats/nvfp4_tensor.py:709-753, inference_workflow.py:309-319), which runs only through mslk or scaled_grouped_mm on
sm100, and a portable emulation that dequantizes both operands to bf16 (prototype/moe_training/nvfp4_grouped_mm.py:62-116).  Here the
experts are a plain holder, NVFP4ExpertWeights, as Float8BlockwiseExpertWeights is for blockwise float8, and the GEMM is a function:
NVFP4Tensor stays 2-D with a 0-dim per-tensor scale and keeps refusing 3-D weights and aten._grouped_mm.
  * weight-only: bf16(sum_k x bf16(dequantize(w_e))) per group, one launch that reads 0.5625 bytes a weight -- the reference's
    torch._grouped_mm(x, dequantize(bf16)^T, offs);
  * codes x codes: the optional per-group amax, the grouped 1 x 16 cast, then the GEMM on codes with NVFP4Tensor's dense output chain
    per group (bf16(acc), or bf16(bf16(acc) bf16(pa_e pb_e)) with per-tensor scales).
Forward only; no bias (_grouped_mm has none); scales row-major.
"""
from typing import Optional, Sequence

import torch

from .. import ops
from ..torch_ops import kernels
from .nvfp4_tensor import BLOCK, E2M1_VALUES, NVFP4Tensor

__all__ = ["NVFP4ExpertWeights", "nvfp4_grouped_mm"]

_CLS = "NVFP4ExpertWeights"
_NAME = "nvfp4_grouped_mm"


def _expert_scale(what, p, e):
    if p is None:
        return None
    if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
        raise ValueError(f"{_CLS}: {what} must be a float32 tensor of one scale an expert, got "
                         f"{p.dtype if isinstance(p, torch.Tensor) else type(p).__name__}")
    if p.dim() not in (1, 3) or p.numel() != e or p.shape[0] != e:
        raise ValueError(f"{_CLS}: {what} must have shape [E] or [E, 1, 1] with E = {e}, got {tuple(p.shape)}")
    return p.reshape(e).contiguous()


class NVFP4ExpertWeights:
    """Expert weights in NVFP4, what the grouped GEMM streams: qdata uint8 [E, N, K/2] (element 2i in the low nibble of byte i), scale
    float8_e4m3fn [E, N, K/16] row-major, per_tensor_scale fp32 [E] (one an expert: the reference's [E, 1, 1]) or None,
    act_per_tensor_scale fp32 [E] (the static scale of each expert's token group) or None."""

    def __init__(self, qdata: torch.Tensor, scale: torch.Tensor, per_tensor_scale: Optional[torch.Tensor] = None,
                 act_per_tensor_scale: Optional[torch.Tensor] = None):
        if qdata.dim() != 3 or qdata.dtype != torch.uint8:
            raise ValueError(f"{_CLS}: qdata must be uint8 [E, N, K/2] (packed e2m1 codes), got {qdata.dtype} {tuple(qdata.shape)}")
        e, n, k = qdata.shape[0], qdata.shape[1], qdata.shape[2] * 2
        if e < 1 or n < 1:
            raise ValueError(f"{_CLS}: qdata must hold at least one expert and one row, got {tuple(qdata.shape)}")
        if k == 0 or k % BLOCK != 0:
            raise ValueError(f"{_CLS}: K must be a positive multiple of {BLOCK}, got {k}")
        want = (e, n, k // BLOCK)
        if scale.dtype != torch.float8_e4m3fn or tuple(scale.shape) != want:
            raise ValueError(f"{_CLS}: scale must be float8_e4m3fn [E, N, K/16] = {want}, row-major, got {scale.dtype} {tuple(scale.shape)}")
        self.qdata, self.scale = qdata.contiguous(), scale.contiguous()
        self.per_tensor_scale = _expert_scale("per_tensor_scale", per_tensor_scale, e)
        self.act_per_tensor_scale = _expert_scale("act_per_tensor_scale", act_per_tensor_scale, e)

    @classmethod
    def from_hp(cls, w: torch.Tensor, use_per_expert_scale: bool = True, act_per_tensor_scale: Optional[torch.Tensor] = None):
        """w bf16 [E, N, K], the experts as stored.  The reference's to_nvfp4(w, per_tensor_scale=per_tensor_amax_to_scale(amax over
        (1, 2)).view(E, 1, 1)) bytes (inference_workflow.py:309-319): the per-expert amax and the cast run on the device over the
        [E N, K] view, whose groups are the experts."""
        if w.dim() != 3 or w.dtype != torch.bfloat16:
            raise ValueError(f"{_CLS}.from_hp: w must be a 3-D bfloat16 tensor [E, N, K], got {w.dtype} {tuple(w.shape)}")
        e, n, k = w.shape
        if e < 1 or n < 1 or k == 0 or k % BLOCK != 0:
            raise ValueError(f"{_CLS}.from_hp: E and N must be positive and K a positive multiple of {BLOCK}, got {tuple(w.shape)}")
        w2 = w.contiguous().reshape(e * n, k)
        offs = torch.arange(1, e + 1, dtype=torch.int32, device=w.device) * n
        k_ = kernels(w2)
        p = k_.nvfp4_group_amax_scale(w2, offs) if use_per_expert_scale else None
        q, s = k_.nvfp4_quantize_grouped(w2, p, offs)
        return cls(q.reshape(e, n, k // 2), s.reshape(e, n, k // BLOCK), p, act_per_tensor_scale)

    @classmethod
    def from_nvfp4_tensors(cls, tensors: Sequence[NVFP4Tensor]):
        """Per-expert 2-D NVFP4Tensors of one shape, stored [N, K] row-major: all with a per-tensor scale or none (likewise the
        activation's)."""
        tensors = list(tensors)
        if not tensors:
            raise ValueError(f"{_CLS}.from_nvfp4_tensors: no experts given")
        for t in tensors:
            if not isinstance(t, NVFP4Tensor) or t.qdata.dim() != 2 or not t.qdata.is_contiguous():
                raise ValueError(f"{_CLS}.from_nvfp4_tensors: every expert must be a 2-D row-major NVFP4Tensor, got {type(t).__name__}")
            if t.qdata.shape != tensors[0].qdata.shape:
                raise ValueError(f"{_CLS}.from_nvfp4_tensors: the experts differ in shape: {tuple(t.shape)} vs {tuple(tensors[0].shape)}")

        def stack(name):
            vals = [getattr(t, name) for t in tensors]
            if all(v is None for v in vals):
                return None
            if any(v is None for v in vals):
                raise ValueError(f"{_CLS}.from_nvfp4_tensors: {name} must be set on every expert or on none")
            return torch.stack([v.reshape(()).to(torch.float32) for v in vals])

        return cls(torch.stack([t.qdata for t in tensors]), torch.stack([t.scale.view(torch.uint8) for t in tensors]).view(torch.float8_e4m3fn),
                   stack("per_tensor_scale"), stack("act_per_tensor_scale"))

    @classmethod
    def from_reference_layout(cls, qdata: torch.Tensor, swizzled_scale: torch.Tensor, per_tensor_scale: Optional[torch.Tensor] = None,
                              act_per_tensor_scale: Optional[torch.Tensor] = None):
        """From the tensors of a reference-produced 3-D NVFP4Tensor with is_swizzled_scales=True: qdata [E, N, K/2], the scale in
        to_blocked's 128 x 4 layout per expert (any shape of E x 32 ceil(N / 128) x 16 ceil(K / 64) elements).  Un-swizzled once, here,
        per expert as NVFP4Tensor.from_reference_layout does."""
        if qdata.dim() != 3:
            raise ValueError(f"{_CLS}.from_reference_layout: qdata must be 3-D [E, N, K/2], got {tuple(qdata.shape)}")
        e = qdata.shape[0]
        if swizzled_scale.numel() % e != 0:
            raise ValueError(f"{_CLS}.from_reference_layout: the swizzled scale's {swizzled_scale.numel()} elements do not divide over "
                             f"{e} experts")
        sw = swizzled_scale.contiguous().view(torch.uint8).reshape(e, -1)
        dense = [NVFP4Tensor.from_reference_layout(qdata[i].contiguous(), sw[i].view(torch.float8_e4m3fn)) for i in range(e)]
        return cls(torch.stack([t.qdata for t in dense]), torch.stack([t.scale.view(torch.uint8) for t in dense]).view(torch.float8_e4m3fn),
                   per_tensor_scale, act_per_tensor_scale)

    @property
    def shape(self):
        """[E, N, K], the experts as stored"""
        e, n, kh = self.qdata.shape
        return torch.Size((e, n, kh * 2))

    @property
    def device(self):
        return self.qdata.device

    def __len__(self):
        return self.qdata.shape[0]

    def __getitem__(self, e: int) -> NVFP4Tensor:
        """Expert e as a dense NVFP4Tensor (views of this holder's tensors) with 0-dim scales."""
        if not isinstance(e, int):
            raise TypeError(f"{_CLS}: experts are indexed by one integer, got {type(e).__name__}")
        p = None if self.per_tensor_scale is None else self.per_tensor_scale[e]
        pa = None if self.act_per_tensor_scale is None else self.act_per_tensor_scale[e]
        return NVFP4Tensor(self.qdata[e], self.scale[e], BLOCK, torch.bfloat16, p, pa)

    def dequantize(self, output_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        """[E, N, K]: f32(code) times (per_tensor_scale[e] f32(block scale)) in fp32, rounded to the output dtype -- NVFP4Tensor.dequantize
        per expert, the reference's bits."""
        e, n, kh = self.qdata.shape
        lut = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=self.qdata.device)
        codes = torch.stack([self.qdata & 0xF, self.qdata >> 4], dim=-1).reshape(e, n, kh * 2)
        s = self.scale.to(torch.float32)
        if self.per_tensor_scale is not None:
            s = self.per_tensor_scale.reshape(e, 1, 1) * s
        out = lut[codes.long()].reshape(e, n, kh * 2 // BLOCK, BLOCK) * s.unsqueeze(-1)
        return out.reshape(e, n, kh * 2).to(output_dtype)


def nvfp4_grouped_mm(A: torch.Tensor, experts: NVFP4ExpertWeights, offs: torch.Tensor, *, weight_only: bool = False,
                     use_dynamic_per_group_scale: bool = False, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """A bf16 [M_total, K] (tokens grouped by expert) x experts -> bf16 [M_total, N]; offs int32 [E], cumulative group ends, read on the
    device (no padding step, no host sync).  Rows past offs[-1] are zero.
    weight_only: one launch, NVFP4Tensor's weight-only linear per group.  Otherwise NVFP4Tensor's dynamic linear per group: the
    activation's scale of group e is the device amax of its rows (use_dynamic_per_group_scale; an all-zero or empty group is outside the
    contract, as a zero per-tensor scale is for the dense cast), else experts.act_per_tensor_scale, else none; then the grouped 1 x 16
    cast and the codes x codes GEMM."""
    if out_dtype != torch.bfloat16:
        raise ValueError(f"{_NAME}: only bfloat16 out_dtype is supported, got {out_dtype}")
    if not isinstance(experts, NVFP4ExpertWeights):
        raise ValueError(f"{_NAME}: experts must be an NVFP4ExpertWeights (NVFP4ExpertWeights.from_hp casts a bfloat16 [E, N, K] tensor "
                         f"once), got {type(experts).__name__}")
    if A.dtype != torch.bfloat16:
        raise NotImplementedError(f"NVFP4 on MI355X takes bfloat16 activations, got {A.dtype}: cast explicitly (.to(torch.bfloat16)) if that "
                                  "rounding is acceptable")
    if A.dim() != 2:
        raise ValueError(f"{_NAME}: A must be a 2-D tensor [M_total, K], got {tuple(A.shape)}")
    e, n, k = experts.shape
    if A.shape[1] != k:
        raise ValueError(f"{_NAME}: shapes {tuple(A.shape)} and {tuple(experts.shape)} [E, N, K] are not compatible")
    if offs.dtype != torch.int32 or offs.dim() != 1 or offs.numel() != e:
        raise ValueError(f"{_NAME}: offs must be int32 [E] = [{e}], got {offs.dtype} {tuple(offs.shape)}")
    if weight_only and use_dynamic_per_group_scale:
        raise ValueError(f"{_NAME}: weight_only casts no activation, so use_dynamic_per_group_scale has no meaning with it")
    A = A.contiguous()
    k_ = kernels(A)
    if weight_only:
        return k_.nvfp4_grouped_mm(ops.NVFP4_KIND_WEIGHT_ONLY, A, None, experts.qdata, experts.scale, offs, None, experts.per_tensor_scale)
    pa = k_.nvfp4_group_amax_scale(A, offs) if use_dynamic_per_group_scale else experts.act_per_tensor_scale
    aq, a_s = k_.nvfp4_quantize_grouped(A, pa, offs)
    return k_.nvfp4_grouped_mm(ops.NVFP4_KIND_DYNAMIC, aq, a_s, experts.qdata, experts.scale, offs, pa, experts.per_tensor_scale)
