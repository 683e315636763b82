"""NVFP4 MoE grouped-GEMM training without a GPU: every refusal of _to_nvfp4_rht_rs_then_scaled_grouped_mm by its message, before any GPU
requirement; the six ops with their fakes; the exported symbols."""
import pytest
import torch

SIGN = (1, 1, 1, -1, 1, -1, -1, -1, -1, -1, -1, 1, -1, 1, -1, -1)


def _args(**kw):
    a = dict(A=torch.zeros(32, 32, dtype=torch.bfloat16), B=torch.zeros(2, 48, 32, dtype=torch.bfloat16), sign_vector=SIGN,
             sr_seed=torch.zeros(1, dtype=torch.int64), offs=torch.tensor([16, 32], dtype=torch.int32))
    a.update(kw)
    return a


REFUSALS = [
    (dict(A=torch.zeros(32)), "input_act must be 2D"),
    (dict(B=torch.zeros(48, 32)), "weight must be 3D"),
    (dict(sign_vector=torch.ones(16)), "sign_vector must be a tuple or list with 16 elements"),
    (dict(sign_vector=SIGN[:15]), "sign_vector must be a tuple or list with 16 elements"),
    (dict(sign_vector=(0,) + SIGN[1:]), "sign_vector elements must be -1 or 1"),
    (dict(offs=None), "offs is required"),
    (dict(offs=torch.tensor([16, 32])), "offs must be a 1D int32 tensor"),
    (dict(offs=torch.tensor([0, 16, 0, 32], dtype=torch.int32)[1::2]), "offs must be contiguous"),
    (dict(offs=torch.tensor([32], dtype=torch.int32)), "one group-end offset per expert"),
    (dict(sr_seed=torch.zeros(2, dtype=torch.int64)), "sr_seed must be a one-element tensor"),
    (dict(sr_seed=torch.zeros(1, dtype=torch.int32)), "sr_seed must be an int64 tensor"),
    (dict(B=torch.zeros(2, 48, 64)), "contraction dimensions differ: 32 and 64"),
    (dict(A=torch.zeros(32, 24), B=torch.zeros(2, 48, 24)), "K and N must be divisible by 16; got K=24, N=48"),
    (dict(B=torch.zeros(2, 40, 32)), "K and N must be divisible by 16; got K=32, N=40"),
    (dict(A=torch.zeros(40, 32)), "M=40 tokens must be divisible by 16"),
    (dict(), "must be GPU tensors"),
    (dict(A=torch.zeros(40, 32), pad_token_groups_for_grouped_mm=True), "must be GPU tensors"),  # (padding lifts the M refusal)
]


@pytest.mark.parametrize("change,message", REFUSALS)
def test_refusals_name_their_cause_before_any_gpu_requirement(change, message):
    from ao_amd.prototype import _to_nvfp4_rht_rs_then_scaled_grouped_mm

    with pytest.raises(ValueError, match=message):
        _to_nvfp4_rht_rs_then_scaled_grouped_mm(**_args(**change))


def test_the_ops_have_fakes_and_the_symbols_are_exported():
    import ao_amd.torch_ops  # noqa: F401
    from ao_amd import _lib, ops, prototype
    from ao_amd.prototype import nvfp4_grouped_training as G

    m, n, k, e = 64, 48, 32, 2
    t = lambda dt, *s: torch.empty(s, dtype=dt, device="meta")  # noqa: E731
    u8, f32 = (lambda *s: t(torch.uint8, *s)), (lambda *s: t(torch.float32, *s))  # noqa: E731
    pair = lambda r, c: [(*r, c // 2), (*r, c // 16)]  # noqa: E731
    x, w, offs = t(torch.bfloat16, m, n), t(torch.bfloat16, e, n, k), t(torch.int32, e)
    cols = (u8(n, m // 2), u8(n, m // 16), u8(k, m // 2), u8(k, m // 16))
    cases = {"nvfp4_train_group_amax": ((x, offs, 0, True), [(e, 2)]),
             "nvfp4_train_quantize_row_col_grouped": ((x, f32(e, 2), offs, 0, None, None, None), pair((n,), m) + pair((m,), n)),
             "nvfp4_train_weight_amax_3d": ((w,), [(e,)]),
             "nvfp4_train_quantize_weight_3d": ((w, f32(e)), pair((e, n), k) + pair((e, k), n)),
             "nvfp4_scaled_grouped_mm": ((u8(m, k // 2), u8(m, k // 16), u8(e, n, k // 2), u8(e, n, k // 16), offs, f32(e), f32(e)), [(m, n)]),
             "nvfp4_grouped_mm_wgrad": ((*cols, f32(e), f32(e), offs), [(e, n, k)])}
    for name, (args, shapes) in cases.items():
        out = getattr(torch.ops.ao_mi355, name)(*args)
        assert [tuple(o.shape) for o in (out if isinstance(out, (tuple, list)) else (out,))] == shapes, name
        assert name in ops.__all__ and callable(getattr(ops, name)) and getattr(_lib.lib(), "ao_" + name) is not None
    assert torch.ops.ao_mi355.nvfp4_grouped_mm_wgrad(*cols, f32(1), f32(1), None).shape == (1, n, k)
    for name in G.__all__:
        assert name in prototype.__all__ and getattr(prototype, name) is getattr(G, name)
