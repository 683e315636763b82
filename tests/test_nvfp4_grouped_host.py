"""CPU: the NVFP4 grouped GEMM's restatement against the fixture written from the reference (tests/nvfp4_grouped_ref.py,
tests/golden/nvfp4_grouped.npz), the host route, the argument checks of the C ABI, NVFP4ExpertWeights' own checks and the fake kernels.
No kernel is launched in this file."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nvfp4_grouped_ref as G  # noqa: E402
import nvfp4_ref as R  # noqa: E402

from ao_amd import _lib, ops  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "nvfp4_grouped.npz"))
with open(os.path.join(os.path.dirname(HERE), "include", "ao_mi355.h")) as fh:
    HEADER = fh.read()
SEAM = int(re.search(r"#define AO_NVFP4_GROUPED_STREAM_MAX_ROWS (\d+)", HEADER).group(1))
STREAM, TILE = "nvfp4_grouped_stream_kernel", "nvfp4_grouped_tile_kernel"
NEW = ["ao_nvfp4_grouped_mm", "ao_nvfp4_group_amax_scale", "ao_nvfp4_quantize_grouped", "ao_nvfp4_grouped_mm_route",
       "ao_nvfp4_grouped_mm_kernel_name", "ao_nvfp4_grouped_mm_set_form"]
KINDS = [0, 1]


def _bf(name):
    return torch.from_numpy(GOLDEN[name].view(np.int16).copy()).view(torch.bfloat16)


def _u8(name):
    return torch.from_numpy(GOLDEN[name].copy())


def _f32(name):
    return torch.from_numpy(np.asarray(GOLDEN[name], dtype=np.float32).copy())


# ---- the restatement against the reference's bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p", "nop"])
def test_the_helper_casts_and_dequantizes_3d_weights_as_the_reference(tag):
    """to_nvfp4(w3d, per_tensor_scale=[E, 1, 1]) is the 2-D cast of the [E N, K] view with one group an expert."""
    w = _bf("w3_w")
    E, N, K = w.shape
    offs = G.offs_of([N] * E)
    p = G.group_amax_scale(w.reshape(E * N, K), offs)
    assert torch.equal(p.view(torch.int32), _f32("w3_p").view(torch.int32)) and len(set(p.tolist())) == E
    q, s = G.cast(w.reshape(E * N, K), offs, p if tag == "p" else None)
    assert torch.equal(q.reshape(E, N, K // 2), _u8(f"w3_{tag}_q")) and torch.equal(s.reshape(E, N, K // 16), _u8(f"w3_{tag}_s"))
    deq = G.dequantize(_u8(f"w3_{tag}_q"), _u8(f"w3_{tag}_s"), p if tag == "p" else None)
    assert torch.equal(R.bits(deq), R.bits(_bf(f"w3_{tag}_deq")))


@pytest.mark.parametrize("tag", ["p", "nop"])
def test_the_helper_reproduces_the_recorded_weight_only_outputs(tag):
    sizes = GOLDEN["gw_sizes"].tolist()
    assert 0 in sizes
    y = G.wo_linear(_bf("gw_x"), _u8("gw_q"), _u8("gw_s"), G.offs_of(sizes), _f32("gw_p") if tag == "p" else None)
    assert torch.equal(R.bits(y), R.bits(_bf(f"gw_{tag}_y")))
    assert not torch.equal(R.bits(_bf("gw_p_y")), R.bits(_bf("gw_nop_y")))


def test_the_helper_reproduces_the_recorded_emulation():
    """The activation codes are the reference cast's; the sums are exact in fp32 (blocks of e2m1 values times 1 or 2 against block scales
    in {1/4 .. 2}), so the emulation's bf16 GEMM and the chain round the same number once."""
    offs = G.offs_of(GOLDEN["gw_sizes"].tolist())
    q, s = R.cast(_bf("ge_x"))
    assert torch.equal(q, _u8("ge_aq")) and torch.equal(s, _u8("ge_as"))
    m64, S = G.mm_sums(_u8("ge_aq"), _u8("ge_as"), _u8("gw_q"), _u8("gw_s"), offs)
    assert float(S.max()) <= 2.0 ** 24 * 2.0 ** -4
    y = G.mm(_u8("ge_aq"), _u8("ge_as"), _u8("gw_q"), _u8("gw_s"), offs)
    assert torch.equal(R.bits(y), R.bits(_bf("ge_y")))


def test_groups_skip_empty_and_non_increasing_pairs():
    assert list(G.groups(torch.tensor([129, 129, 200]))) == [(0, 0, 129), (2, 129, 200)]
    assert list(G.groups(torch.tensor([0, 0, 40]))) == [(2, 0, 40)]
    assert G.offs_of([2, 0, 5]).tolist() == [2, 2, 7] and G.offs_of([2, 0, 5]).dtype == torch.int32


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_every_new_header_symbol_has_a_signature():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    after = HEADER[HEADER.index("NVFP4 grouped GEMM for MoE experts"):]
    in_block = sorted(set(re.findall(r"\b(ao_nvfp4_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", after, flags=re.S))))
    assert in_block == sorted(NEW)
    for name in NEW:
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    assert lib.ao_nvfp4_grouped_mm_kernel_name.restype is ctypes.c_char_p
    for name in ("nvfp4_grouped_mm", "nvfp4_group_amax_scale", "nvfp4_quantize_grouped", "nvfp4_grouped_mm_route",
                 "nvfp4_grouped_mm_kernel_name", "nvfp4_grouped_mm_set_form"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    from ao_amd import prototype

    assert callable(prototype.nvfp4_grouped_mm) and prototype.NVFP4ExpertWeights.__name__ in prototype.__all__
    assert "#define AO_MI355_ABI_VERSION 2" in HEADER


def _by_seam(m_total, e):
    """the product route: the header's seam on the mean group size ceil(M_total / E)"""
    return STREAM if (m_total + e - 1) // e <= SEAM else TILE


@pytest.mark.parametrize("kind", KINDS)
def test_route_on_the_mean_group_size(kind):
    assert 0 <= SEAM <= 512
    # the seam sits on ceil(M_total / E), tail rows included: the last M_total of the stream form, the mean rounded up, the first beyond
    for m in sorted({SEAM * 4, max(SEAM * 4 - 3, 0), SEAM * 4 + 1, 0, 1, 64, 16 * 4, 16 * 4 + 1, 2048}):
        assert ops.nvfp4_grouped_mm_kernel_name(kind, m, 130, 256, 4) == _by_seam(m, 4), m
        assert ops.nvfp4_grouped_mm_route(kind, m, 130, 256, 4)["kernel"] == _by_seam(m, 4), m
    assert ops.nvfp4_grouped_mm_kernel_name(kind, SEAM * 4, 130, 256, 4) == STREAM
    assert ops.nvfp4_grouped_mm_kernel_name(kind, SEAM * 4 + 1, 130, 256, 4) == TILE
    assert ops.nvfp4_grouped_mm_kernel_name(kind, 64, 4096, 7168, 32) == _by_seam(64, 32)
    assert ops.nvfp4_grouped_mm_kernel_name(kind, 16384, 4096, 7168, 32) == TILE  # mean 512 rows
    # the tiled form: grid (ceil(N / 64), ceil(M_total / 64) + E), up to 65535 rows
    m = SEAM * 4 + 1
    assert ops.nvfp4_grouped_mm_route(kind, m, 130, 256, 4) == {"kernel": TILE, "waves": 4, "m_tiles": 4, "tile_m": 64, "tile_n": 64,
                                                                "grid": (3, (m + 63) // 64 + 4)}
    assert ops.nvfp4_grouped_mm_route(kind, 16384, 4096, 7168, 32) == {"kernel": TILE, "waves": 4, "m_tiles": 4, "tile_m": 64, "tile_n": 64,
                                                                      "grid": (64, 256 + 32)}
    assert ops.nvfp4_grouped_mm_route(kind, 64 * 60000, 16, 16, 5535)["grid"] == (1, 65535)
    assert ops.nvfp4_grouped_mm_route(kind, 64 * 60000 + 1, 16, 16, 5535)["kernel"] == "invalid"
    assert ops.nvfp4_grouped_mm_route(kind, 0, 16, 16, 5)["kernel"] == STREAM  # a mean of 0 rows is below any seam (never launched)
    try:
        ops.nvfp4_grouped_mm_set_form(2)
        assert ops.nvfp4_grouped_mm_kernel_name(kind, 64, 4096, 7168, 32) == TILE
        assert ops.nvfp4_grouped_mm_route(kind, 64, 4096, 7168, 32)["grid"] == (64, 1 + 32)
        # the streaming form: grid (ceil(N / 16), E), m-tiles and waves of the stream plan at the MEAN group size
        ops.nvfp4_grouped_mm_set_form(1)
        assert ops.nvfp4_grouped_mm_kernel_name(kind, 16384, 4096, 7168, 32) == STREAM
        r = ops.nvfp4_grouped_mm_route(kind, 64, 4096, 7168, 32)  # mean 2 rows: one m-tile; 256 column tiles: 8 waves
        assert r == {"kernel": STREAM, "waves": 8, "m_tiles": 1, "tile_m": 16, "tile_n": 16, "grid": (256, 32)}
        assert ops.nvfp4_grouped_mm_route(kind, 16 * 4, 130, 256, 4) == {"kernel": STREAM, "waves": 2, "m_tiles": 1, "tile_m": 16, "tile_n": 16,
                                                                        "grid": (9, 4)}
        r = ops.nvfp4_grouped_mm_route(kind, 17 * 3, 257, 1152, 3)  # a mean of 17 rows: two m-tiles
        assert (r["m_tiles"], r["waves"], r["tile_m"], r["grid"]) == (2, 8, 32, (17, 3))
        assert ops.nvfp4_grouped_mm_route(kind, 17 * 3 - 2, 257, 1152, 3)["m_tiles"] == 2  # ceil(49 / 3) = 17
        assert ops.nvfp4_grouped_mm_route(kind, 16384, 4096, 7168, 32) == {"kernel": STREAM, "waves": 8, "m_tiles": 4, "tile_m": 64, "tile_n": 16,
                                                                          "grid": (256, 32)}
    finally:
        ops.nvfp4_grouped_mm_set_form(0)
    assert ops.nvfp4_grouped_mm_kernel_name(kind, 16384, 4096, 7168, 32) == TILE
    # the dense family's forced form is its own, and the grouped one leaves the dense route alone
    try:
        ops.nvfp4_set_form(1)
        assert ops.nvfp4_grouped_mm_kernel_name(kind, 16384, 4096, 7168, 32) == TILE
        ops.nvfp4_set_form(0)
        ops.nvfp4_grouped_mm_set_form(2)
        assert ops.nvfp4_linear_kernel_name(kind, 4, 4096, 7168) == "nvfp4_stream_kernel"
    finally:
        ops.nvfp4_set_form(0)
        ops.nvfp4_grouped_mm_set_form(0)


# (M_total, N, K, E): K = 8, K = 24, K = 0, E = 0, E = 65536, N K and M_total K past 2^31, N = 0, M_total < 0
BAD = [(4, 16, 8, 2), (4, 16, 24, 2), (4, 16, 0, 2), (4, 16, 16, 0), (4, 16, 16, 65536), (4, 1 << 19, 1 << 12, 2), (1 << 20, 16, 1 << 12, 2),
       (4, 0, 16, 2), (-1, 16, 16, 2)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bad", BAD)
def test_bad_shapes_are_invalid(bad, kind):
    assert ops.nvfp4_grouped_mm_route(kind, *bad)["kernel"] == "invalid"
    assert ops.nvfp4_grouped_mm_kernel_name(kind, *bad) == "invalid"
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert lib.ao_nvfp4_grouped_mm(kind, p, p, p, p, p, None, p, p, p, *bad, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "ao_nvfp4_grouped_mm: bad kind or shape" in lib.ao_last_error().decode()


def test_bad_kind_is_invalid():
    assert ops.nvfp4_grouped_mm_route(2, 4, 16, 16, 2)["kernel"] == "invalid"
    assert ops.nvfp4_grouped_mm_kernel_name(-1, 4, 16, 16, 2) == "invalid"


def test_whole_weight_may_pass_2_to_the_31():
    # 256 unsharded experts of [4096, 7168]: 7.5 G weights; only the per-expert N K is bounded
    assert ops.nvfp4_grouped_mm_kernel_name(0, 64, 4096, 7168, 256) == _by_seam(64, 256)
    assert ops.nvfp4_grouped_mm_route(0, 256 * 512, 4096, 7168, 256)["grid"] == (64, 2048 + 256)


def test_argument_checks_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    mm = lib.ao_nvfp4_grouped_mm
    INV, NUL, OK = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_ERR_NULL_POINTER, _lib.AO_OK
    # kind, x, a, a_scale, b, b_scale, pa, pb, offs, out
    needed = {0: (0, 3, 4, 7, 8), 1: (1, 2, 3, 4, 7, 8)}
    for kind in KINDS:
        for i in needed[kind]:
            args = [p, p, p, p, p, None, None, p, p]
            args[i] = None
            assert mm(kind, *args, 4, 16, 32, 2, None) == NUL, (kind, i)
            assert "ao_nvfp4_grouped_mm: null pointer" in lib.ao_last_error().decode()
    assert mm(0, p, None, None, p, p, p, p, p, p, 4, 16, 32, 2, None) == INV  # the weight-only kind takes no pa
    assert "no activation scale" in lib.ao_last_error().decode()
    assert mm(0, p + 8, None, None, p, p, None, p, p, p, 4, 16, 32, 2, None) == INV  # x not 16-byte aligned
    assert mm(1, None, p + 8, p, p, p, None, p, p, p, 4, 16, 32, 2, None) == INV  # codes not 16-byte aligned (K % 32 == 0)
    assert mm(1, None, p, p, p + 8, p, None, p, p, p, 4, 16, 32, 2, None) == INV
    assert mm(1, None, p, p + 1, p, p, None, p, p, p, 4, 16, 32, 2, None) == INV  # block scales not 2-byte aligned
    assert mm(1, None, p + 4, p, p, p, None, p, p, p, 4, 16, 48, 2, None) == INV  # K % 32 != 0: 8-byte
    assert mm(1, None, p, p, p, p, p + 2, p, p, p, 4, 16, 32, 2, None) == INV  # per-expert scales not 4-byte aligned
    assert mm(1, None, p, p, p, p, None, p, p + 2, p, 4, 16, 32, 2, None) == INV  # offs not 4-byte aligned
    assert "ao_nvfp4_grouped_mm" in lib.ao_last_error().decode()
    for kind in KINDS:
        assert mm(kind, None, None, None, p, p, None, None, p, None, 0, 16, 32, 2, None) == OK  # M_total = 0: nothing to launch
    out = (ctypes.c_int32 * 7)()
    assert lib.ao_nvfp4_grouped_mm_route(0, 1, 16, 16, 1, None, 7) == NUL
    assert lib.ao_nvfp4_grouped_mm_route(0, 1, 16, 16, 1, out, 6) == INV
    assert lib.ao_nvfp4_grouped_mm_set_form(3) == INV and lib.ao_nvfp4_grouped_mm_set_form(-1) == INV
    # the grouped cast and amax
    amax, quant = lib.ao_nvfp4_group_amax_scale, lib.ao_nvfp4_quantize_grouped
    for shape in ((4, 8, 2), (4, 24, 2), (4, 16, 0), (4, 16, 65536), (-1, 16, 2)):
        assert amax(p, p, p, *shape, None) == INV and "ao_nvfp4_group_amax_scale: bad shape" in lib.ao_last_error().decode()
        assert quant(p, p, p, p, p, *shape, None) == INV and "ao_nvfp4_quantize_grouped: bad shape" in lib.ao_last_error().decode()
    assert amax(p, None, p, 4, 16, 2, None) == NUL and amax(p, p, None, 4, 16, 2, None) == NUL
    assert amax(p, p, p + 2, 4, 16, 2, None) == INV
    for i in (0, 2, 3, 4):  # x, offs, q, scale (p may be NULL)
        args = [p] * 5
        args[i] = None
        assert quant(*args, 4, 16, 2, None) == NUL, i
    assert quant(p + 8, p, p, p, p, 4, 16, 2, None) == INV and quant(p, p, p, p + 4, p, 4, 16, 2, None) == INV
    assert quant(None, None, p, None, None, 0, 16, 2, None) == OK


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    q, s = torch.zeros(2, 3, 16, dtype=torch.uint8), torch.zeros(2, 3, 2, dtype=torch.float8_e4m3fn)
    offs = torch.tensor([1, 2], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="nvfp4_grouped_mm: .*no CPU fallback"):
        ops.nvfp4_grouped_mm(0, torch.zeros(2, 32, dtype=torch.bfloat16), None, q, s, offs)
    with pytest.raises(RuntimeError, match="nvfp4_group_amax_scale: .*no CPU fallback"):
        ops.nvfp4_group_amax_scale(torch.zeros(2, 32, dtype=torch.bfloat16), offs)
    with pytest.raises(RuntimeError, match="nvfp4_quantize_grouped: .*no CPU fallback"):
        ops.nvfp4_quantize_grouped(torch.zeros(2, 32, dtype=torch.bfloat16), None, offs)


def test_expert_weights_check_their_tensors():
    from ao_amd.prototype import NVFP4ExpertWeights, NVFP4Tensor

    q, s = torch.zeros(3, 20, 24, dtype=torch.uint8), torch.zeros(3, 20, 3, dtype=torch.float8_e4m3fn)
    p = torch.tensor([0.5, 0.25, 2.0])
    w = NVFP4ExpertWeights(q, s, p.reshape(3, 1, 1), p * 2)
    assert w.shape == torch.Size((3, 20, 48)) and len(w) == 3 and tuple(w.per_tensor_scale.shape) == (3,)
    t = w[1]
    assert isinstance(t, NVFP4Tensor) and tuple(t.shape) == (20, 48) and t.per_tensor_scale.dim() == 0 and t.act_per_tensor_scale.dim() == 0
    assert t.per_tensor_scale.item() == 0.25 and t.act_per_tensor_scale.item() == 0.5 and t.is_swizzled_scales is False
    assert NVFP4ExpertWeights(q, s)[2].per_tensor_scale is None
    assert tuple(w.dequantize().shape) == (3, 20, 48) and w.dequantize().dtype == torch.bfloat16
    bad = [((q[0], s[0]), "qdata must be uint8 \\[E, N, K/2\\]"),
           ((q.to(torch.int8), s), "qdata must be uint8"),
           ((torch.zeros(3, 20, 20, dtype=torch.uint8), s), "K must be a positive multiple of 16"),
           ((q, s.view(torch.uint8)), "scale must be float8_e4m3fn"),
           ((q, torch.zeros(3, 20, 4, dtype=torch.float8_e4m3fn)), "scale must be float8_e4m3fn \\[E, N, K/16\\] = \\(3, 20, 3\\)"),
           ((q, s, torch.tensor(0.5)), "per_tensor_scale must have shape \\[E\\] or \\[E, 1, 1\\]"),
           ((q, s, p[:2]), "per_tensor_scale must have shape"),
           ((q, s, p.double()), "per_tensor_scale must be a float32 tensor"),
           ((q, s, None, torch.ones(1, 3)), "act_per_tensor_scale must have shape")]
    for args, why in bad:
        with pytest.raises(ValueError, match="NVFP4ExpertWeights: " + why):
            NVFP4ExpertWeights(*args)
    with pytest.raises(ValueError, match="from_hp: w must be a 3-D bfloat16 tensor"):
        NVFP4ExpertWeights.from_hp(torch.zeros(3, 20, 48))
    with pytest.raises(ValueError, match="from_hp: .*K a positive multiple of 16"):
        NVFP4ExpertWeights.from_hp(torch.zeros(3, 20, 40, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="no experts given"):
        NVFP4ExpertWeights.from_nvfp4_tensors([])
    a, b = NVFP4Tensor(q[0], s[0], 16, torch.bfloat16, p[0]), NVFP4Tensor(q[1], s[1], 16, torch.bfloat16)
    with pytest.raises(ValueError, match="per_tensor_scale must be set on every expert or on none"):
        NVFP4ExpertWeights.from_nvfp4_tensors([a, b])
    st = NVFP4ExpertWeights.from_nvfp4_tensors([a, NVFP4Tensor(q[1], s[1], 16, torch.bfloat16, p[1])])
    assert st.shape == torch.Size((2, 20, 48)) and st.per_tensor_scale.tolist() == [0.5, 0.25] and st.act_per_tensor_scale is None


def test_expert_weights_from_the_reference_layout_unswizzle_per_expert():
    from ao_amd.prototype import NVFP4ExpertWeights

    g = torch.Generator().manual_seed(3)
    E, N, K = 2, 20, 80
    q = torch.randint(0, 256, (E, N, K // 2), generator=g).to(torch.uint8)
    rm = torch.randint(0, 120, (E, N, K // 16), generator=g).to(torch.uint8)
    rb, cb = (N + 127) // 128, (K // 16 + 3) // 4
    sw = torch.zeros(E, rb * cb * 512, dtype=torch.uint8)
    for e in range(E):
        for r in range(N):
            for c in range(K // 16):
                sw[e, ((r // 128) * cb + c // 4) * 512 + (r % 32) * 16 + (r % 128 // 32) * 4 + c % 4] = rm[e, r, c]
    w = NVFP4ExpertWeights.from_reference_layout(q, sw.view(torch.float8_e4m3fn))
    assert torch.equal(w.scale.view(torch.uint8), rm) and torch.equal(w.qdata, q)
    for e in range(E):
        assert torch.equal(R.unswizzle(sw[e], N, K // 16), rm[e])


def test_grouped_mm_refusals_carry_the_reason():
    from ao_amd.prototype import NVFP4ExpertWeights, nvfp4_grouped_mm

    w = NVFP4ExpertWeights(torch.zeros(3, 20, 24, dtype=torch.uint8), torch.zeros(3, 20, 3, dtype=torch.float8_e4m3fn))
    offs = torch.tensor([1, 2, 4], dtype=torch.int32)
    x = torch.zeros(4, 48, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="takes bfloat16 activations, got torch.float32"):
        nvfp4_grouped_mm(x.float(), w, offs)
    with pytest.raises(ValueError, match="A must be a 2-D tensor"):
        nvfp4_grouped_mm(x.reshape(2, 2, 48), w, offs)
    with pytest.raises(ValueError, match="are not compatible"):
        nvfp4_grouped_mm(x[:, :32], w, offs)
    with pytest.raises(ValueError, match="offs must be int32 \\[E\\] = \\[3\\]"):
        nvfp4_grouped_mm(x, w, offs[:2])
    with pytest.raises(ValueError, match="offs must be int32"):
        nvfp4_grouped_mm(x, w, offs.long())
    with pytest.raises(ValueError, match="experts must be an NVFP4ExpertWeights"):
        nvfp4_grouped_mm(x, torch.zeros(3, 20, 48, dtype=torch.bfloat16), offs)
    with pytest.raises(ValueError, match="weight_only casts no activation"):
        nvfp4_grouped_mm(x, w, offs, weight_only=True, use_dynamic_per_group_scale=True)
    with pytest.raises(ValueError, match="only bfloat16 out_dtype"):
        nvfp4_grouped_mm(x, w, offs, out_dtype=torch.float32)


def test_fake_kernels_trace_shapes():
    import ao_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        d = "cuda"
        x = torch.empty(7, 80, dtype=torch.bfloat16, device=d)
        offs = torch.empty(3, dtype=torch.int32, device=d)
        wq, ws = torch.empty(3, 130, 40, dtype=torch.uint8, device=d), torch.empty(3, 130, 5, dtype=torch.float8_e4m3fn, device=d)
        pe = torch.empty(3, device=d)
        p = torch.ops.ao_mi355.nvfp4_group_amax_scale(x, offs)
        assert p.shape == (3,) and p.dtype == torch.float32
        q, s = torch.ops.ao_mi355.nvfp4_quantize_grouped(x, p, offs)
        assert q.shape == (7, 40) and q.dtype == torch.uint8 and s.shape == (7, 5) and s.dtype == torch.float8_e4m3fn
        y = torch.ops.ao_mi355.nvfp4_grouped_mm(1, q, s, wq, ws, offs, p, pe)
        assert y.shape == (7, 130) and y.dtype == torch.bfloat16
        y = torch.ops.ao_mi355.nvfp4_grouped_mm(0, x, None, wq, ws, offs, None, None)
        assert y.shape == (7, 130) and y.dtype == torch.bfloat16
