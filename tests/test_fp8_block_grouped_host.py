"""CPU: the blockwise float8 grouped GEMM's numpy restatement against the fixture written from the reference
(tests/fp8_block_grouped_ref.py, tests/golden/fp8_block_grouped.npz), the host route, the argument checks of the C ABI and the fake
kernel.  No kernel is launched in this file."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fp8_block_grouped_ref as G  # noqa: E402
import fp8_block_ref as R  # noqa: E402

from ao_amd import _lib, ops  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "fp8_block_grouped.npz"))
with open(os.path.join(os.path.dirname(HERE), "include", "ao_mi355.h")) as fh:
    SEAM = int(re.search(r"#define AO_FP8_BLOCK_GROUPED_STREAM_MAX_ROWS (\d+)", fh.read()).group(1))
STREAM, TILE = "fp8_block_grouped_stream_kernel", "fp8_block_grouped_tile_kernel"
NEW = ["ao_fp8_block_grouped_mm", "ao_fp8_block_grouped_mm_route", "ao_fp8_block_grouped_mm_kernel_name", "ao_fp8_block_grouped_mm_set_form"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_fp8_block_grouped", os.path.join(HERE, "golden", "make_golden_fp8_block_grouped.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ---- the restatement against the reference's bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B"])
def test_the_helpers_casts_equal_the_fixture(case):
    gen = _generator()
    sizes, N, K, seed = gen.CASES[case]
    np.testing.assert_array_equal(GOLDEN[f"{case}_offs"], G.offs_of(sizes))
    q, s = R.cast_1x128(GOLDEN[f"{case}_x"])
    assert R.same_codes(q, GOLDEN[f"{case}_aq"])
    np.testing.assert_array_equal(s, GOLDEN[f"{case}_as"])
    w, _ = gen.weights(seed, len(sizes), N, K)  # the weights are drawn again, not stored
    wq, ws = G.cast_experts(_bits(w))
    assert R.same_codes(wq, GOLDEN[f"{case}_wq"])
    np.testing.assert_array_equal(ws, GOLDEN[f"{case}_ws"])


@pytest.mark.parametrize("case", ["A", "B"])
def test_the_chain_is_no_farther_from_float64_than_the_emulation(case):
    aq, a_s, wq, ws, offs = (GOLDEN[f"{case}_{k}"] for k in ("aq", "as", "wq", "ws", "offs"))
    y64, S = G.grouped_f64(aq, a_s, wq, ws, offs)
    rows = int(offs[-1])
    assert rows == aq.shape[0] and float(np.abs(y64).sum()) > 0
    chain = G.l2_to(y64, G.grouped_chain_bits(aq, a_s, wq, ws, offs), rows)
    emulated = G.l2_to(y64, GOLDEN[f"{case}_emulated"], rows)
    print(f"case {case}: l2 to float64: chain {chain:.5g}, emulated {emulated:.5g} ({20 * np.log10(emulated / chain):.2f} dB)")
    assert chain <= emulated


def test_groups_clamp_and_skip_like_the_kernel():
    assert G.groups([129, 129, 200], 200) == [(0, 0, 129), (2, 129, 200)]
    assert G.groups([0, 0, 40], 40) == [(2, 0, 40)]
    assert G.groups([5, 3, 300, -1], 10) == [(0, 0, 5), (2, 3, 10)]  # a non-increasing pair is empty; bounds clamp to [0, M_total]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_exports_the_new_symbols():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW:
        assert hasattr(lib, name) and name in declared and name in _lib._SIGNATURES
    for name in ("fp8_block_grouped_mm", "fp8_block_grouped_mm_route", "fp8_block_grouped_mm_kernel_name", "fp8_block_grouped_mm_set_form"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    from ao_amd import prototype

    assert callable(prototype.fp8_blockwise_grouped_mm) and prototype.Float8BlockwiseExpertWeights.__name__ in prototype.__all__


def test_route_on_the_mean_group_size():
    assert SEAM == 16
    r = ops.fp8_block_grouped_mm_route(64, 4096, 7168, 32)  # mean 2 rows: one m-tile; 256 column tiles: 8 waves
    assert r == {"kernel": STREAM, "waves": 8, "m_tiles": 1, "tile_m": 16, "tile_n": 16, "grid": (256, 32)}
    r = ops.fp8_block_grouped_mm_route(16384, 4096, 7168, 32)  # mean 512 rows
    assert r == {"kernel": TILE, "waves": 4, "m_tiles": 4, "tile_m": 128, "tile_n": 128, "grid": (32, 128 + 32)}
    assert ops.fp8_block_grouped_mm_kernel_name(64, 4096, 7168, 32) == STREAM
    assert ops.fp8_block_grouped_mm_kernel_name(16384, 4096, 7168, 32) == TILE
    # the seam sits on ceil(M_total / E)
    assert ops.fp8_block_grouped_mm_kernel_name(SEAM * 4, 130, 256, 4) == STREAM
    assert ops.fp8_block_grouped_mm_kernel_name(SEAM * 4 - 3, 130, 256, 4) == STREAM
    assert ops.fp8_block_grouped_mm_kernel_name(SEAM * 4 + 1, 130, 256, 4) == TILE
    assert ops.fp8_block_grouped_mm_route(SEAM * 4, 130, 256, 4) == {"kernel": STREAM, "waves": 2, "m_tiles": 1, "tile_m": 16, "tile_n": 16,
                                                                      "grid": (9, 4)}
    assert ops.fp8_block_grouped_mm_route(SEAM * 4 + 1, 130, 256, 4) == {"kernel": TILE, "waves": 4, "m_tiles": 4, "tile_m": 128, "tile_n": 128,
                                                                          "grid": (2, 1 + 4)}
    assert ops.fp8_block_grouped_mm_route(0, 16, 128, 5)["kernel"] == STREAM
    # the tile form's grid rows: ceil(M_total / 128) + E, up to 65535
    assert ops.fp8_block_grouped_mm_route(128 * 60000, 128, 128, 5535)["grid"] == (1, 65535)
    assert ops.fp8_block_grouped_mm_route(128 * 60000 + 1, 128, 128, 5535)["kernel"] == "invalid"
    try:
        ops.fp8_block_grouped_mm_set_form(2)
        assert ops.fp8_block_grouped_mm_kernel_name(64, 4096, 7168, 32) == TILE
        assert ops.fp8_block_grouped_mm_route(64, 4096, 7168, 32)["grid"] == (32, 1 + 32)
        ops.fp8_block_grouped_mm_set_form(1)
        assert ops.fp8_block_grouped_mm_kernel_name(16384, 4096, 7168, 32) == STREAM
        r = ops.fp8_block_grouped_mm_route(17 * 3, 257, 1152, 3)  # the stream plan at a mean of 17 rows: two m-tiles
        assert (r["m_tiles"], r["waves"], r["tile_m"], r["grid"]) == (2, 8, 32, (17, 3))
        assert ops.fp8_block_grouped_mm_route(16384, 4096, 7168, 32) == {"kernel": STREAM, "waves": 8, "m_tiles": 4, "tile_m": 64, "tile_n": 16,
                                                                         "grid": (256, 32)}
    finally:
        ops.fp8_block_grouped_mm_set_form(0)
    assert ops.fp8_block_grouped_mm_kernel_name(16384, 4096, 7168, 32) == TILE
    # the dense family's forced form is its own
    try:
        ops.fp8_block_linear_set_form(2)
        assert ops.fp8_block_grouped_mm_kernel_name(64, 4096, 7168, 32) == STREAM
    finally:
        ops.fp8_block_linear_set_form(0)


@pytest.mark.parametrize("bad", [(4, 16, 64, 2), (4, 16, 192, 2), (4, 16, 0, 2), (4, 16, 128, 0), (4, 16, 128, 65536), (4, 1 << 19, 1 << 12, 2),
                                 (1 << 20, 16, 1 << 12, 2), (4, 0, 128, 2), (-1, 16, 128, 2)])
def test_bad_shapes_are_invalid(bad):
    assert ops.fp8_block_grouped_mm_route(*bad)["kernel"] == "invalid"
    assert ops.fp8_block_grouped_mm_kernel_name(*bad) == "invalid"
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert lib.ao_fp8_block_grouped_mm(p, p, p, p, p, p, *bad, None) == _lib.AO_ERR_INVALID_ARGUMENT
    assert "ao_fp8_block_grouped_mm: bad shape" in lib.ao_last_error().decode()


def test_whole_weight_may_pass_2_gib():
    # DeepSeek-V3's 256 unsharded experts, gate and up merged: 7.5 GB of codes; only the per-expert N K is bounded
    assert ops.fp8_block_grouped_mm_kernel_name(64, 4096, 7168, 256) == STREAM
    assert ops.fp8_block_grouped_mm_route(256 * 512, 4096, 7168, 256)["grid"] == (32, 1024 + 256)


def test_argument_checks_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    mm = lib.ao_fp8_block_grouped_mm
    INV, NUL = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_ERR_NULL_POINTER
    for i in range(6):  # a, a_scale, b, b_scale, offs, out
        args = [p] * 6
        args[i] = None
        assert mm(*args, 4, 16, 128, 2, None) == NUL, i
        assert "ao_fp8_block_grouped_mm: null pointer" in lib.ao_last_error().decode()
    assert mm(p + 8, p, p, p, p, p, 4, 16, 128, 2, None) == INV  # codes not 16-byte aligned
    assert mm(p, p, p + 8, p, p, p, 4, 16, 128, 2, None) == INV
    assert mm(p, p + 2, p, p, p, p, 4, 16, 128, 2, None) == INV  # scales not 4-byte aligned
    assert mm(p, p, p, p, p + 2, p, 4, 16, 128, 2, None) == INV  # offs not 4-byte aligned
    assert "ao_fp8_block_grouped_mm" in lib.ao_last_error().decode()
    assert mm(None, None, p, p, p, None, 0, 16, 128, 2, None) == _lib.AO_OK  # M_total = 0: nothing to launch
    out = (ctypes.c_int32 * 7)()
    assert lib.ao_fp8_block_grouped_mm_route(1, 16, 128, 1, None, 7) == NUL
    assert lib.ao_fp8_block_grouped_mm_route(1, 16, 128, 1, out, 6) == INV
    assert lib.ao_fp8_block_grouped_mm_set_form(3) == INV and lib.ao_fp8_block_grouped_mm_set_form(-1) == INV


def test_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="fp8_block_grouped_mm: .*no CPU fallback"):
        ops.fp8_block_grouped_mm(torch.zeros(2, 128, dtype=torch.float8_e4m3fn), torch.ones(2, 1), torch.zeros(1, 16, 128, dtype=torch.float8_e4m3fn),
                                 torch.ones(1, 1, 1), torch.tensor([2], dtype=torch.int32))


def test_expert_weights_check_their_tensors():
    from ao_amd.prototype import Float8BlockwiseExpertWeights

    w = Float8BlockwiseExpertWeights(torch.zeros(3, 130, 256, dtype=torch.float8_e4m3fn), torch.ones(3, 2, 2))  # any N, as a checkpoint gives it
    assert w.shape == torch.Size((3, 256, 130))
    for data, scale in ((torch.zeros(130, 256, dtype=torch.float8_e4m3fn), torch.ones(2, 2)),
                        (torch.zeros(3, 130, 200, dtype=torch.float8_e4m3fn), torch.ones(3, 2, 2)),
                        (torch.zeros(3, 130, 256, dtype=torch.float8_e4m3fn), torch.ones(3, 1, 2)),
                        (torch.zeros(3, 130, 256, dtype=torch.uint8), torch.ones(3, 2, 2))):
        with pytest.raises(ValueError, match="Float8BlockwiseExpertWeights"):
            Float8BlockwiseExpertWeights(data, scale)


def test_fake_kernel_traces_shapes():
    import ao_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        y = torch.ops.ao_mi355.fp8_block_grouped_mm(torch.empty(7, 256, dtype=torch.float8_e4m3fn, device="cuda"), torch.empty(7, 2, device="cuda"),
                                                    torch.empty(3, 130, 256, dtype=torch.float8_e4m3fn, device="cuda"),
                                                    torch.empty(3, 2, 2, device="cuda"), torch.empty(3, dtype=torch.int32, device="cuda"))
        assert y.shape == (7, 130) and y.dtype == torch.bfloat16

