"""The balanced grid of the one-row int4 kernel: left-over n-tiles run as two half-tile workgroups that meet through the
split-K workspace.  The result is the whole-tile grid's, bit for bit -- the last arriver adds the eight per-wave partials in wave order --
so every GPU check here is an equality.  The CPU half pins the rule's arithmetic and that the first ten route fields did not move."""
import ctypes

import pytest
import torch

import route_cases as rc
from ao_amd import _lib

OFF, ON = 981, 982  # ao_int4_set_tuning: the balanced grid never / wherever the form allows
LLAMA = {"qkv": (6144, 4096), "o": (4096, 4096), "gate": (14336, 4096), "up": (14336, 4096), "down": (4096, 14336)}
# shapes of the form (one row, K = 4096) whose left-over count under the forced mode differs from the product's rule: a single left-over
# tile behind whole rounds, every tile left over (fewer tiles than CUs), and more than one round with an odd rest
SMALL = ((4112, 4096), (384, 4096), (16, 4096), (8400, 4096))
GROUPS = (32, 64, 128, 256)


def _route11(lib, m, n, k, g):
    out = (ctypes.c_int32 * 11)()
    assert lib.ao_int4_mm_route(m, n, k, g, out, 11) == 0
    return list(out)


# ---- CPU: the rule and the route query -------------------------------------------------------------------------------------------
def test_rule_arithmetic():
    lib = _lib.lib()
    h = lib.ao_int4_balanced_halves
    # T tiles on C CUs: r = T mod C tiles are cut when C < T <= 4 C and 2 r = C
    assert h(896, 256, 0) == 128 and h(384, 256, 0) == 128  # gate / up, qkv on the MI355X
    assert h(256, 256, 0) == 0  # o: even
    assert h(1792, 256, 0) == 0  # merged gate_up: 7 per CU, two rounds
    assert h(128, 256, 0) == 0  # T <= C: not a left-over behind whole rounds
    assert h(640, 256, 0) == 128 and h(1152, 256, 0) == 0  # 2.5 per CU: one round; 4.5 per CU: not resident at once
    assert h(257, 256, 0) == 0 and h(320, 256, 0) == 0 and h(448, 256, 0) == 0  # r = 1, C / 4, 3 C / 4: not measured, today's grid
    assert h(456, 304, 0) == 152 and h(384, 304, 0) == 0  # another CU count: the rule follows C, not the literal 256
    assert h(96, 64, 0) == 32 and h(96, 63, 0) == 0  # 2 r = C needs an even C
    assert h(0, 256, 0) == 0 and h(896, 0, 0) == 0 and h(-16, 256, 1) == 0
    # forced: any left-over count
    assert h(257, 256, 1) == 1 and h(24, 256, 1) == 24 and h(525, 256, 1) == 13 and h(512, 256, 1) == 0


def test_route_reports_the_halves_in_slot_eleven():
    lib = _lib.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    for g in GROUPS:
        for name, (n, k) in LLAMA.items():
            r = _route11(lib, 1, n, k, g)
            want = lib.ao_int4_balanced_halves(n // 16, cus, 0) if k == 4096 else 0
            assert r[10] == want, (name, g, r)
            assert r[8] == 1, "the balanced grid is not a K split: `split` stays 1"
            if cus == 256:
                assert r[10] == {"qkv": 128, "gate": 128, "up": 128}.get(name, 0), (name, g, r)
        assert _route11(lib, 1, 28672, 4096, g)[10] == 0  # merged gate_up
        for m in (2, 4, 16, 128):
            assert _route11(lib, m, 14336, 4096, g)[10] == 0  # one row only
    assert lib.ao_int4_mm_kernel_name(1, 14336, 4096, 128) == b"int4_mm_kernel"


def test_first_ten_route_fields_are_the_ten_field_query():
    """Every int4 case of route_cases: the eleven-field query's first ten fields equal the ten-field query's, which test_route_coverage pins
    against the committed signatures; a ten-field buffer is not written past its end."""
    lib = _lib.lib()
    seen = 0
    for case, _ in rc.CASES:
        if case.family != "int4":
            continue
        out = (ctypes.c_int32 * 12)(*([-7] * 12))
        assert lib.ao_int4_mm_route(case.M, case.N, case.K, case.G, out, 10) == 0
        assert list(out)[10:] == [-7, -7]
        assert list(out)[:10] == _route11(lib, case.M, case.N, case.K, case.G)[:10]
        seen += 1
    assert seen > 20
    # the overrides steer launches only
    before = _route11(lib, 1, 14336, 4096, 128)
    for mode in (OFF, ON):
        lib.ao_int4_set_tuning(0, mode)
        try:
            assert lib.ao_int4_overridden() == 1
            assert _route11(lib, 1, 14336, 4096, 128) == before
        finally:
            lib.ao_int4_set_tuning(0, 0)
    assert lib.ao_int4_overridden() == 0


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _case(n, k, g, seed):
    from ao_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16, generator=gen) * 0.02
    q, sz = ops.int4_quantize_tinygemm(w, g)
    x = torch.randn(1, k, device="cuda", dtype=torch.bfloat16, generator=gen)
    return x, q, sz


def _mm(lib, mode, x, q, sz, g):
    from ao_amd import ops

    lib.ao_int4_set_tuning(0, mode)
    try:
        y = ops.weight_int4pack_mm(x, q, g, sz)
        torch.cuda.synchronize()
    finally:
        lib.ao_int4_set_tuning(0, 0)
    return y.view(torch.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("n,k", [LLAMA["qkv"], LLAMA["gate"], LLAMA["o"]] + list(SMALL))
def test_balanced_equals_whole_tile_grid_bit_for_bit(n, k, g):
    lib = _lib.lib()
    x, q, sz = _case(n, k, g, n + g)
    off = _mm(lib, OFF, x, q, sz, g)
    on = _mm(lib, ON, x, q, sz, g)
    assert torch.equal(on, off), f"{int((on != off).sum())} of {n} outputs differ"
    assert torch.equal(_mm(lib, 0, x, q, sz, g), off), "the product route"
    # a race in the meeting shows as a launch that differs from the first
    for i in range(20):
        again = _mm(lib, ON, x, q, sz, g)
        assert torch.equal(again, on), f"launch {i + 2}: {int((again != on).sum())} outputs differ from the first launch"


@pytest.mark.gpu
def test_tickets_reset_under_graph_replay():
    from ao_amd import ops

    lib = _lib.lib()
    n, k = LLAMA["gate"]
    x, q, sz = _case(n, k, 128, 5)
    want = _mm(lib, OFF, x, q, sz, 128)
    stream = torch.cuda.Stream()
    lib.ao_int4_set_tuning(0, ON)
    try:
        with torch.cuda.stream(stream):
            y = ops.weight_int4pack_mm(x, q, 128, sz)  # eager first: the workspace is allocated outside capture
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                y = ops.weight_int4pack_mm(x, q, 128, sz)
                y2 = ops.weight_int4pack_mm(x, q, 128, sz)  # two launches per replay share the tickets back to back
            for i in range(6):
                y.zero_()
                y2.zero_()
                graph.replay()
                stream.synchronize()
                assert torch.equal(y.view(torch.int16), want) and torch.equal(y2.view(torch.int16), want), f"replay {i + 1}"
    finally:
        lib.ao_int4_set_tuning(0, 0)
