"""The committed case list of the weight-only linears (tests/wo8_cases.py) covers every route the product can take, at its edges (CPU:
ao_wo8_linear_route is host logic)."""
import pytest

import wo8_cases as wc
from ao_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@pytest.fixture(scope="module")
def reach(lib):
    return wc.reachable(lib)


def test_the_grid_reaches_both_forms_and_every_m_tile_count(lib, reach):
    for fmt in wc.FMT:
        sigs = {s for s in reach if s[0] == fmt}
        assert {s[1] for s in sigs} == {"stream", "tile"}
        # (no K of the grid has 2 or 3 k steps: the pool adds the 2-wave workgroups)
        assert {s[2] for s in sigs if s[1] == "stream"} == {1, 4, 8, 16}
        assert {wc.signature(lib, c)[2] for c in wc.CASES if c[0] == fmt} == {1, 2, 4, 8, 16}
        assert {s[3] for s in sigs if s[1] == "stream"} == {1, 2, 4}


def test_every_reachable_signature_has_a_case(lib, reach):
    have = {wc.signature(lib, c) for c in wc.CASES}
    missing = sorted(s for s in reach if s not in have)
    assert not missing, f"no case runs {missing}"


def test_cases_meet_the_edge_requirements(lib):
    by_sig = {}
    for c in wc.CASES:
        by_sig.setdefault(wc.signature(lib, c), set()).update(wc.properties(lib, c))
    for sig, props in sorted(by_sig.items()):
        fmt, kernel, waves, mt = sig
        want = {"edge_lo", "edge_hi", "ragged_n", "small_n", "wide_n"}
        if kernel == "tile":
            want |= {"ragged_m", "k16", "partial_k"}
        else:
            if mt > 1:
                want.add("ragged_m")
            if waves == 1:
                want.add("k16")
            if waves > 1:
                want |= {"uneven_waves", "partial_k"}
        assert want <= props, f"{sig}: no case with {sorted(want - props)}"
    rows = {c[1] for c in wc.CASES}
    # M = 1, the stream form's last and the tiled form's first row count, the m-tile band edges
    assert {1, 16, 17, 32, 33, 64, 65} <= rows


def test_committed_cases_are_what_the_pool_derives(lib):
    assert wc.CASES == wc.derive_cases(lib), "the routes moved: run `python tests/wo8_cases.py` and commit its list"


def test_cases_are_valid_and_small(lib):
    assert len(set(wc.CASES)) == len(wc.CASES)
    for fmt, M, N, K in wc.CASES:
        assert fmt in wc.FMT and 1 <= M <= 257 and 1 <= N <= 1040 and 16 <= K <= 4096 and K % 16 == 0
        assert wc.signature(lib, (fmt, M, N, K))[1] != "invalid"


def test_the_seam_is_where_the_kernel_constants_put_it(lib):
    """The stream form's last row count and the tiled form's first (wo8_kernels.hip: kStreamMaxRows*), on every grid shape."""
    import route_cases

    for fmt in wc.FMT:
        for N, K in route_cases.NK_GRID + wc.EXTRA_NK:
            assert wc.route(lib, fmt, 64, N, K)["kernel"] == "stream"
            assert wc.route(lib, fmt, 65, N, K)["kernel"] == "tile"
