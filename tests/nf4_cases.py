"""The routes the fused NF4 linear (nf4_stream_kernel) can take, and the case list that runs each of them (test_nf4_host.py checks the
list on the CPU, test_nf4_gpu.py runs it).  The method of nvfp4_cases.py for this family.

A route's *signature* is what selects a template instantiation of nf4_kernels.hip: the waves of a workgroup and its m-tiles.  The family
has one fused form and a seam above which the route says "not fused"; the signatures are discovered, and the cases run, with the stream
form FORCED (ao_nf4_linear_set_form(1)), so the list does not move with the seam.  Discovery runs over route_cases.M_GRID x NK_GRID plus
N in {1, 17} and K in {32, 96}; the cases come from a pool of small shapes (K <= 4096: the exact-sum inputs of the GPU test), for every
signature and every requirement it can meet the cheapest shape of the pool.  A case is (M, N, K, block_size, scaler_block_size), the
format picked by `fmt`: the largest block size that divides K and the largest scaler block size up to 8 that divides the block count.
CASES is committed; `python tests/nf4_cases.py` prints it, and test_nf4_host.py fails when the committed list is not what the derivation
picks, so a route change shows as a diff here.
"""
import ctypes
import itertools

import route_cases

EXTRA_NK = tuple(itertools.product((1, 17), (32, 96)))

# the pool the cases are picked from (every K a multiple of 32, the smallest block)
POOL_M = (1, 5, 16, 17, 32, 33, 64, 65, 100, 128, 129, 257)
POOL_N = (1, 17, 48, 1000, 1040)
POOL_K = (32, 64, 96, 128, 160, 256, 384, 512, 544, 640, 1024, 1056, 1152, 2048, 2080, 4096)

# edge: the first / last row count of the signature's band; ragged_m: M % 16 != 0; ragged_n: N % 16 != 0 above one tile; small_n: N
# below one tile; one_block_k: K is one block; partial_k: the last 128-k step is partial; uneven_waves: the k steps do not divide over the
# waves; wide_n: many column tiles (N >= 1000)
REQUIREMENTS = ("edge_lo", "edge_hi", "ragged_m", "ragged_n", "small_n", "one_block_k", "partial_k", "uneven_waves", "wide_n")


def fmt(N, K):
    B = next(b for b in (128, 64, 32) if K % b == 0)
    blocks = N * K // B
    SB = next(s for s in (8, 4, 2, 1) if blocks % s == 0)
    return B, SB


class forced_stream:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.ao_nf4_linear_set_form(1) == 0

    def __exit__(self, *exc):
        assert self.lib.ao_nf4_linear_set_form(0) == 0
        return False


def route(lib, M, N, K, B, SB):
    """the route as the library reports it NOW (under the caller's form)"""
    out = (ctypes.c_int32 * 7)()
    rc = lib.ao_nf4_linear_route(M, N, K, B, SB, out, 7)
    assert rc == 0, rc
    kernel, waves, mt, tile_m, tile_n, gx, gy = list(out)
    return {"kernel": ("not fused", "stream")[kernel], "waves": waves, "m_tiles": mt, "rows": tile_m, "cols": tile_n, "grid": (gx, gy),
            "parts": waves}


def signature(lib, case):
    r = route(lib, *case)
    return (r["kernel"], r["waves"], r["m_tiles"])


def reachable(lib):
    """signature -> number of grid cells that reach it (stream form forced)"""
    reach = {}
    with forced_stream(lib):
        for M in route_cases.M_GRID:
            for N, K in route_cases.NK_GRID + EXTRA_NK:
                if K % 32:
                    continue
                sig = signature(lib, (M, N, K) + fmt(N, K))
                if sig[0] == "stream":
                    reach[sig] = reach.get(sig, 0) + 1
    return reach


def band(lib, sig, N, K):
    """The row counts of the pool's range (1 .. 257) that reach `sig` at this N, K."""
    return [m for m in range(1, max(POOL_M) + 1) if signature(lib, (m, N, K) + fmt(N, K)) == sig]


def properties(lib, case):
    M, N, K, B, SB = case
    sig = signature(lib, case)
    r = route(lib, *case)
    rows = band(lib, sig, N, K)
    ksteps = (K + 127) // 128
    props = set()
    if M == rows[0]:
        props.add("edge_lo")
    if M == rows[-1]:
        props.add("edge_hi")
    if M % 16:
        props.add("ragged_m")
    if N % 16 and N > 16:
        props.add("ragged_n")
    if N < 16:
        props.add("small_n")
    if N >= 1000:
        props.add("wide_n")
    if K == B:
        props.add("one_block_k")
    if K % 128 and K > 128:
        props.add("partial_k")
    if r["waves"] > 1 and ksteps % r["waves"]:
        props.add("uneven_waves")
    return props


def cost(case):
    M, N, K = case[:3]
    return (M * N * K, M, N, K)


def pool():
    return [(M, N, K) + fmt(N, K) for M in POOL_M for N in POOL_N for K in POOL_K]


def derive_cases(lib):
    with forced_stream(lib):
        by_sig = {}
        for case in pool():
            sig = signature(lib, case)
            if sig[0] == "stream":
                by_sig.setdefault(sig, []).append(case)
        picked = set()
        for sig, items in by_sig.items():
            items.sort(key=cost)
            props = {case: properties(lib, case) for case in items}
            for req in REQUIREMENTS:
                for case in items:
                    if req in props[case]:
                        picked.add(case)
                        break
    return sorted(picked, key=cost)


# ---- committed (python tests/nf4_cases.py) ----
CASES = [
    (1, 1, 32, 32, 1),
    (1, 1, 160, 32, 1),
    (1, 1, 384, 128, 1),
    (1, 1, 512, 128, 4),
    (16, 1, 32, 32, 1),
    (1, 1, 544, 32, 1),
    (1, 17, 32, 32, 1),
    (17, 1, 32, 32, 1),
    (1, 1, 1024, 128, 8),
    (32, 1, 32, 32, 1),
    (1, 1, 1056, 32, 1),
    (33, 1, 32, 32, 1),
    (1, 1, 2048, 128, 8),
    (1, 1, 2080, 32, 1),
    (16, 1, 160, 32, 1),
    (1, 17, 160, 32, 1),
    (17, 1, 160, 32, 1),
    (32, 1, 160, 32, 1),
    (33, 1, 160, 32, 1),
    (17, 1, 384, 128, 1),
    (16, 1, 512, 128, 4),
    (257, 1, 32, 32, 1),
    (1, 17, 512, 128, 4),
    (17, 1, 512, 128, 4),
    (17, 1, 544, 32, 1),
    (17, 17, 32, 32, 1),
    (33, 1, 384, 128, 1),
    (16, 1, 1024, 128, 8),
    (32, 1, 512, 128, 4),
    (33, 1, 512, 128, 4),
    (1, 17, 1024, 128, 8),
    (17, 1, 1024, 128, 8),
    (17, 1, 1056, 32, 1),
    (33, 1, 544, 32, 1),
    (33, 17, 32, 32, 1),
    (1, 1000, 32, 32, 8),
    (16, 1, 2048, 128, 8),
    (32, 1, 1024, 128, 8),
    (33, 1, 1024, 128, 8),
    (1, 17, 2048, 128, 8),
    (17, 1, 2048, 128, 8),
    (33, 1, 1056, 32, 1),
    (17, 1, 2080, 32, 1),
    (257, 1, 160, 32, 1),
    (17, 17, 160, 32, 1),
    (32, 1, 2048, 128, 8),
    (33, 17, 160, 32, 1),
    (257, 1, 512, 128, 4),
    (17, 17, 512, 128, 4),
    (1, 1000, 160, 32, 8),
    (257, 1, 1024, 128, 8),
    (33, 17, 512, 128, 4),
    (17, 17, 1024, 128, 8),
    (1, 1000, 512, 128, 8),
    (17, 1000, 32, 32, 8),
    (33, 17, 1024, 128, 8),
    (17, 17, 2048, 128, 8),
    (1, 1000, 1024, 128, 8),
    (33, 1000, 32, 32, 8),
    (1, 1000, 2048, 128, 8),
    (17, 1000, 160, 32, 8),
    (33, 1000, 160, 32, 8),
    (17, 1000, 512, 128, 8),
    (33, 1000, 512, 128, 8),
    (17, 1000, 1024, 128, 8),
    (33, 1000, 1024, 128, 8),
    (17, 1000, 2048, 128, 8),
]

if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from ao_amd import _lib

    print("CASES = [")
    for c in derive_cases(_lib.lib()):
        print("    %r," % (c,))
    print("]")
