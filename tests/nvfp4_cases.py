"""The routes the NVFP4 linears (weight-only, kind "wo"; codes x codes, kind "dyn") can take, and the case list that runs each of them
(test_nvfp4_host.py checks the list on the CPU, test_nvfp4_gpu.py runs it).  The method of wo8_cases.py for this family alone.

A route's *signature* is what selects a template instantiation of nvfp4_kernels.hip: the kind, nvfp4_route's kernel, the waves of a
workgroup and its m-tiles.  The reachable signatures are discovered over route_cases.M_GRID x NK_GRID plus N in {1, 17} and K in
{16, 48}; the cases come from a pool of small shapes (nothing above 257 x 1040 x 4096: the exact-sum inputs of the GPU test need
K <= 4096): for every signature and every requirement it can meet, the cheapest shape of the pool.  CASES is committed;
`python tests/nvfp4_cases.py` prints it, and test_nvfp4_host.py fails when the committed list is not what the derivation picks, so a route
change shows as a diff here.
"""
import ctypes
import itertools

import route_cases

KIND = {"wo": 0, "dyn": 1}  # AO_NVFP4_KIND_*
KERNELS = ("invalid", "stream", "tile")
EXTRA_NK = tuple(itertools.product((1, 17), (16, 48)))

# the pool the cases are picked from
POOL_M = (1, 5, 16, 17, 32, 33, 64, 65, 100, 128, 129, 257)
POOL_N = (1, 17, 48, 1000, 1040)
POOL_K = (16, 48, 128, 144, 256, 384, 512, 528, 640, 1024, 1040, 1152, 2048, 2064, 4096)

# edge: the first / last row count of the signature's band (M = 1, the stream form's last and the tiled form's first row count, every
# m-tile band edge); ragged_m: M % 16 != 0; ragged_n: N % 16 != 0 above one tile; small_n: N below one tile; k16: K = 16;
# partial_k: the last 128-k step (64-k step of the tiled form) is partial; odd_blocks: K is no multiple of 32, so a row's last block stands
# alone (the 8-byte loads of the stream form); uneven_waves: the k steps do not divide over the waves; wide_n: many column tiles
# (N >= 1000: 16 tiles of the tiled form, both wave columns of the last one in range, a ragged last tile)
REQUIREMENTS = ("edge_lo", "edge_hi", "ragged_m", "ragged_n", "small_n", "k16", "partial_k", "odd_blocks", "uneven_waves", "wide_n")


def route(lib, kind, M, N, K):
    out = (ctypes.c_int32 * 7)()
    rc = lib.ao_nvfp4_linear_route(KIND[kind], M, N, K, out, 7)
    assert rc == 0, rc
    kernel, waves, mt, tile_m, tile_n, gx, gy = list(out)
    return {"kernel": KERNELS[kernel], "waves": waves, "m_tiles": mt, "rows": tile_m, "cols": tile_n, "grid": (gx, gy),
            "parts": waves if KERNELS[kernel] == "stream" else 1}


def signature(lib, case):
    fmt, M, N, K = case
    r = route(lib, fmt, M, N, K)
    return (fmt, r["kernel"], r["waves"], r["m_tiles"])


def reachable(lib):
    """signature -> number of grid cells that reach it"""
    reach = {}
    for fmt in KIND:
        for M in route_cases.M_GRID:
            for N, K in route_cases.NK_GRID + EXTRA_NK:
                sig = signature(lib, (fmt, M, N, K))
                if sig[1] != "invalid":
                    reach[sig] = reach.get(sig, 0) + 1
    return reach


def band(lib, sig, N, K):
    """The row counts of the pool's range (1 .. 257) that reach `sig` at this N, K."""
    return [m for m in range(1, max(POOL_M) + 1) if signature(lib, (sig[0], m, N, K)) == sig]


def properties(lib, case):
    fmt, M, N, K = case
    sig = signature(lib, case)
    r = route(lib, fmt, M, N, K)
    rows = band(lib, sig, N, K)
    step = 128 if r["kernel"] == "stream" else 64
    ksteps = (K + step - 1) // step
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
    if K == 16:
        props.add("k16")
    if K % step and K > step:
        props.add("partial_k")
    if K % 32 and K > 16:
        props.add("odd_blocks")
    if r["kernel"] == "stream" and r["waves"] > 1 and ksteps % r["waves"]:
        props.add("uneven_waves")
    return props


def cost(case):
    fmt, M, N, K = case
    return (M * N * K, M, N, K)


def pool():
    return [(fmt, M, N, K) for fmt in KIND for M in POOL_M for N in POOL_N for K in POOL_K]


def derive_cases(lib):
    by_sig = {}
    for case in pool():
        sig = signature(lib, case)
        if sig[1] != "invalid":
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
    return sorted(picked, key=lambda c: (c[0],) + cost(c))


# ---- committed (python tests/nvfp4_cases.py) ----
CASES = [
    ('dyn', 1, 1, 16),
    ('dyn', 1, 1, 48),
    ('dyn', 1, 1, 144),
    ('dyn', 16, 1, 16),
    ('dyn', 1, 17, 16),
    ('dyn', 17, 1, 16),
    ('dyn', 1, 1, 384),
    ('dyn', 1, 1, 512),
    ('dyn', 32, 1, 16),
    ('dyn', 1, 1, 528),
    ('dyn', 33, 1, 16),
    ('dyn', 17, 1, 48),
    ('dyn', 1, 1, 1024),
    ('dyn', 64, 1, 16),
    ('dyn', 1, 1, 1040),
    ('dyn', 65, 1, 16),
    ('dyn', 33, 1, 48),
    ('dyn', 1, 1, 2048),
    ('dyn', 1, 1, 2064),
    ('dyn', 16, 1, 144),
    ('dyn', 1, 17, 144),
    ('dyn', 17, 1, 144),
    ('dyn', 65, 1, 48),
    ('dyn', 257, 1, 16),
    ('dyn', 32, 1, 144),
    ('dyn', 17, 17, 16),
    ('dyn', 33, 1, 144),
    ('dyn', 17, 1, 384),
    ('dyn', 16, 1, 512),
    ('dyn', 1, 17, 512),
    ('dyn', 17, 1, 512),
    ('dyn', 17, 1, 528),
    ('dyn', 33, 17, 16),
    ('dyn', 64, 1, 144),
    ('dyn', 65, 1, 144),
    ('dyn', 33, 1, 384),
    ('dyn', 1, 1000, 16),
    ('dyn', 16, 1, 1024),
    ('dyn', 32, 1, 512),
    ('dyn', 33, 1, 512),
    ('dyn', 1, 17, 1024),
    ('dyn', 17, 1, 1024),
    ('dyn', 33, 1, 528),
    ('dyn', 17, 1, 1040),
    ('dyn', 65, 17, 16),
    ('dyn', 16, 1, 2048),
    ('dyn', 32, 1, 1024),
    ('dyn', 64, 1, 512),
    ('dyn', 33, 1, 1024),
    ('dyn', 33, 1, 1040),
    ('dyn', 1, 17, 2048),
    ('dyn', 17, 1, 2048),
    ('dyn', 17, 1, 2064),
    ('dyn', 17, 17, 144),
    ('dyn', 32, 1, 2048),
    ('dyn', 64, 1, 1024),
    ('dyn', 33, 17, 144),
    ('dyn', 1, 1000, 144),
    ('dyn', 17, 17, 512),
    ('dyn', 17, 1000, 16),
    ('dyn', 33, 17, 512),
    ('dyn', 17, 17, 1024),
    ('dyn', 1, 1000, 512),
    ('dyn', 33, 1000, 16),
    ('dyn', 33, 17, 1024),
    ('dyn', 17, 17, 2048),
    ('dyn', 1, 1000, 1024),
    ('dyn', 65, 1000, 16),
    ('dyn', 1, 1000, 2048),
    ('dyn', 17, 1000, 144),
    ('dyn', 33, 1000, 144),
    ('dyn', 17, 1000, 512),
    ('dyn', 33, 1000, 512),
    ('dyn', 17, 1000, 1024),
    ('dyn', 33, 1000, 1024),
    ('dyn', 17, 1000, 2048),
    ('wo', 1, 1, 16),
    ('wo', 1, 1, 48),
    ('wo', 1, 1, 144),
    ('wo', 16, 1, 16),
    ('wo', 1, 17, 16),
    ('wo', 17, 1, 16),
    ('wo', 1, 1, 384),
    ('wo', 1, 1, 512),
    ('wo', 32, 1, 16),
    ('wo', 1, 1, 528),
    ('wo', 33, 1, 16),
    ('wo', 17, 1, 48),
    ('wo', 1, 1, 1024),
    ('wo', 64, 1, 16),
    ('wo', 1, 1, 1040),
    ('wo', 65, 1, 16),
    ('wo', 33, 1, 48),
    ('wo', 1, 1, 2048),
    ('wo', 1, 1, 2064),
    ('wo', 16, 1, 144),
    ('wo', 1, 17, 144),
    ('wo', 17, 1, 144),
    ('wo', 65, 1, 48),
    ('wo', 257, 1, 16),
    ('wo', 32, 1, 144),
    ('wo', 17, 17, 16),
    ('wo', 33, 1, 144),
    ('wo', 17, 1, 384),
    ('wo', 16, 1, 512),
    ('wo', 1, 17, 512),
    ('wo', 17, 1, 512),
    ('wo', 17, 1, 528),
    ('wo', 33, 17, 16),
    ('wo', 64, 1, 144),
    ('wo', 65, 1, 144),
    ('wo', 33, 1, 384),
    ('wo', 1, 1000, 16),
    ('wo', 16, 1, 1024),
    ('wo', 32, 1, 512),
    ('wo', 33, 1, 512),
    ('wo', 1, 17, 1024),
    ('wo', 17, 1, 1024),
    ('wo', 33, 1, 528),
    ('wo', 17, 1, 1040),
    ('wo', 65, 17, 16),
    ('wo', 16, 1, 2048),
    ('wo', 32, 1, 1024),
    ('wo', 64, 1, 512),
    ('wo', 33, 1, 1024),
    ('wo', 33, 1, 1040),
    ('wo', 1, 17, 2048),
    ('wo', 17, 1, 2048),
    ('wo', 17, 1, 2064),
    ('wo', 17, 17, 144),
    ('wo', 32, 1, 2048),
    ('wo', 64, 1, 1024),
    ('wo', 33, 17, 144),
    ('wo', 1, 1000, 144),
    ('wo', 17, 17, 512),
    ('wo', 17, 1000, 16),
    ('wo', 33, 17, 512),
    ('wo', 17, 17, 1024),
    ('wo', 1, 1000, 512),
    ('wo', 33, 1000, 16),
    ('wo', 33, 17, 1024),
    ('wo', 17, 17, 2048),
    ('wo', 1, 1000, 1024),
    ('wo', 65, 1000, 16),
    ('wo', 1, 1000, 2048),
    ('wo', 17, 1000, 144),
    ('wo', 33, 1000, 144),
    ('wo', 17, 1000, 512),
    ('wo', 33, 1000, 512),
    ('wo', 17, 1000, 1024),
    ('wo', 33, 1000, 1024),
    ('wo', 17, 1000, 2048),
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
