"""The GEMM routes the product can take, and the case list that runs each of them (test_route_coverage.py checks the list on the CPU,
test_route_parity_gpu.py runs it).

A route's *signature* is what selects a different template instantiation or code path: for the 8-bit entry points the kernel of
gemm8_route, its tile, whether K is cut into parts, the dec8 shape and the mid8 m-tiles (launch_gemm8, gemm8_scaled, dyn_linear); for
the int4 matmul every field of int4_route that launch_route switches on, plus the group size; for fp8 x int4 the form
ao_fp8_int4_kernel_name names (or the fused cast's form), the group size and whether the weight has zeros; for the MX dense linears
(family "mx") the format, codes or fused cast, and mx_route's kernel, waves and m-tiles; for the grouped GEMMs (GCase, family "grouped")
the entry and every field of grouped8_route that picks an instantiation (kernel, waves, m-tiles, slim, scale fetches, weight stages,
cast).

CASES / GROUPED_CASES are committed, with REACH / GROUPED_REACH: how many cells of the grid reach each signature.
`python tests/route_cases.py` prints them (the smallest shape per requirement of each signature); test_route_coverage.py fails, naming
the signature, when the committed lists no longer cover the routes or a band moved.
"""
import ctypes
import itertools

# ---- the discovery grid ----
M_GRID = tuple(range(1, 18)) + (24, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 192, 255, 256, 257, 320, 384, 448, 511, 512, 513,
                                576, 640, 768, 1024, 1280, 1536, 2048, 4096)
NK_GRID = (
    # Llama-3-8B: qkv, o, gate, gate_up, down
    (6144, 4096), (4096, 4096), (14336, 4096), (28672, 4096), (4096, 14336),
    # Llama-3-70B at TP8: qkv, o, gate_up, down
    (1280, 8192), (8192, 1024), (7168, 8192), (8192, 3584),
    # Llama-2-13B
    (15360, 5120), (5120, 5120), (13824, 5120), (5120, 13824),
    # Qwen2-7B
    (4608, 3584), (3584, 3584), (37888, 3584), (3584, 18944),
    # Mixtral / wide weights of the int4 sweeps
    (10240, 8192), (28672, 8192), (12288, 4096), (4096, 12288),
    # ragged N and K
    (48, 4096), (208, 1152), (1040, 2560), (4112, 1040), (16400, 4096), (4096, 10240), (4096, 16384), (1000, 4096), (4100, 1152),
    (48, 16384), (208, 13824),
)
GROUPS = (32, 64, 128, 256)

# Gemm8Entry order (gemm8_route.h)
ENTRIES8 = ("int8_scaled", "fp8_scaled", "int_mm", "fp8_mm_f32", "int8_dyn", "fp8_dyn")
# Gemm8Kernel order
KERNELS8 = ("invalid", "dec8", "mid8", "stream8", "rb8", "p8h", "p8", "p8p", "dma128", "dma256", "dma256x128", "dma256x256w4", "regstage",
            "dyn8")
FORMS4 = ("tile", "rb", "w32")
FP8_INT4_ENTRIES = ("linear_sym", "linear_asym", "dyn_sym", "dyn_asym")
SCALED = ("int8_scaled", "fp8_scaled")
# the MX dense linears: <format>_codes (ao_mx_linear) and <format>_fused (ao_mx_dynamic_linear, the stream form only)
MX_ENTRIES = ("e4m3_codes", "e4m3_fused", "e2m1_codes", "e2m1_fused")
MX_FMT = {"e4m3": 0, "e2m1": 4}  # AO_MX_FMT_*
MX_KERNELS = ("invalid", "stream", "tile")
MX_N = (16, 17, 257, 1000, 4096, 4100, 14336, 16384, 28672)
MX_K = (32, 96, 128, 160, 384, 1024, 4096, 4160, 14336)  # 4160: 33 k steps, the last one half masked
WITH_BIAS = SCALED + ("int8_dyn", "fp8_dyn") + FP8_INT4_ENTRIES + MX_ENTRIES


class Case(tuple):
    """(family, entry, M, N, K, G, bias, aligned): family "gemm8" / "int4" / "fp8_int4" / "mx"; G the int4 group size (0 otherwise);
    aligned False: scales and bias passed at a 4- / 2-byte offset (MX: the E8M0 scale bytes at a 1-byte offset)."""

    __slots__ = ()

    def __new__(cls, family, entry, M, N, K, G, bias, aligned):
        return tuple.__new__(cls, (family, entry, M, N, K, G, bias, aligned))

    family = property(lambda s: s[0])
    entry = property(lambda s: s[1])
    M = property(lambda s: s[2])
    N = property(lambda s: s[3])
    K = property(lambda s: s[4])
    G = property(lambda s: s[5])
    bias = property(lambda s: s[6])
    aligned = property(lambda s: s[7])


# ---- the route queries ----
def route8(lib, entry, M, N, K, aligned=True):
    out = (ctypes.c_int32 * 11)()
    rc = lib.ao_gemm8_route(ENTRIES8.index(entry), M, N, K, int(aligned), out, 11)
    assert rc == 0, rc
    keys = ("kernel", "tile_rows", "tile_cols", "k_parts", "dec_waves", "dec_depth", "dec_loop", "dec_half", "dec_rows8", "mid_mt", "mid_split")
    r = dict(zip(keys, list(out)))
    r["kernel"] = KERNELS8[r["kernel"]]
    return r


def route4(lib, M, N, K, G):
    out = (ctypes.c_int32 * 10)()
    rc = lib.ao_int4_mm_route(M, N, K, G, out, 10)
    assert rc == 0, rc
    r = dict(zip(("form", "rows", "depth", "straight", "waves", "nt", "mt", "cg", "split", "prod"), list(out)))
    r["form"] = FORMS4[r["form"]]
    return r


def fp8_int4_form(lib, entry, M, N, K, G):
    """ao_fp8_int4_kernel_name's form, or the fused cast's: the wave-private cast at M = 1 with <= 16 k-blocks per wave
    (launch_fp8_int4), else the workgroup-wide one.  None where the entry does not take the shape."""
    if entry.startswith("dyn"):
        if not lib.ao_fp8_int4_dynamic_fits(M, N, K) or K % G:
            return None
        kbl = K // 128
        wpb = 8 if kbl >= 16 else 4
        if wpb > kbl:
            wpb = 4 if kbl < 4 else kbl
        return "fused_priv" if M == 1 and (kbl + wpb - 1) // wpb <= 16 else "fused_wg"
    name = lib.ao_fp8_int4_kernel_name(M, N, K, G).decode()
    return None if name == "invalid" else name[len("fp8_int4_mm_kernel"):]


def mx_route(lib, fmt, M, N, K):
    out = (ctypes.c_int32 * 7)()
    rc = lib.ao_mx_linear_route(fmt, M, N, K, out, 7)
    assert rc == 0, rc
    r = dict(zip(("kernel", "waves", "mt", "tile_m", "tile_n", "grid_x", "grid_y"), list(out)))
    r["kernel"] = MX_KERNELS[r["kernel"]]
    return r


def mx_wave_cap(r, N):
    """The stream form's waves before K cuts them down (mx_route): 16, 8 from 256 column tiles, 4 from 1024; 8 at 4 m-tiles."""
    ntiles = (N + 15) // 16
    w = 4 if ntiles >= 1024 else 8 if ntiles >= 256 else 16
    return min(w, 8) if r["mt"] == 4 else w


def route_of(lib, case):
    """The product route of a case, with the launch geometry the edge requirements read: rows / cols of one tile (or slab) and the
    K parts.  None where no kernel takes the shape."""
    fam, entry, M, N, K, G = case[:6]
    if fam == "mx":
        fmt, form = entry.split("_")
        r = mx_route(lib, MX_FMT[fmt], M, N, K)
        if r["kernel"] == "invalid" or (form == "fused" and r["kernel"] != "stream"):
            return None
        sig = [fam, entry, r["kernel"], "w%d" % r["waves"], "mt%d" % r["mt"]]
        return {"sig": "/".join(sig), "rows": r["tile_m"], "cols": r["tile_n"], "parts": 1, "raw": r}
    if fam == "gemm8":
        r = route8(lib, entry, M, N, K, case.aligned)
        if r["kernel"] == "invalid":
            return None
        k = r["kernel"]
        sig = [fam, entry, k]
        if k == "dec8":
            rows, cols, parts = (8 if r["dec_rows8"] else 16), 16, 1
            sig += ["w%d" % r["dec_waves"], "d%d" % r["dec_depth"]] + [f for f in ("loop", "half", "rows8") if r["dec_" + f]]
        elif k == "mid8":
            rows, cols, parts = 16 * r["mid_mt"], 128, r["mid_split"]
            sig += ["mt%d" % r["mid_mt"]]
        elif k in ("stream8", "dyn8"):
            rows, cols, parts = 16, 16, 1
        else:
            rows, cols, parts = r["tile_rows"], r["tile_cols"], r["k_parts"]
            sig += ["%dx%d" % (rows, cols)]
        if parts > 1:
            sig += ["kparts"]
        return {"sig": "/".join(sig), "rows": rows, "cols": cols, "parts": parts, "raw": r}
    if fam == "int4":
        if N % 16 or K % 128 or K % G:
            return None
        r = route4(lib, M, N, K, G)
        sig = [fam, "g%d" % G, r["form"]]
        if r["form"] == "tile":
            rows, cols = r["rows"], 16
            sig += ["r%d" % r["rows"], "d%d" % r["depth"]] + (["straight"] if r["straight"] else [])
        elif r["form"] == "rb":
            rows, cols = 16 * r["mt"], 16 * r["waves"] * r["nt"]
            sig += ["w%d" % r["waves"], "nt%d" % r["nt"], "mt%d" % r["mt"]] + (["prod"] if r["prod"] else [])
        else:
            rows, cols = 128, 128 * r["cg"]
            sig += ["cg%d" % r["cg"]] + (["prod"] if r["prod"] else [])
        if r["split"] > 1:
            sig += ["kparts"]
        return {"sig": "/".join(sig), "rows": rows, "cols": cols, "parts": r["split"], "raw": r}
    if fam == "fp8_int4":
        if N % 16 or K % 128 or K % G:
            return None
        form = fp8_int4_form(lib, entry, M, N, K, G)
        if form is None:
            return None
        mt, nt = (int(form[1]), int(form[3])) if form.startswith("<") else (1, 1)
        return {"sig": "/".join([fam, entry, "g%d" % G, form]), "rows": 16 * mt, "cols": 16 * nt, "parts": 1, "raw": form}
    raise ValueError(fam)


def signature(lib, case):
    r = route_of(lib, case)
    return None if r is None else r["sig"]


# ---- the edge requirements ----
def _same_sig_at(lib, case, m):
    if m < 1:
        return False
    return signature(lib, Case(*((case[0], case[1], m) + tuple(case[3:])))) == signature(lib, case)


def properties(lib, case, route=None):
    """The edge requirements a case meets: 'edge' (M - 1 or M + 1 takes another route), 'ragged_m' (M not a multiple of the tile or
    slab rows), 'ragged_n' (N not a multiple of the tile columns), 'uneven_k' (K parts that do not divide the 128-wide k-blocks),
    'unaligned' (scales and bias off their 16-byte alignment), 'realigned' (unaligned, and aligned operands take another route); MX:
    'n_tiles' (more than one column tile), 'masked_k' (K % 128 != 0), 'uneven_waves' (k steps not a multiple of the stream form's
    waves), 'fewer_waves' (fewer k steps than the waves the column tiles ask for)."""
    r = route or route_of(lib, case)
    props = set()
    if not _same_sig_at(lib, case, case.M - 1) or not _same_sig_at(lib, case, case.M + 1):
        props.add("edge")
    if case.M % r["rows"]:
        props.add("ragged_m")
    if case.N % r["cols"]:
        props.add("ragged_n")
    if r["parts"] > 1 and (case.K // 128) % r["parts"]:
        props.add("uneven_k")
    if case.family == "mx":
        if case.N > r["cols"]:
            props.add("n_tiles")  # more than one column tile
        if case.K % 128:
            props.add("masked_k")  # the last k step masked: the e4m3 upper half, the e2m1 blocks >= K / 32
        ksteps = (case.K + 127) // 128
        if r["raw"]["kernel"] == "stream" and ksteps % r["raw"]["waves"]:
            props.add("uneven_waves")
        if r["raw"]["kernel"] == "stream" and r["raw"]["waves"] < mx_wave_cap(r["raw"], case.N):
            props.add("fewer_waves")
    if not case.aligned:
        props.add("unaligned")
        if signature(lib, Case(*(tuple(case[:7]) + (True,)))) != r["sig"]:
            props.add("realigned")
    return props


REQUIREMENTS = ("edge", "ragged_m", "ragged_n", "uneven_k", "realigned", "n_tiles", "masked_k", "uneven_waves", "fewer_waves")


def grid_cases():
    """Every case of the discovery grid (bias off: the signature does not depend on it)."""
    for M, (N, K) in itertools.product(M_GRID, NK_GRID):
        for entry in ENTRIES8:
            for aligned in ((True, False) if entry in SCALED else (True,)):
                yield Case("gemm8", entry, M, N, K, 0, False, aligned)
        for G in GROUPS:
            yield Case("int4", "mm", M, N, K, G, False, True)
            for entry in FP8_INT4_ENTRIES:
                yield Case("fp8_int4", entry, M, N, K, G, False, True)
    for M, N, K in itertools.product(M_GRID, MX_N, MX_K):
        for entry in MX_ENTRIES:
            for aligned in (True, False):
                yield Case("mx", entry, M, N, K, 0, False, aligned)


def reachable(lib):
    """signature -> [(case, properties)] over the grid."""
    out = {}
    for c in grid_cases():
        r = route_of(lib, c)
        if r is None:
            continue
        out.setdefault(r["sig"], []).append((c, None, r))
    return out


def cost(case):
    return (case.M * case.N * case.K, case.M, case.N, case.K)


def needed(lib, sig, items):
    """The requirements a signature admits on the grid (a signature reached only at M = 1 admits no ragged M ...), with the grid's
    cases in order of cost.  A requirement is met by its cheapest case; 'unaligned' is asked once per (entry, kernel) below, and
    'realigned' of every signature that unaligned scales reach from another route."""
    props = []
    for c, _, r in sorted(items, key=lambda t: cost(t[0])):
        props.append((c, properties(lib, c, r)))
    admitted = set()
    for _, p in props:
        admitted |= p
    return [q for q in REQUIREMENTS if q in admitted] + (["unaligned"] if "unaligned" in admitted else []), props


def derive_cases(lib):
    """The cheapest case per (signature, requirement), in the order of REQUIREMENTS; a case also meets the later requirements it happens
    to meet.  An entry that takes a bias runs each case twice, without and with one: the two epilogue paths of every route."""
    cases = []
    unaligned_kernels = set()
    for sig, items in sorted(reachable(lib).items()):
        reqs, props = needed(lib, sig, items)
        if sig.split("/")[0] in ("gemm8", "mx"):
            key = tuple(sig.split("/")[:3])
            if "unaligned" in reqs and key in unaligned_kernels:
                reqs.remove("unaligned")
            elif "unaligned" in reqs:
                unaligned_kernels.add(key)
        elif "unaligned" in reqs:
            reqs.remove("unaligned")
        if not reqs:
            reqs = ["any"]
        missing = list(reqs)
        while missing:
            c, p = next((c, p) for c, p in props if missing[0] in p or missing[0] == "any")
            for bias in ((False, True) if c.entry in WITH_BIAS else (False,)):
                cases.append((Case(c.family, c.entry, c.M, c.N, c.K, c.G, bias, c.aligned), sig))
            missing = [q for q in missing[1:] if q not in p]
    return cases


# ---- the grouped GEMMs (grouped8_route) ----
# Grouped8Entry order: ao_fp8_grouped_mm, ao_mxfp8_grouped_mm, _dyn, _dyn_pair, _pair
GROUPED_ENTRIES = ("fp8", "mx", "mx_dyn", "mx_dyn_pair", "mx_pair")
GROUPED_KERNELS = ("invalid", "rb8", "mx_stream", "mx_grouped", "stream8")
FUSED = ("mx_dyn", "mx_dyn_pair")  # the fused cast: every case runs under both scaling modes
PAIRS = ("mx_dyn_pair", "mx_pair")
E_GRID = (1, 2, 8, 16, 64, 65, 128)
GN_GRID = (16, 48, 208, 1024, 1040, 4096, 14336)
GK_GRID = (128, 384, 512, 2048, 4096, 14336)
OFFS = ("spread", "one")  # group-size patterns (group_sizes)
STREAM_GRID = {8: 512, 16: 256}  # mx_stream_kernel's workgroups (launch_mx_stream: two per CU at 8 waves, one at 16)


def gm_grid(E):
    """M_total on both sides of the slab heights and of 48 E (the decode-size bound)."""
    return tuple(sorted({1, 17, 63, 64, 65, 127, 128, 129, 48 * E, 48 * E + 1}))


class GCase(tuple):
    """(family, entry, M, N, K, E, aligned, offs, mode): family "grouped"; M the total rows; offs the group_sizes pattern; mode the
    fused cast's scaling ("floor" / "rceil", "" for the other entries); aligned False: the scales passed at a 4-byte offset (what
    ao_mxfp8_grouped_mm's aligned flag covers; the fused-cast and pair forms refuse it, the rowwise form reads it alike)."""

    __slots__ = ()

    def __new__(cls, family, entry, M, N, K, E, aligned, offs, mode):
        return tuple.__new__(cls, (family, entry, M, N, K, E, aligned, offs, mode))

    family = property(lambda s: s[0])
    entry = property(lambda s: s[1])
    M = property(lambda s: s[2])
    N = property(lambda s: s[3])
    K = property(lambda s: s[4])
    E = property(lambda s: s[5])
    aligned = property(lambda s: s[6])
    offs = property(lambda s: s[7])
    mode = property(lambda s: s[8])


def route_grouped(lib, entry, M, N, K, E, aligned=True):
    out = (ctypes.c_int32 * 10)()
    rc = lib.ao_grouped8_route(GROUPED_ENTRIES.index(entry), M, N, K, E, int(aligned), out, 10)
    assert rc == 0, rc
    r = dict(zip(("kernel", "waves", "mt", "slim", "qs", "sw", "cast", "tn", "slab_rows", "slabs"), list(out)))
    r["kernel"] = GROUPED_KERNELS[r["kernel"]]
    return r


def grouped_route_of(lib, case):
    """The product route of a grouped case: its signature, the rows of one m-tile / slab and the columns of one tile.  None where the
    entry refuses the shape."""
    r = route_grouped(lib, case.entry, case.M, case.N, case.K, case.E, case.aligned)
    k = r["kernel"]
    if k == "invalid":
        return None
    sig = ["grouped", case.entry, k]
    if k in ("rb8", "mx_stream"):
        sig += ["w%d" % r["waves"]]
    if r["mt"]:
        sig += ["mt%d" % r["mt"]]
    if r["slim"]:
        sig += ["slim"]
    if r["qs"]:
        sig += ["qs%d" % r["qs"]]
    if r["sw"]:
        sig += ["sw%d" % r["sw"]]
    if r["cast"]:
        sig += ["cast%d" % r["cast"]]
    rows = {"rb8": r["slab_rows"], "mx_stream": 64}.get(k, 16 * r["mt"])
    cols = {"rb8": 16 * r["waves"], "mx_stream": 16 * r["waves"], "mx_grouped": 16 * r["tn"]}.get(k, 16)
    return {"sig": "/".join(sig), "rows": rows, "cols": cols, "parts": 1, "raw": r}


def group_sizes(E, M, pattern):
    """Rows per expert.  'one': every row on the last expert.  'spread': expert 0, the middle one (E >= 5) and the last (E >= 5) empty,
    then a one-row group, a group of up to 99 rows starting at row 1 (inside an m-tile; larger than a 64-row slab from 100 rows), the
    rest spread over the other experts from the highest down (experts >= 64 get tokens first), and the last row past offs[-1]."""
    sizes = [0] * E
    if pattern == "one":
        sizes[-1] = M
        return sizes
    budget = M - (1 if M >= 2 else 0)
    skip = {0, E // 2, E - 1} if E >= 5 else {0} if E >= 2 else set()
    nonempty = [e for e in range(E) if e not in skip]
    if len(nonempty) >= 2 and budget >= 2:
        sizes[nonempty[0]] = 1
        sizes[nonempty[1]] = min(budget - 1, 99)
        rest, left = nonempty[2:], budget - 1 - sizes[nonempty[1]]
        if not rest:
            sizes[nonempty[1]] += left
        for i, e in enumerate(reversed(rest)):
            sizes[e] = left // len(rest) + (1 if i < left % len(rest) else 0)
    else:
        sizes[nonempty[0]] = budget
    return sizes


def stream_partition(route, N, K, sizes, pair):
    """mx_stream_kernel's shares (tests/test_streamk_partition.py restates the rule): the (slab, column tile, k step) space in W
    contiguous shares of G // W or one more steps.  -> (W >= 2 and a share holds steps of two experts' tiles, the most pieces share
    boundaries cut one tile into)."""
    waves, ksteps = route["waves"], K // 128
    nt = (N + 16 * waves - 1) // (16 * waves) * (2 if pair else 1)
    slab_expert = [e for e, s in enumerate(sizes) for _ in range((s + 63) // 64)]
    G = len(slab_expert) * nt * ksteps
    if G == 0:
        return False, 1
    W = min(STREAM_GRID[waves], max(1, G // 16))
    sq, sr = divmod(G, W)
    bounds = [v * sq + min(v, sr) for v in range(W + 1)]
    expert = lambda g: slab_expert[g // ksteps // nt]  # noqa: E731
    cross = W >= 2 and any(expert(g0) != expert(g1 - 1) for g0, g1 in zip(bounds, bounds[1:]))
    pieces = {}
    for b in bounds[1:-1]:
        if b % ksteps:
            pieces[b // ksteps] = pieces.get(b // ksteps, 1) + 1
    return cross, max(pieces.values(), default=1)


GROUPED_REQUIREMENTS = ("edge", "ragged_m", "ragged_n", "n_tiles", "k_loop", "empty_first", "empty_mid", "empty_last", "one_row",
                        "mid_tile_start", "spans_slab", "one_expert", "tail", "high_expert", "share_cross", "tile_cut", "tile_cut3",
                        "realigned")
KLOOP_STEPS = 6  # the deepest operand ring (rb8_kernel's weight stages): more k steps than this wrap every ring


def grouped_properties(lib, case, route=None):
    """The edge requirements a grouped case meets: 'edge' (M_total - 1 or + 1 takes another route), 'ragged_m' / 'ragged_n' (M_total
    not a multiple of the slab or m-tile rows, N of the tile columns), 'n_tiles' (more than one column tile), 'k_loop' (more k steps
    than the deepest operand ring, and with the scales fetched per 4 steps at least 3 scale blocks), and of its group sizes: an empty
    expert first, in the middle, last; a one-row group; a group starting inside a 16-row m-tile; a group larger
    than one slab; every row on one expert; rows past offs[-1]; tokens on an expert >= 64; on the stream-K form a share over two
    experts' tiles (two or more shares), a tile cut by a share boundary and one cut into three or more pieces; 'unaligned' /
    'realigned' as for the dense families."""
    r = route or grouped_route_of(lib, case)
    props = set()
    for m in (case.M - 1, case.M + 1):
        other = grouped_route_of(lib, GCase(*((case[0], case[1], m) + tuple(case[3:])))) if m >= 1 else r
        if other is None or other["sig"] != r["sig"]:
            props.add("edge")
    if case.M % r["rows"]:
        props.add("ragged_m")
    if case.N % r["cols"]:
        props.add("ragged_n")
    if case.N > r["cols"]:
        props.add("n_tiles")
    ksteps = case.K // 128
    if ksteps > KLOOP_STEPS and (r["raw"]["qs"] != 4 or ksteps >= 12):
        props.add("k_loop")
    sizes = group_sizes(case.E, case.M, case.offs)
    starts = [sum(sizes[:e]) for e in range(case.E)]
    if case.E > 1:
        props |= {q for q, e in (("empty_first", 0), ("empty_last", case.E - 1)) if sizes[e] == 0}
        if any(s == 0 for s in sizes[1:-1]):
            props.add("empty_mid")
    if 1 in sizes:
        props.add("one_row")
    if any(s and st % 16 for s, st in zip(sizes, starts)):
        props.add("mid_tile_start")
    if max(sizes) > r["rows"]:
        props.add("spans_slab")
    if max(sizes) == case.M:
        props.add("one_expert")
    if sum(sizes) < case.M:
        props.add("tail")
    if any(sizes[64:]):
        props.add("high_expert")
    if r["raw"]["kernel"] == "mx_stream":
        cross, pieces = stream_partition(r["raw"], case.N, case.K, sizes, case.entry in PAIRS)
        props |= {q for q, v in (("share_cross", cross), ("tile_cut", pieces >= 2), ("tile_cut3", pieces >= 3)) if v}
    if not case.aligned:
        props.add("unaligned")
        other = grouped_route_of(lib, GCase(*(tuple(case[:6]) + (True,) + tuple(case[7:]))))
        if other is None or other["sig"] != r["sig"]:
            props.add("realigned")
    return props


def grouped_grid_cases():
    """Every shape of the grouped discovery grid (group pattern and scaling mode do not change the signature)."""
    for entry in GROUPED_ENTRIES:
        for E in E_GRID:
            for M, N, K in itertools.product(gm_grid(E), GN_GRID, GK_GRID):
                for aligned in (True, False):
                    yield GCase("grouped", entry, M, N, K, E, aligned, "spread", "rceil" if entry in FUSED else "")


def grouped_reachable(lib):
    out = {}
    for c in grouped_grid_cases():
        r = grouped_route_of(lib, c)
        if r is not None:
            out.setdefault(r["sig"], []).append((c, None, r))
    return out


def grouped_cost(case):
    """Output and weight elements: a case's expert weights are E x N x K (twice for the pair forms)."""
    return (case.M * case.N * case.K + case.E * case.N * case.K, case.M, case.E, case.N, case.K)


def grouped_needed(lib, sig, items):
    """The requirements a grouped signature admits on the grid (every shape under every group pattern), with those cases in order of
    cost; 'unaligned' is asked once per (entry, kernel) below."""
    props = []
    for c, _, r in sorted(items, key=lambda t: grouped_cost(t[0])):
        for pat in OFFS:
            cp = GCase(*(tuple(c[:7]) + (pat, c.mode)))
            props.append((cp, grouped_properties(lib, cp, r)))
    admitted = set()
    for _, p in props:
        admitted |= p
    return [q for q in GROUPED_REQUIREMENTS if q in admitted] + (["unaligned"] if "unaligned" in admitted else []), props


def derive_grouped_cases(lib):
    """The cheapest case per (signature, requirement); the fused-cast entries run each case under both scaling modes."""
    cases = []
    unaligned_kernels = set()
    for sig, items in sorted(grouped_reachable(lib).items()):
        reqs, props = grouped_needed(lib, sig, items)
        key = tuple(sig.split("/")[1:3])
        if "unaligned" in reqs and key in unaligned_kernels:
            reqs.remove("unaligned")
        elif "unaligned" in reqs:
            unaligned_kernels.add(key)
        missing = list(reqs) or ["any"]
        while missing:
            c, p = next((c, p) for c, p in props if missing[0] in p or missing[0] == "any")
            for mode in (("floor", "rceil") if c.entry in FUSED else ("",)):
                cases.append((GCase(*(tuple(c[:8]) + (mode,))), sig))
            missing = [q for q in missing[1:] if q not in p]
    return cases


# (case, signature): what derive_cases(lib) picks on the grid -- regenerate with `python tests/route_cases.py` after a route changes
CASES = [
    (Case('fp8_int4', 'dyn_asym', 1, 48, 4096, 128, False, True), 'fp8_int4/dyn_asym/g128/fused_priv'),
    (Case('fp8_int4', 'dyn_asym', 1, 48, 4096, 128, True, True), 'fp8_int4/dyn_asym/g128/fused_priv'),
    (Case('fp8_int4', 'dyn_asym', 2, 48, 4096, 128, False, True), 'fp8_int4/dyn_asym/g128/fused_wg'),
    (Case('fp8_int4', 'dyn_asym', 2, 48, 4096, 128, True, True), 'fp8_int4/dyn_asym/g128/fused_wg'),
    (Case('fp8_int4', 'dyn_asym', 1, 48, 4096, 256, False, True), 'fp8_int4/dyn_asym/g256/fused_priv'),
    (Case('fp8_int4', 'dyn_asym', 1, 48, 4096, 256, True, True), 'fp8_int4/dyn_asym/g256/fused_priv'),
    (Case('fp8_int4', 'dyn_asym', 2, 48, 4096, 256, False, True), 'fp8_int4/dyn_asym/g256/fused_wg'),
    (Case('fp8_int4', 'dyn_asym', 2, 48, 4096, 256, True, True), 'fp8_int4/dyn_asym/g256/fused_wg'),
    (Case('fp8_int4', 'dyn_asym', 1, 48, 4096, 32, False, True), 'fp8_int4/dyn_asym/g32/fused_priv'),
    (Case('fp8_int4', 'dyn_asym', 1, 48, 4096, 32, True, True), 'fp8_int4/dyn_asym/g32/fused_priv'),
    (Case('fp8_int4', 'dyn_asym', 2, 48, 4096, 32, False, True), 'fp8_int4/dyn_asym/g32/fused_wg'),
    (Case('fp8_int4', 'dyn_asym', 2, 48, 4096, 32, True, True), 'fp8_int4/dyn_asym/g32/fused_wg'),
    (Case('fp8_int4', 'dyn_asym', 1, 48, 4096, 64, False, True), 'fp8_int4/dyn_asym/g64/fused_priv'),
    (Case('fp8_int4', 'dyn_asym', 1, 48, 4096, 64, True, True), 'fp8_int4/dyn_asym/g64/fused_priv'),
    (Case('fp8_int4', 'dyn_asym', 2, 48, 4096, 64, False, True), 'fp8_int4/dyn_asym/g64/fused_wg'),
    (Case('fp8_int4', 'dyn_asym', 2, 48, 4096, 64, True, True), 'fp8_int4/dyn_asym/g64/fused_wg'),
    (Case('fp8_int4', 'dyn_sym', 1, 48, 4096, 128, False, True), 'fp8_int4/dyn_sym/g128/fused_priv'),
    (Case('fp8_int4', 'dyn_sym', 1, 48, 4096, 128, True, True), 'fp8_int4/dyn_sym/g128/fused_priv'),
    (Case('fp8_int4', 'dyn_sym', 2, 48, 4096, 128, False, True), 'fp8_int4/dyn_sym/g128/fused_wg'),
    (Case('fp8_int4', 'dyn_sym', 2, 48, 4096, 128, True, True), 'fp8_int4/dyn_sym/g128/fused_wg'),
    (Case('fp8_int4', 'dyn_sym', 1, 48, 4096, 256, False, True), 'fp8_int4/dyn_sym/g256/fused_priv'),
    (Case('fp8_int4', 'dyn_sym', 1, 48, 4096, 256, True, True), 'fp8_int4/dyn_sym/g256/fused_priv'),
    (Case('fp8_int4', 'dyn_sym', 2, 48, 4096, 256, False, True), 'fp8_int4/dyn_sym/g256/fused_wg'),
    (Case('fp8_int4', 'dyn_sym', 2, 48, 4096, 256, True, True), 'fp8_int4/dyn_sym/g256/fused_wg'),
    (Case('fp8_int4', 'dyn_sym', 1, 48, 4096, 32, False, True), 'fp8_int4/dyn_sym/g32/fused_priv'),
    (Case('fp8_int4', 'dyn_sym', 1, 48, 4096, 32, True, True), 'fp8_int4/dyn_sym/g32/fused_priv'),
    (Case('fp8_int4', 'dyn_sym', 2, 48, 4096, 32, False, True), 'fp8_int4/dyn_sym/g32/fused_wg'),
    (Case('fp8_int4', 'dyn_sym', 2, 48, 4096, 32, True, True), 'fp8_int4/dyn_sym/g32/fused_wg'),
    (Case('fp8_int4', 'dyn_sym', 1, 48, 4096, 64, False, True), 'fp8_int4/dyn_sym/g64/fused_priv'),
    (Case('fp8_int4', 'dyn_sym', 1, 48, 4096, 64, True, True), 'fp8_int4/dyn_sym/g64/fused_priv'),
    (Case('fp8_int4', 'dyn_sym', 2, 48, 4096, 64, False, True), 'fp8_int4/dyn_sym/g64/fused_wg'),
    (Case('fp8_int4', 'dyn_sym', 2, 48, 4096, 64, True, True), 'fp8_int4/dyn_sym/g64/fused_wg'),
    (Case('fp8_int4', 'linear_asym', 1, 48, 4096, 128, False, True), 'fp8_int4/linear_asym/g128/<1x1>'),
    (Case('fp8_int4', 'linear_asym', 1, 48, 4096, 128, True, True), 'fp8_int4/linear_asym/g128/<1x1>'),
    (Case('fp8_int4', 'linear_asym', 17, 48, 4096, 128, False, True), 'fp8_int4/linear_asym/g128/<2x1>'),
    (Case('fp8_int4', 'linear_asym', 17, 48, 4096, 128, True, True), 'fp8_int4/linear_asym/g128/<2x1>'),
    (Case('fp8_int4', 'linear_asym', 33, 1280, 8192, 128, False, True), 'fp8_int4/linear_asym/g128/<2x2>'),
    (Case('fp8_int4', 'linear_asym', 33, 1280, 8192, 128, True, True), 'fp8_int4/linear_asym/g128/<2x2>'),
    (Case('fp8_int4', 'linear_asym', 1, 48, 4096, 256, False, True), 'fp8_int4/linear_asym/g256/<1x1>'),
    (Case('fp8_int4', 'linear_asym', 1, 48, 4096, 256, True, True), 'fp8_int4/linear_asym/g256/<1x1>'),
    (Case('fp8_int4', 'linear_asym', 17, 48, 4096, 256, False, True), 'fp8_int4/linear_asym/g256/<2x1>'),
    (Case('fp8_int4', 'linear_asym', 17, 48, 4096, 256, True, True), 'fp8_int4/linear_asym/g256/<2x1>'),
    (Case('fp8_int4', 'linear_asym', 33, 1280, 8192, 256, False, True), 'fp8_int4/linear_asym/g256/<2x2>'),
    (Case('fp8_int4', 'linear_asym', 33, 1280, 8192, 256, True, True), 'fp8_int4/linear_asym/g256/<2x2>'),
    (Case('fp8_int4', 'linear_asym', 1, 48, 4096, 32, False, True), 'fp8_int4/linear_asym/g32/<1x1>'),
    (Case('fp8_int4', 'linear_asym', 1, 48, 4096, 32, True, True), 'fp8_int4/linear_asym/g32/<1x1>'),
    (Case('fp8_int4', 'linear_asym', 17, 48, 4096, 32, False, True), 'fp8_int4/linear_asym/g32/<2x1>'),
    (Case('fp8_int4', 'linear_asym', 17, 48, 4096, 32, True, True), 'fp8_int4/linear_asym/g32/<2x1>'),
    (Case('fp8_int4', 'linear_asym', 1, 48, 4096, 64, False, True), 'fp8_int4/linear_asym/g64/<1x1>'),
    (Case('fp8_int4', 'linear_asym', 1, 48, 4096, 64, True, True), 'fp8_int4/linear_asym/g64/<1x1>'),
    (Case('fp8_int4', 'linear_asym', 17, 48, 4096, 64, False, True), 'fp8_int4/linear_asym/g64/<2x1>'),
    (Case('fp8_int4', 'linear_asym', 17, 48, 4096, 64, True, True), 'fp8_int4/linear_asym/g64/<2x1>'),
    (Case('fp8_int4', 'linear_sym', 1, 48, 4096, 128, False, True), 'fp8_int4/linear_sym/g128/<1x1>'),
    (Case('fp8_int4', 'linear_sym', 1, 48, 4096, 128, True, True), 'fp8_int4/linear_sym/g128/<1x1>'),
    (Case('fp8_int4', 'linear_sym', 17, 48, 4096, 128, False, True), 'fp8_int4/linear_sym/g128/<2x1>'),
    (Case('fp8_int4', 'linear_sym', 17, 48, 4096, 128, True, True), 'fp8_int4/linear_sym/g128/<2x1>'),
    (Case('fp8_int4', 'linear_sym', 33, 1280, 8192, 128, False, True), 'fp8_int4/linear_sym/g128/<2x2>'),
    (Case('fp8_int4', 'linear_sym', 33, 1280, 8192, 128, True, True), 'fp8_int4/linear_sym/g128/<2x2>'),
    (Case('fp8_int4', 'linear_sym', 1, 48, 4096, 256, False, True), 'fp8_int4/linear_sym/g256/<1x1>'),
    (Case('fp8_int4', 'linear_sym', 1, 48, 4096, 256, True, True), 'fp8_int4/linear_sym/g256/<1x1>'),
    (Case('fp8_int4', 'linear_sym', 17, 48, 4096, 256, False, True), 'fp8_int4/linear_sym/g256/<2x1>'),
    (Case('fp8_int4', 'linear_sym', 17, 48, 4096, 256, True, True), 'fp8_int4/linear_sym/g256/<2x1>'),
    (Case('fp8_int4', 'linear_sym', 33, 1280, 8192, 256, False, True), 'fp8_int4/linear_sym/g256/<2x2>'),
    (Case('fp8_int4', 'linear_sym', 33, 1280, 8192, 256, True, True), 'fp8_int4/linear_sym/g256/<2x2>'),
    (Case('fp8_int4', 'linear_sym', 1, 48, 4096, 32, False, True), 'fp8_int4/linear_sym/g32/<1x1>'),
    (Case('fp8_int4', 'linear_sym', 1, 48, 4096, 32, True, True), 'fp8_int4/linear_sym/g32/<1x1>'),
    (Case('fp8_int4', 'linear_sym', 17, 48, 4096, 32, False, True), 'fp8_int4/linear_sym/g32/<2x1>'),
    (Case('fp8_int4', 'linear_sym', 17, 48, 4096, 32, True, True), 'fp8_int4/linear_sym/g32/<2x1>'),
    (Case('fp8_int4', 'linear_sym', 1, 48, 4096, 64, False, True), 'fp8_int4/linear_sym/g64/<1x1>'),
    (Case('fp8_int4', 'linear_sym', 1, 48, 4096, 64, True, True), 'fp8_int4/linear_sym/g64/<1x1>'),
    (Case('fp8_int4', 'linear_sym', 17, 48, 4096, 64, False, True), 'fp8_int4/linear_sym/g64/<2x1>'),
    (Case('fp8_int4', 'linear_sym', 17, 48, 4096, 64, True, True), 'fp8_int4/linear_sym/g64/<2x1>'),
    (Case('gemm8', 'fp8_dyn', 1, 8192, 1024, 0, False, True), 'gemm8/fp8_dyn/dec8/w1/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 8192, 1024, 0, True, True), 'gemm8/fp8_dyn/dec8/w1/d8'),
    (Case('gemm8', 'fp8_dyn', 9, 1040, 2560, 0, False, True), 'gemm8/fp8_dyn/dec8/w10/d2/rows8'),
    (Case('gemm8', 'fp8_dyn', 9, 1040, 2560, 0, True, True), 'gemm8/fp8_dyn/dec8/w10/d2/rows8'),
    (Case('gemm8', 'fp8_dyn', 5, 5120, 5120, 0, False, True), 'gemm8/fp8_dyn/dec8/w10/d4'),
    (Case('gemm8', 'fp8_dyn', 5, 5120, 5120, 0, True, True), 'gemm8/fp8_dyn/dec8/w10/d4'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 10240, 0, False, True), 'gemm8/fp8_dyn/dec8/w10/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 10240, 0, True, True), 'gemm8/fp8_dyn/dec8/w10/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 12288, 0, False, True), 'gemm8/fp8_dyn/dec8/w12/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 12288, 0, True, True), 'gemm8/fp8_dyn/dec8/w12/d8'),
    (Case('gemm8', 'fp8_dyn', 9, 3584, 3584, 0, False, True), 'gemm8/fp8_dyn/dec8/w14/d2'),
    (Case('gemm8', 'fp8_dyn', 9, 3584, 3584, 0, True, True), 'gemm8/fp8_dyn/dec8/w14/d2'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 14336, 0, False, True), 'gemm8/fp8_dyn/dec8/w14/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 14336, 0, True, True), 'gemm8/fp8_dyn/dec8/w14/d8'),
    (Case('gemm8', 'fp8_dyn', 5, 7168, 8192, 0, False, True), 'gemm8/fp8_dyn/dec8/w16/d4'),
    (Case('gemm8', 'fp8_dyn', 5, 7168, 8192, 0, True, True), 'gemm8/fp8_dyn/dec8/w16/d4'),
    (Case('gemm8', 'fp8_dyn', 1, 208, 13824, 0, False, True), 'gemm8/fp8_dyn/dec8/w16/d4/loop'),
    (Case('gemm8', 'fp8_dyn', 1, 208, 13824, 0, True, True), 'gemm8/fp8_dyn/dec8/w16/d4/loop'),
    (Case('gemm8', 'fp8_dyn', 5, 1280, 8192, 0, False, True), 'gemm8/fp8_dyn/dec8/w16/d4/rows8'),
    (Case('gemm8', 'fp8_dyn', 5, 1280, 8192, 0, True, True), 'gemm8/fp8_dyn/dec8/w16/d4/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 16384, 0, False, True), 'gemm8/fp8_dyn/dec8/w16/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 16384, 0, True, True), 'gemm8/fp8_dyn/dec8/w16/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 48, 16384, 0, False, True), 'gemm8/fp8_dyn/dec8/w16/d8/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 48, 16384, 0, True, True), 'gemm8/fp8_dyn/dec8/w16/d8/rows8'),
    (Case('gemm8', 'fp8_dyn', 5, 8192, 1024, 0, False, True), 'gemm8/fp8_dyn/dec8/w2/d4'),
    (Case('gemm8', 'fp8_dyn', 5, 8192, 1024, 0, True, True), 'gemm8/fp8_dyn/dec8/w2/d4'),
    (Case('gemm8', 'fp8_dyn', 9, 8192, 1024, 0, False, True), 'gemm8/fp8_dyn/dec8/w4/d2'),
    (Case('gemm8', 'fp8_dyn', 9, 8192, 1024, 0, True, True), 'gemm8/fp8_dyn/dec8/w4/d2'),
    (Case('gemm8', 'fp8_dyn', 1, 3584, 3584, 0, False, True), 'gemm8/fp8_dyn/dec8/w4/d7'),
    (Case('gemm8', 'fp8_dyn', 1, 3584, 3584, 0, True, True), 'gemm8/fp8_dyn/dec8/w4/d7'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 4096, 0, False, True), 'gemm8/fp8_dyn/dec8/w4/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 4096, 4096, 0, True, True), 'gemm8/fp8_dyn/dec8/w4/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 48, 4096, 0, False, True), 'gemm8/fp8_dyn/dec8/w4/d8/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 48, 4096, 0, True, True), 'gemm8/fp8_dyn/dec8/w4/d8/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 1040, 2560, 0, False, True), 'gemm8/fp8_dyn/dec8/w5/d4/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 1040, 2560, 0, True, True), 'gemm8/fp8_dyn/dec8/w5/d4/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 5120, 5120, 0, False, True), 'gemm8/fp8_dyn/dec8/w5/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 5120, 5120, 0, True, True), 'gemm8/fp8_dyn/dec8/w5/d8'),
    (Case('gemm8', 'fp8_dyn', 5, 3584, 3584, 0, False, True), 'gemm8/fp8_dyn/dec8/w7/d4'),
    (Case('gemm8', 'fp8_dyn', 5, 3584, 3584, 0, True, True), 'gemm8/fp8_dyn/dec8/w7/d4'),
    (Case('gemm8', 'fp8_dyn', 5, 4096, 4096, 0, False, True), 'gemm8/fp8_dyn/dec8/w8/d4'),
    (Case('gemm8', 'fp8_dyn', 5, 4096, 4096, 0, True, True), 'gemm8/fp8_dyn/dec8/w8/d4'),
    (Case('gemm8', 'fp8_dyn', 5, 48, 4096, 0, False, True), 'gemm8/fp8_dyn/dec8/w8/d4/rows8'),
    (Case('gemm8', 'fp8_dyn', 5, 48, 4096, 0, True, True), 'gemm8/fp8_dyn/dec8/w8/d4/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 7168, 8192, 0, False, True), 'gemm8/fp8_dyn/dec8/w8/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 7168, 8192, 0, True, True), 'gemm8/fp8_dyn/dec8/w8/d8'),
    (Case('gemm8', 'fp8_dyn', 1, 1280, 8192, 0, False, True), 'gemm8/fp8_dyn/dec8/w8/d8/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 1280, 8192, 0, True, True), 'gemm8/fp8_dyn/dec8/w8/d8/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 208, 1152, 0, False, True), 'gemm8/fp8_dyn/dec8/w9/d1/rows8'),
    (Case('gemm8', 'fp8_dyn', 1, 208, 1152, 0, True, True), 'gemm8/fp8_dyn/dec8/w9/d1/rows8'),
    (Case('gemm8', 'fp8_dyn', 17, 28672, 4096, 0, False, True), 'gemm8/fp8_dyn/mid8/mt2'),
    (Case('gemm8', 'fp8_dyn', 17, 28672, 4096, 0, True, True), 'gemm8/fp8_dyn/mid8/mt2'),
    (Case('gemm8', 'fp8_dyn', 17, 48, 4096, 0, False, True), 'gemm8/fp8_dyn/mid8/mt2/kparts'),
    (Case('gemm8', 'fp8_dyn', 17, 48, 4096, 0, True, True), 'gemm8/fp8_dyn/mid8/mt2/kparts'),
    (Case('gemm8', 'fp8_mm_f32', 1, 48, 4096, 0, False, True), 'gemm8/fp8_mm_f32/dma128/128x128'),
    (Case('gemm8', 'fp8_mm_f32', 1, 37888, 3584, 0, False, True), 'gemm8/fp8_mm_f32/p8/256x256'),
    (Case('gemm8', 'fp8_mm_f32', 257, 16400, 4096, 0, False, True), 'gemm8/fp8_mm_f32/p8/256x256'),
    (Case('gemm8', 'fp8_mm_f32', 513, 8192, 1024, 0, False, True), 'gemm8/fp8_mm_f32/p8h/256x128'),
    (Case('gemm8', 'fp8_mm_f32', 129, 16400, 4096, 0, False, True), 'gemm8/fp8_mm_f32/p8h/256x128'),
    (Case('gemm8', 'fp8_mm_f32', 257, 4096, 10240, 0, False, True), 'gemm8/fp8_mm_f32/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_mm_f32', 4096, 208, 13824, 0, False, True), 'gemm8/fp8_mm_f32/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_mm_f32', 2048, 1280, 8192, 0, False, True), 'gemm8/fp8_mm_f32/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_mm_f32', 1280, 8192, 1024, 0, False, True), 'gemm8/fp8_mm_f32/p8p/256x256'),
    (Case('gemm8', 'fp8_mm_f32', 1, 4112, 1040, 0, False, True), 'gemm8/fp8_mm_f32/regstage/128x128'),
    (Case('gemm8', 'fp8_scaled', 1, 8192, 1024, 0, False, True), 'gemm8/fp8_scaled/dec8/w1/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 8192, 1024, 0, True, True), 'gemm8/fp8_scaled/dec8/w1/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 8192, 1024, 0, False, False), 'gemm8/fp8_scaled/dec8/w1/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 8192, 1024, 0, True, False), 'gemm8/fp8_scaled/dec8/w1/d8'),
    (Case('gemm8', 'fp8_scaled', 9, 1040, 2560, 0, False, True), 'gemm8/fp8_scaled/dec8/w10/d2/rows8'),
    (Case('gemm8', 'fp8_scaled', 9, 1040, 2560, 0, True, True), 'gemm8/fp8_scaled/dec8/w10/d2/rows8'),
    (Case('gemm8', 'fp8_scaled', 5, 5120, 5120, 0, False, True), 'gemm8/fp8_scaled/dec8/w10/d4'),
    (Case('gemm8', 'fp8_scaled', 5, 5120, 5120, 0, True, True), 'gemm8/fp8_scaled/dec8/w10/d4'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 10240, 0, False, True), 'gemm8/fp8_scaled/dec8/w10/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 10240, 0, True, True), 'gemm8/fp8_scaled/dec8/w10/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 12288, 0, False, True), 'gemm8/fp8_scaled/dec8/w12/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 12288, 0, True, True), 'gemm8/fp8_scaled/dec8/w12/d8'),
    (Case('gemm8', 'fp8_scaled', 9, 3584, 3584, 0, False, True), 'gemm8/fp8_scaled/dec8/w14/d2'),
    (Case('gemm8', 'fp8_scaled', 9, 3584, 3584, 0, True, True), 'gemm8/fp8_scaled/dec8/w14/d2'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 14336, 0, False, True), 'gemm8/fp8_scaled/dec8/w14/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 14336, 0, True, True), 'gemm8/fp8_scaled/dec8/w14/d8'),
    (Case('gemm8', 'fp8_scaled', 5, 7168, 8192, 0, False, True), 'gemm8/fp8_scaled/dec8/w16/d4'),
    (Case('gemm8', 'fp8_scaled', 5, 7168, 8192, 0, True, True), 'gemm8/fp8_scaled/dec8/w16/d4'),
    (Case('gemm8', 'fp8_scaled', 1, 208, 13824, 0, False, True), 'gemm8/fp8_scaled/dec8/w16/d4/loop'),
    (Case('gemm8', 'fp8_scaled', 1, 208, 13824, 0, True, True), 'gemm8/fp8_scaled/dec8/w16/d4/loop'),
    (Case('gemm8', 'fp8_scaled', 5, 1280, 8192, 0, False, True), 'gemm8/fp8_scaled/dec8/w16/d4/rows8'),
    (Case('gemm8', 'fp8_scaled', 5, 1280, 8192, 0, True, True), 'gemm8/fp8_scaled/dec8/w16/d4/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 16384, 0, False, True), 'gemm8/fp8_scaled/dec8/w16/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 16384, 0, True, True), 'gemm8/fp8_scaled/dec8/w16/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 48, 16384, 0, False, True), 'gemm8/fp8_scaled/dec8/w16/d8/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 48, 16384, 0, True, True), 'gemm8/fp8_scaled/dec8/w16/d8/rows8'),
    (Case('gemm8', 'fp8_scaled', 5, 8192, 1024, 0, False, True), 'gemm8/fp8_scaled/dec8/w2/d4'),
    (Case('gemm8', 'fp8_scaled', 5, 8192, 1024, 0, True, True), 'gemm8/fp8_scaled/dec8/w2/d4'),
    (Case('gemm8', 'fp8_scaled', 9, 8192, 1024, 0, False, True), 'gemm8/fp8_scaled/dec8/w4/d2'),
    (Case('gemm8', 'fp8_scaled', 9, 8192, 1024, 0, True, True), 'gemm8/fp8_scaled/dec8/w4/d2'),
    (Case('gemm8', 'fp8_scaled', 1, 3584, 3584, 0, False, True), 'gemm8/fp8_scaled/dec8/w4/d7'),
    (Case('gemm8', 'fp8_scaled', 1, 3584, 3584, 0, True, True), 'gemm8/fp8_scaled/dec8/w4/d7'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 4096, 0, False, True), 'gemm8/fp8_scaled/dec8/w4/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 4096, 4096, 0, True, True), 'gemm8/fp8_scaled/dec8/w4/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 48, 4096, 0, False, True), 'gemm8/fp8_scaled/dec8/w4/d8/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 48, 4096, 0, True, True), 'gemm8/fp8_scaled/dec8/w4/d8/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 1040, 2560, 0, False, True), 'gemm8/fp8_scaled/dec8/w5/d4/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 1040, 2560, 0, True, True), 'gemm8/fp8_scaled/dec8/w5/d4/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 5120, 5120, 0, False, True), 'gemm8/fp8_scaled/dec8/w5/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 5120, 5120, 0, True, True), 'gemm8/fp8_scaled/dec8/w5/d8'),
    (Case('gemm8', 'fp8_scaled', 5, 3584, 3584, 0, False, True), 'gemm8/fp8_scaled/dec8/w7/d4'),
    (Case('gemm8', 'fp8_scaled', 5, 3584, 3584, 0, True, True), 'gemm8/fp8_scaled/dec8/w7/d4'),
    (Case('gemm8', 'fp8_scaled', 5, 4096, 4096, 0, False, True), 'gemm8/fp8_scaled/dec8/w8/d4'),
    (Case('gemm8', 'fp8_scaled', 5, 4096, 4096, 0, True, True), 'gemm8/fp8_scaled/dec8/w8/d4'),
    (Case('gemm8', 'fp8_scaled', 5, 48, 4096, 0, False, True), 'gemm8/fp8_scaled/dec8/w8/d4/rows8'),
    (Case('gemm8', 'fp8_scaled', 5, 48, 4096, 0, True, True), 'gemm8/fp8_scaled/dec8/w8/d4/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 7168, 8192, 0, False, True), 'gemm8/fp8_scaled/dec8/w8/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 7168, 8192, 0, True, True), 'gemm8/fp8_scaled/dec8/w8/d8'),
    (Case('gemm8', 'fp8_scaled', 1, 1280, 8192, 0, False, True), 'gemm8/fp8_scaled/dec8/w8/d8/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 1280, 8192, 0, True, True), 'gemm8/fp8_scaled/dec8/w8/d8/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 208, 1152, 0, False, True), 'gemm8/fp8_scaled/dec8/w9/d1/rows8'),
    (Case('gemm8', 'fp8_scaled', 1, 208, 1152, 0, True, True), 'gemm8/fp8_scaled/dec8/w9/d1/rows8'),
    (Case('gemm8', 'fp8_scaled', 17, 28672, 4096, 0, False, True), 'gemm8/fp8_scaled/mid8/mt2'),
    (Case('gemm8', 'fp8_scaled', 17, 28672, 4096, 0, True, True), 'gemm8/fp8_scaled/mid8/mt2'),
    (Case('gemm8', 'fp8_scaled', 17, 28672, 4096, 0, False, False), 'gemm8/fp8_scaled/mid8/mt2'),
    (Case('gemm8', 'fp8_scaled', 17, 28672, 4096, 0, True, False), 'gemm8/fp8_scaled/mid8/mt2'),
    (Case('gemm8', 'fp8_scaled', 17, 48, 4096, 0, False, True), 'gemm8/fp8_scaled/mid8/mt2/kparts'),
    (Case('gemm8', 'fp8_scaled', 17, 48, 4096, 0, True, True), 'gemm8/fp8_scaled/mid8/mt2/kparts'),
    (Case('gemm8', 'fp8_scaled', 65, 37888, 3584, 0, False, True), 'gemm8/fp8_scaled/p8/256x256'),
    (Case('gemm8', 'fp8_scaled', 65, 37888, 3584, 0, True, True), 'gemm8/fp8_scaled/p8/256x256'),
    (Case('gemm8', 'fp8_scaled', 257, 16400, 4096, 0, False, True), 'gemm8/fp8_scaled/p8/256x256'),
    (Case('gemm8', 'fp8_scaled', 257, 16400, 4096, 0, True, True), 'gemm8/fp8_scaled/p8/256x256'),
    (Case('gemm8', 'fp8_scaled', 1280, 8192, 1024, 0, False, False), 'gemm8/fp8_scaled/p8/256x256'),
    (Case('gemm8', 'fp8_scaled', 1280, 8192, 1024, 0, True, False), 'gemm8/fp8_scaled/p8/256x256'),
    (Case('gemm8', 'fp8_scaled', 513, 8192, 1024, 0, False, True), 'gemm8/fp8_scaled/p8h/256x128'),
    (Case('gemm8', 'fp8_scaled', 513, 8192, 1024, 0, True, True), 'gemm8/fp8_scaled/p8h/256x128'),
    (Case('gemm8', 'fp8_scaled', 129, 16400, 4096, 0, False, True), 'gemm8/fp8_scaled/p8h/256x128'),
    (Case('gemm8', 'fp8_scaled', 129, 16400, 4096, 0, True, True), 'gemm8/fp8_scaled/p8h/256x128'),
    (Case('gemm8', 'fp8_scaled', 513, 8192, 1024, 0, False, False), 'gemm8/fp8_scaled/p8h/256x128'),
    (Case('gemm8', 'fp8_scaled', 513, 8192, 1024, 0, True, False), 'gemm8/fp8_scaled/p8h/256x128'),
    (Case('gemm8', 'fp8_scaled', 257, 4096, 10240, 0, False, True), 'gemm8/fp8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 257, 4096, 10240, 0, True, True), 'gemm8/fp8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 4096, 208, 13824, 0, False, True), 'gemm8/fp8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 4096, 208, 13824, 0, True, True), 'gemm8/fp8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 2048, 1280, 8192, 0, False, True), 'gemm8/fp8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 2048, 1280, 8192, 0, True, True), 'gemm8/fp8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 1280, 8192, 1024, 0, False, True), 'gemm8/fp8_scaled/p8p/256x256'),
    (Case('gemm8', 'fp8_scaled', 1280, 8192, 1024, 0, True, True), 'gemm8/fp8_scaled/p8p/256x256'),
    (Case('gemm8', 'fp8_scaled', 257, 8192, 1024, 0, False, True), 'gemm8/fp8_scaled/rb8/128x128'),
    (Case('gemm8', 'fp8_scaled', 257, 8192, 1024, 0, True, True), 'gemm8/fp8_scaled/rb8/128x128'),
    (Case('gemm8', 'fp8_scaled', 65, 16400, 4096, 0, False, True), 'gemm8/fp8_scaled/rb8/128x128'),
    (Case('gemm8', 'fp8_scaled', 65, 16400, 4096, 0, True, True), 'gemm8/fp8_scaled/rb8/128x128'),
    (Case('gemm8', 'fp8_scaled', 257, 8192, 1024, 0, False, False), 'gemm8/fp8_scaled/rb8/128x128'),
    (Case('gemm8', 'fp8_scaled', 257, 8192, 1024, 0, True, False), 'gemm8/fp8_scaled/rb8/128x128'),
    (Case('gemm8', 'fp8_scaled', 513, 1280, 8192, 0, False, True), 'gemm8/fp8_scaled/rb8/128x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 513, 1280, 8192, 0, True, True), 'gemm8/fp8_scaled/rb8/128x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 513, 208, 1152, 0, False, True), 'gemm8/fp8_scaled/rb8/128x32'),
    (Case('gemm8', 'fp8_scaled', 513, 208, 1152, 0, True, True), 'gemm8/fp8_scaled/rb8/128x32'),
    (Case('gemm8', 'fp8_scaled', 513, 48, 4096, 0, False, True), 'gemm8/fp8_scaled/rb8/128x32/kparts'),
    (Case('gemm8', 'fp8_scaled', 513, 48, 4096, 0, True, True), 'gemm8/fp8_scaled/rb8/128x32/kparts'),
    (Case('gemm8', 'fp8_scaled', 1024, 1040, 2560, 0, False, True), 'gemm8/fp8_scaled/rb8/128x64'),
    (Case('gemm8', 'fp8_scaled', 1024, 1040, 2560, 0, True, True), 'gemm8/fp8_scaled/rb8/128x64'),
    (Case('gemm8', 'fp8_scaled', 513, 1040, 2560, 0, False, True), 'gemm8/fp8_scaled/rb8/128x64/kparts'),
    (Case('gemm8', 'fp8_scaled', 513, 1040, 2560, 0, True, True), 'gemm8/fp8_scaled/rb8/128x64/kparts'),
    (Case('gemm8', 'fp8_scaled', 129, 8192, 1024, 0, False, True), 'gemm8/fp8_scaled/rb8/64x128'),
    (Case('gemm8', 'fp8_scaled', 129, 8192, 1024, 0, True, True), 'gemm8/fp8_scaled/rb8/64x128'),
    (Case('gemm8', 'fp8_scaled', 17, 16400, 4096, 0, False, True), 'gemm8/fp8_scaled/rb8/64x128'),
    (Case('gemm8', 'fp8_scaled', 17, 16400, 4096, 0, True, True), 'gemm8/fp8_scaled/rb8/64x128'),
    (Case('gemm8', 'fp8_scaled', 33, 6144, 4096, 0, False, True), 'gemm8/fp8_scaled/rb8/64x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 33, 6144, 4096, 0, True, True), 'gemm8/fp8_scaled/rb8/64x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 65, 4608, 3584, 0, False, True), 'gemm8/fp8_scaled/rb8/64x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 65, 4608, 3584, 0, True, True), 'gemm8/fp8_scaled/rb8/64x128/kparts'),
    (Case('gemm8', 'fp8_scaled', 33, 208, 1152, 0, False, True), 'gemm8/fp8_scaled/rb8/64x32'),
    (Case('gemm8', 'fp8_scaled', 33, 208, 1152, 0, True, True), 'gemm8/fp8_scaled/rb8/64x32'),
    (Case('gemm8', 'fp8_scaled', 33, 48, 4096, 0, False, True), 'gemm8/fp8_scaled/rb8/64x32/kparts'),
    (Case('gemm8', 'fp8_scaled', 33, 48, 4096, 0, True, True), 'gemm8/fp8_scaled/rb8/64x32/kparts'),
    (Case('gemm8', 'fp8_scaled', 33, 208, 13824, 0, False, True), 'gemm8/fp8_scaled/rb8/64x32/kparts'),
    (Case('gemm8', 'fp8_scaled', 33, 208, 13824, 0, True, True), 'gemm8/fp8_scaled/rb8/64x32/kparts'),
    (Case('gemm8', 'fp8_scaled', 65, 8192, 1024, 0, False, True), 'gemm8/fp8_scaled/rb8/64x64'),
    (Case('gemm8', 'fp8_scaled', 65, 8192, 1024, 0, True, True), 'gemm8/fp8_scaled/rb8/64x64'),
    (Case('gemm8', 'fp8_scaled', 511, 1040, 2560, 0, False, True), 'gemm8/fp8_scaled/rb8/64x64'),
    (Case('gemm8', 'fp8_scaled', 511, 1040, 2560, 0, True, True), 'gemm8/fp8_scaled/rb8/64x64'),
    (Case('gemm8', 'fp8_scaled', 17, 4608, 3584, 0, False, True), 'gemm8/fp8_scaled/rb8/64x64/kparts'),
    (Case('gemm8', 'fp8_scaled', 17, 4608, 3584, 0, True, True), 'gemm8/fp8_scaled/rb8/64x64/kparts'),
    (Case('gemm8', 'fp8_scaled', 129, 1040, 2560, 0, False, True), 'gemm8/fp8_scaled/rb8/64x64/kparts'),
    (Case('gemm8', 'fp8_scaled', 129, 1040, 2560, 0, True, True), 'gemm8/fp8_scaled/rb8/64x64/kparts'),
    (Case('gemm8', 'fp8_scaled', 1, 4112, 1040, 0, False, True), 'gemm8/fp8_scaled/regstage/128x128'),
    (Case('gemm8', 'fp8_scaled', 1, 4112, 1040, 0, True, True), 'gemm8/fp8_scaled/regstage/128x128'),
    (Case('gemm8', 'fp8_scaled', 1, 4112, 1040, 0, False, False), 'gemm8/fp8_scaled/regstage/128x128'),
    (Case('gemm8', 'fp8_scaled', 1, 4112, 1040, 0, True, False), 'gemm8/fp8_scaled/regstage/128x128'),
    (Case('gemm8', 'fp8_scaled', 17, 208, 1152, 0, False, True), 'gemm8/fp8_scaled/stream8'),
    (Case('gemm8', 'fp8_scaled', 17, 208, 1152, 0, True, True), 'gemm8/fp8_scaled/stream8'),
    (Case('gemm8', 'fp8_scaled', 17, 208, 1152, 0, False, False), 'gemm8/fp8_scaled/stream8'),
    (Case('gemm8', 'fp8_scaled', 17, 208, 1152, 0, True, False), 'gemm8/fp8_scaled/stream8'),
    (Case('gemm8', 'int8_dyn', 1, 8192, 1024, 0, False, True), 'gemm8/int8_dyn/dec8/w1/d8'),
    (Case('gemm8', 'int8_dyn', 1, 8192, 1024, 0, True, True), 'gemm8/int8_dyn/dec8/w1/d8'),
    (Case('gemm8', 'int8_dyn', 9, 1040, 2560, 0, False, True), 'gemm8/int8_dyn/dec8/w10/d2/rows8'),
    (Case('gemm8', 'int8_dyn', 9, 1040, 2560, 0, True, True), 'gemm8/int8_dyn/dec8/w10/d2/rows8'),
    (Case('gemm8', 'int8_dyn', 5, 5120, 5120, 0, False, True), 'gemm8/int8_dyn/dec8/w10/d4'),
    (Case('gemm8', 'int8_dyn', 5, 5120, 5120, 0, True, True), 'gemm8/int8_dyn/dec8/w10/d4'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 10240, 0, False, True), 'gemm8/int8_dyn/dec8/w10/d8'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 10240, 0, True, True), 'gemm8/int8_dyn/dec8/w10/d8'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 12288, 0, False, True), 'gemm8/int8_dyn/dec8/w12/d8'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 12288, 0, True, True), 'gemm8/int8_dyn/dec8/w12/d8'),
    (Case('gemm8', 'int8_dyn', 9, 3584, 3584, 0, False, True), 'gemm8/int8_dyn/dec8/w14/d2'),
    (Case('gemm8', 'int8_dyn', 9, 3584, 3584, 0, True, True), 'gemm8/int8_dyn/dec8/w14/d2'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 14336, 0, False, True), 'gemm8/int8_dyn/dec8/w14/d8'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 14336, 0, True, True), 'gemm8/int8_dyn/dec8/w14/d8'),
    (Case('gemm8', 'int8_dyn', 5, 7168, 8192, 0, False, True), 'gemm8/int8_dyn/dec8/w16/d4'),
    (Case('gemm8', 'int8_dyn', 5, 7168, 8192, 0, True, True), 'gemm8/int8_dyn/dec8/w16/d4'),
    (Case('gemm8', 'int8_dyn', 1, 208, 13824, 0, False, True), 'gemm8/int8_dyn/dec8/w16/d4/loop'),
    (Case('gemm8', 'int8_dyn', 1, 208, 13824, 0, True, True), 'gemm8/int8_dyn/dec8/w16/d4/loop'),
    (Case('gemm8', 'int8_dyn', 5, 1280, 8192, 0, False, True), 'gemm8/int8_dyn/dec8/w16/d4/rows8'),
    (Case('gemm8', 'int8_dyn', 5, 1280, 8192, 0, True, True), 'gemm8/int8_dyn/dec8/w16/d4/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 16384, 0, False, True), 'gemm8/int8_dyn/dec8/w16/d8'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 16384, 0, True, True), 'gemm8/int8_dyn/dec8/w16/d8'),
    (Case('gemm8', 'int8_dyn', 1, 48, 16384, 0, False, True), 'gemm8/int8_dyn/dec8/w16/d8/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 48, 16384, 0, True, True), 'gemm8/int8_dyn/dec8/w16/d8/rows8'),
    (Case('gemm8', 'int8_dyn', 5, 8192, 1024, 0, False, True), 'gemm8/int8_dyn/dec8/w2/d4'),
    (Case('gemm8', 'int8_dyn', 5, 8192, 1024, 0, True, True), 'gemm8/int8_dyn/dec8/w2/d4'),
    (Case('gemm8', 'int8_dyn', 9, 8192, 1024, 0, False, True), 'gemm8/int8_dyn/dec8/w4/d2'),
    (Case('gemm8', 'int8_dyn', 9, 8192, 1024, 0, True, True), 'gemm8/int8_dyn/dec8/w4/d2'),
    (Case('gemm8', 'int8_dyn', 1, 3584, 3584, 0, False, True), 'gemm8/int8_dyn/dec8/w4/d7'),
    (Case('gemm8', 'int8_dyn', 1, 3584, 3584, 0, True, True), 'gemm8/int8_dyn/dec8/w4/d7'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 4096, 0, False, True), 'gemm8/int8_dyn/dec8/w4/d8'),
    (Case('gemm8', 'int8_dyn', 1, 4096, 4096, 0, True, True), 'gemm8/int8_dyn/dec8/w4/d8'),
    (Case('gemm8', 'int8_dyn', 1, 48, 4096, 0, False, True), 'gemm8/int8_dyn/dec8/w4/d8/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 48, 4096, 0, True, True), 'gemm8/int8_dyn/dec8/w4/d8/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 1040, 2560, 0, False, True), 'gemm8/int8_dyn/dec8/w5/d4/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 1040, 2560, 0, True, True), 'gemm8/int8_dyn/dec8/w5/d4/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 5120, 5120, 0, False, True), 'gemm8/int8_dyn/dec8/w5/d8'),
    (Case('gemm8', 'int8_dyn', 1, 5120, 5120, 0, True, True), 'gemm8/int8_dyn/dec8/w5/d8'),
    (Case('gemm8', 'int8_dyn', 5, 3584, 3584, 0, False, True), 'gemm8/int8_dyn/dec8/w7/d4'),
    (Case('gemm8', 'int8_dyn', 5, 3584, 3584, 0, True, True), 'gemm8/int8_dyn/dec8/w7/d4'),
    (Case('gemm8', 'int8_dyn', 5, 4096, 4096, 0, False, True), 'gemm8/int8_dyn/dec8/w8/d4'),
    (Case('gemm8', 'int8_dyn', 5, 4096, 4096, 0, True, True), 'gemm8/int8_dyn/dec8/w8/d4'),
    (Case('gemm8', 'int8_dyn', 5, 48, 4096, 0, False, True), 'gemm8/int8_dyn/dec8/w8/d4/rows8'),
    (Case('gemm8', 'int8_dyn', 5, 48, 4096, 0, True, True), 'gemm8/int8_dyn/dec8/w8/d4/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 7168, 8192, 0, False, True), 'gemm8/int8_dyn/dec8/w8/d8'),
    (Case('gemm8', 'int8_dyn', 1, 7168, 8192, 0, True, True), 'gemm8/int8_dyn/dec8/w8/d8'),
    (Case('gemm8', 'int8_dyn', 1, 1280, 8192, 0, False, True), 'gemm8/int8_dyn/dec8/w8/d8/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 1280, 8192, 0, True, True), 'gemm8/int8_dyn/dec8/w8/d8/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 208, 1152, 0, False, True), 'gemm8/int8_dyn/dec8/w9/d1/rows8'),
    (Case('gemm8', 'int8_dyn', 1, 208, 1152, 0, True, True), 'gemm8/int8_dyn/dec8/w9/d1/rows8'),
    (Case('gemm8', 'int8_dyn', 17, 28672, 4096, 0, False, True), 'gemm8/int8_dyn/mid8/mt2'),
    (Case('gemm8', 'int8_dyn', 17, 28672, 4096, 0, True, True), 'gemm8/int8_dyn/mid8/mt2'),
    (Case('gemm8', 'int8_dyn', 17, 48, 4096, 0, False, True), 'gemm8/int8_dyn/mid8/mt2/kparts'),
    (Case('gemm8', 'int8_dyn', 17, 48, 4096, 0, True, True), 'gemm8/int8_dyn/mid8/mt2/kparts'),
    (Case('gemm8', 'int8_scaled', 1, 8192, 1024, 0, False, True), 'gemm8/int8_scaled/dec8/w1/d8'),
    (Case('gemm8', 'int8_scaled', 1, 8192, 1024, 0, True, True), 'gemm8/int8_scaled/dec8/w1/d8'),
    (Case('gemm8', 'int8_scaled', 1, 8192, 1024, 0, False, False), 'gemm8/int8_scaled/dec8/w1/d8'),
    (Case('gemm8', 'int8_scaled', 1, 8192, 1024, 0, True, False), 'gemm8/int8_scaled/dec8/w1/d8'),
    (Case('gemm8', 'int8_scaled', 9, 1040, 2560, 0, False, True), 'gemm8/int8_scaled/dec8/w10/d2/rows8'),
    (Case('gemm8', 'int8_scaled', 9, 1040, 2560, 0, True, True), 'gemm8/int8_scaled/dec8/w10/d2/rows8'),
    (Case('gemm8', 'int8_scaled', 5, 5120, 5120, 0, False, True), 'gemm8/int8_scaled/dec8/w10/d4'),
    (Case('gemm8', 'int8_scaled', 5, 5120, 5120, 0, True, True), 'gemm8/int8_scaled/dec8/w10/d4'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 10240, 0, False, True), 'gemm8/int8_scaled/dec8/w10/d8'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 10240, 0, True, True), 'gemm8/int8_scaled/dec8/w10/d8'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 12288, 0, False, True), 'gemm8/int8_scaled/dec8/w12/d8'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 12288, 0, True, True), 'gemm8/int8_scaled/dec8/w12/d8'),
    (Case('gemm8', 'int8_scaled', 9, 3584, 3584, 0, False, True), 'gemm8/int8_scaled/dec8/w14/d2'),
    (Case('gemm8', 'int8_scaled', 9, 3584, 3584, 0, True, True), 'gemm8/int8_scaled/dec8/w14/d2'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 14336, 0, False, True), 'gemm8/int8_scaled/dec8/w14/d8'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 14336, 0, True, True), 'gemm8/int8_scaled/dec8/w14/d8'),
    (Case('gemm8', 'int8_scaled', 5, 7168, 8192, 0, False, True), 'gemm8/int8_scaled/dec8/w16/d4'),
    (Case('gemm8', 'int8_scaled', 5, 7168, 8192, 0, True, True), 'gemm8/int8_scaled/dec8/w16/d4'),
    (Case('gemm8', 'int8_scaled', 1, 208, 13824, 0, False, True), 'gemm8/int8_scaled/dec8/w16/d4/loop'),
    (Case('gemm8', 'int8_scaled', 1, 208, 13824, 0, True, True), 'gemm8/int8_scaled/dec8/w16/d4/loop'),
    (Case('gemm8', 'int8_scaled', 5, 1280, 8192, 0, False, True), 'gemm8/int8_scaled/dec8/w16/d4/rows8'),
    (Case('gemm8', 'int8_scaled', 5, 1280, 8192, 0, True, True), 'gemm8/int8_scaled/dec8/w16/d4/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 16384, 0, False, True), 'gemm8/int8_scaled/dec8/w16/d8'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 16384, 0, True, True), 'gemm8/int8_scaled/dec8/w16/d8'),
    (Case('gemm8', 'int8_scaled', 1, 48, 16384, 0, False, True), 'gemm8/int8_scaled/dec8/w16/d8/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 48, 16384, 0, True, True), 'gemm8/int8_scaled/dec8/w16/d8/rows8'),
    (Case('gemm8', 'int8_scaled', 5, 8192, 1024, 0, False, True), 'gemm8/int8_scaled/dec8/w2/d4'),
    (Case('gemm8', 'int8_scaled', 5, 8192, 1024, 0, True, True), 'gemm8/int8_scaled/dec8/w2/d4'),
    (Case('gemm8', 'int8_scaled', 9, 8192, 1024, 0, False, True), 'gemm8/int8_scaled/dec8/w4/d2'),
    (Case('gemm8', 'int8_scaled', 9, 8192, 1024, 0, True, True), 'gemm8/int8_scaled/dec8/w4/d2'),
    (Case('gemm8', 'int8_scaled', 1, 3584, 3584, 0, False, True), 'gemm8/int8_scaled/dec8/w4/d7'),
    (Case('gemm8', 'int8_scaled', 1, 3584, 3584, 0, True, True), 'gemm8/int8_scaled/dec8/w4/d7'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 4096, 0, False, True), 'gemm8/int8_scaled/dec8/w4/d8'),
    (Case('gemm8', 'int8_scaled', 1, 4096, 4096, 0, True, True), 'gemm8/int8_scaled/dec8/w4/d8'),
    (Case('gemm8', 'int8_scaled', 1, 48, 4096, 0, False, True), 'gemm8/int8_scaled/dec8/w4/d8/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 48, 4096, 0, True, True), 'gemm8/int8_scaled/dec8/w4/d8/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 1040, 2560, 0, False, True), 'gemm8/int8_scaled/dec8/w5/d4/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 1040, 2560, 0, True, True), 'gemm8/int8_scaled/dec8/w5/d4/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 5120, 5120, 0, False, True), 'gemm8/int8_scaled/dec8/w5/d8'),
    (Case('gemm8', 'int8_scaled', 1, 5120, 5120, 0, True, True), 'gemm8/int8_scaled/dec8/w5/d8'),
    (Case('gemm8', 'int8_scaled', 5, 3584, 3584, 0, False, True), 'gemm8/int8_scaled/dec8/w7/d4'),
    (Case('gemm8', 'int8_scaled', 5, 3584, 3584, 0, True, True), 'gemm8/int8_scaled/dec8/w7/d4'),
    (Case('gemm8', 'int8_scaled', 5, 4096, 4096, 0, False, True), 'gemm8/int8_scaled/dec8/w8/d4'),
    (Case('gemm8', 'int8_scaled', 5, 4096, 4096, 0, True, True), 'gemm8/int8_scaled/dec8/w8/d4'),
    (Case('gemm8', 'int8_scaled', 5, 48, 4096, 0, False, True), 'gemm8/int8_scaled/dec8/w8/d4/rows8'),
    (Case('gemm8', 'int8_scaled', 5, 48, 4096, 0, True, True), 'gemm8/int8_scaled/dec8/w8/d4/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 7168, 8192, 0, False, True), 'gemm8/int8_scaled/dec8/w8/d8'),
    (Case('gemm8', 'int8_scaled', 1, 7168, 8192, 0, True, True), 'gemm8/int8_scaled/dec8/w8/d8'),
    (Case('gemm8', 'int8_scaled', 1, 1280, 8192, 0, False, True), 'gemm8/int8_scaled/dec8/w8/d8/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 1280, 8192, 0, True, True), 'gemm8/int8_scaled/dec8/w8/d8/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 208, 1152, 0, False, True), 'gemm8/int8_scaled/dec8/w9/d1/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 208, 1152, 0, True, True), 'gemm8/int8_scaled/dec8/w9/d1/rows8'),
    (Case('gemm8', 'int8_scaled', 1, 1000, 4096, 0, False, True), 'gemm8/int8_scaled/dma128/128x128'),
    (Case('gemm8', 'int8_scaled', 1, 1000, 4096, 0, True, True), 'gemm8/int8_scaled/dma128/128x128'),
    (Case('gemm8', 'int8_scaled', 1, 1000, 4096, 0, False, False), 'gemm8/int8_scaled/dma128/128x128'),
    (Case('gemm8', 'int8_scaled', 1, 1000, 4096, 0, True, False), 'gemm8/int8_scaled/dma128/128x128'),
    (Case('gemm8', 'int8_scaled', 17, 28672, 4096, 0, False, True), 'gemm8/int8_scaled/mid8/mt2'),
    (Case('gemm8', 'int8_scaled', 17, 28672, 4096, 0, True, True), 'gemm8/int8_scaled/mid8/mt2'),
    (Case('gemm8', 'int8_scaled', 17, 28672, 4096, 0, False, False), 'gemm8/int8_scaled/mid8/mt2'),
    (Case('gemm8', 'int8_scaled', 17, 28672, 4096, 0, True, False), 'gemm8/int8_scaled/mid8/mt2'),
    (Case('gemm8', 'int8_scaled', 17, 48, 4096, 0, False, True), 'gemm8/int8_scaled/mid8/mt2/kparts'),
    (Case('gemm8', 'int8_scaled', 17, 48, 4096, 0, True, True), 'gemm8/int8_scaled/mid8/mt2/kparts'),
    (Case('gemm8', 'int8_scaled', 65, 37888, 3584, 0, False, True), 'gemm8/int8_scaled/p8/256x256'),
    (Case('gemm8', 'int8_scaled', 65, 37888, 3584, 0, True, True), 'gemm8/int8_scaled/p8/256x256'),
    (Case('gemm8', 'int8_scaled', 257, 16400, 4096, 0, False, True), 'gemm8/int8_scaled/p8/256x256'),
    (Case('gemm8', 'int8_scaled', 257, 16400, 4096, 0, True, True), 'gemm8/int8_scaled/p8/256x256'),
    (Case('gemm8', 'int8_scaled', 1280, 8192, 1024, 0, False, False), 'gemm8/int8_scaled/p8/256x256'),
    (Case('gemm8', 'int8_scaled', 1280, 8192, 1024, 0, True, False), 'gemm8/int8_scaled/p8/256x256'),
    (Case('gemm8', 'int8_scaled', 513, 8192, 1024, 0, False, True), 'gemm8/int8_scaled/p8h/256x128'),
    (Case('gemm8', 'int8_scaled', 513, 8192, 1024, 0, True, True), 'gemm8/int8_scaled/p8h/256x128'),
    (Case('gemm8', 'int8_scaled', 129, 16400, 4096, 0, False, True), 'gemm8/int8_scaled/p8h/256x128'),
    (Case('gemm8', 'int8_scaled', 129, 16400, 4096, 0, True, True), 'gemm8/int8_scaled/p8h/256x128'),
    (Case('gemm8', 'int8_scaled', 513, 8192, 1024, 0, False, False), 'gemm8/int8_scaled/p8h/256x128'),
    (Case('gemm8', 'int8_scaled', 513, 8192, 1024, 0, True, False), 'gemm8/int8_scaled/p8h/256x128'),
    (Case('gemm8', 'int8_scaled', 257, 4096, 10240, 0, False, True), 'gemm8/int8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'int8_scaled', 257, 4096, 10240, 0, True, True), 'gemm8/int8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'int8_scaled', 4096, 208, 13824, 0, False, True), 'gemm8/int8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'int8_scaled', 4096, 208, 13824, 0, True, True), 'gemm8/int8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'int8_scaled', 2048, 1280, 8192, 0, False, True), 'gemm8/int8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'int8_scaled', 2048, 1280, 8192, 0, True, True), 'gemm8/int8_scaled/p8h/256x128/kparts'),
    (Case('gemm8', 'int8_scaled', 1280, 8192, 1024, 0, False, True), 'gemm8/int8_scaled/p8p/256x256'),
    (Case('gemm8', 'int8_scaled', 1280, 8192, 1024, 0, True, True), 'gemm8/int8_scaled/p8p/256x256'),
    (Case('gemm8', 'int8_scaled', 257, 8192, 1024, 0, False, True), 'gemm8/int8_scaled/rb8/128x128'),
    (Case('gemm8', 'int8_scaled', 257, 8192, 1024, 0, True, True), 'gemm8/int8_scaled/rb8/128x128'),
    (Case('gemm8', 'int8_scaled', 65, 16400, 4096, 0, False, True), 'gemm8/int8_scaled/rb8/128x128'),
    (Case('gemm8', 'int8_scaled', 65, 16400, 4096, 0, True, True), 'gemm8/int8_scaled/rb8/128x128'),
    (Case('gemm8', 'int8_scaled', 257, 8192, 1024, 0, False, False), 'gemm8/int8_scaled/rb8/128x128'),
    (Case('gemm8', 'int8_scaled', 257, 8192, 1024, 0, True, False), 'gemm8/int8_scaled/rb8/128x128'),
    (Case('gemm8', 'int8_scaled', 513, 1280, 8192, 0, False, True), 'gemm8/int8_scaled/rb8/128x128/kparts'),
    (Case('gemm8', 'int8_scaled', 513, 1280, 8192, 0, True, True), 'gemm8/int8_scaled/rb8/128x128/kparts'),
    (Case('gemm8', 'int8_scaled', 513, 208, 1152, 0, False, True), 'gemm8/int8_scaled/rb8/128x32'),
    (Case('gemm8', 'int8_scaled', 513, 208, 1152, 0, True, True), 'gemm8/int8_scaled/rb8/128x32'),
    (Case('gemm8', 'int8_scaled', 513, 48, 4096, 0, False, True), 'gemm8/int8_scaled/rb8/128x32/kparts'),
    (Case('gemm8', 'int8_scaled', 513, 48, 4096, 0, True, True), 'gemm8/int8_scaled/rb8/128x32/kparts'),
    (Case('gemm8', 'int8_scaled', 1024, 1040, 2560, 0, False, True), 'gemm8/int8_scaled/rb8/128x64'),
    (Case('gemm8', 'int8_scaled', 1024, 1040, 2560, 0, True, True), 'gemm8/int8_scaled/rb8/128x64'),
    (Case('gemm8', 'int8_scaled', 513, 1040, 2560, 0, False, True), 'gemm8/int8_scaled/rb8/128x64/kparts'),
    (Case('gemm8', 'int8_scaled', 513, 1040, 2560, 0, True, True), 'gemm8/int8_scaled/rb8/128x64/kparts'),
    (Case('gemm8', 'int8_scaled', 129, 8192, 1024, 0, False, True), 'gemm8/int8_scaled/rb8/64x128'),
    (Case('gemm8', 'int8_scaled', 129, 8192, 1024, 0, True, True), 'gemm8/int8_scaled/rb8/64x128'),
    (Case('gemm8', 'int8_scaled', 17, 16400, 4096, 0, False, True), 'gemm8/int8_scaled/rb8/64x128'),
    (Case('gemm8', 'int8_scaled', 17, 16400, 4096, 0, True, True), 'gemm8/int8_scaled/rb8/64x128'),
    (Case('gemm8', 'int8_scaled', 33, 6144, 4096, 0, False, True), 'gemm8/int8_scaled/rb8/64x128/kparts'),
    (Case('gemm8', 'int8_scaled', 33, 6144, 4096, 0, True, True), 'gemm8/int8_scaled/rb8/64x128/kparts'),
    (Case('gemm8', 'int8_scaled', 65, 4608, 3584, 0, False, True), 'gemm8/int8_scaled/rb8/64x128/kparts'),
    (Case('gemm8', 'int8_scaled', 65, 4608, 3584, 0, True, True), 'gemm8/int8_scaled/rb8/64x128/kparts'),
    (Case('gemm8', 'int8_scaled', 33, 208, 1152, 0, False, True), 'gemm8/int8_scaled/rb8/64x32'),
    (Case('gemm8', 'int8_scaled', 33, 208, 1152, 0, True, True), 'gemm8/int8_scaled/rb8/64x32'),
    (Case('gemm8', 'int8_scaled', 33, 48, 4096, 0, False, True), 'gemm8/int8_scaled/rb8/64x32/kparts'),
    (Case('gemm8', 'int8_scaled', 33, 48, 4096, 0, True, True), 'gemm8/int8_scaled/rb8/64x32/kparts'),
    (Case('gemm8', 'int8_scaled', 33, 208, 13824, 0, False, True), 'gemm8/int8_scaled/rb8/64x32/kparts'),
    (Case('gemm8', 'int8_scaled', 33, 208, 13824, 0, True, True), 'gemm8/int8_scaled/rb8/64x32/kparts'),
    (Case('gemm8', 'int8_scaled', 65, 8192, 1024, 0, False, True), 'gemm8/int8_scaled/rb8/64x64'),
    (Case('gemm8', 'int8_scaled', 65, 8192, 1024, 0, True, True), 'gemm8/int8_scaled/rb8/64x64'),
    (Case('gemm8', 'int8_scaled', 511, 1040, 2560, 0, False, True), 'gemm8/int8_scaled/rb8/64x64'),
    (Case('gemm8', 'int8_scaled', 511, 1040, 2560, 0, True, True), 'gemm8/int8_scaled/rb8/64x64'),
    (Case('gemm8', 'int8_scaled', 17, 4608, 3584, 0, False, True), 'gemm8/int8_scaled/rb8/64x64/kparts'),
    (Case('gemm8', 'int8_scaled', 17, 4608, 3584, 0, True, True), 'gemm8/int8_scaled/rb8/64x64/kparts'),
    (Case('gemm8', 'int8_scaled', 129, 1040, 2560, 0, False, True), 'gemm8/int8_scaled/rb8/64x64/kparts'),
    (Case('gemm8', 'int8_scaled', 129, 1040, 2560, 0, True, True), 'gemm8/int8_scaled/rb8/64x64/kparts'),
    (Case('gemm8', 'int8_scaled', 1, 4112, 1040, 0, False, True), 'gemm8/int8_scaled/regstage/128x128'),
    (Case('gemm8', 'int8_scaled', 1, 4112, 1040, 0, True, True), 'gemm8/int8_scaled/regstage/128x128'),
    (Case('gemm8', 'int8_scaled', 1, 4112, 1040, 0, False, False), 'gemm8/int8_scaled/regstage/128x128'),
    (Case('gemm8', 'int8_scaled', 1, 4112, 1040, 0, True, False), 'gemm8/int8_scaled/regstage/128x128'),
    (Case('gemm8', 'int8_scaled', 17, 208, 1152, 0, False, True), 'gemm8/int8_scaled/stream8'),
    (Case('gemm8', 'int8_scaled', 17, 208, 1152, 0, True, True), 'gemm8/int8_scaled/stream8'),
    (Case('gemm8', 'int8_scaled', 17, 208, 1152, 0, False, False), 'gemm8/int8_scaled/stream8'),
    (Case('gemm8', 'int8_scaled', 17, 208, 1152, 0, True, False), 'gemm8/int8_scaled/stream8'),
    (Case('gemm8', 'int_mm', 1, 48, 4096, 0, False, True), 'gemm8/int_mm/dma128/128x128'),
    (Case('gemm8', 'int_mm', 1, 37888, 3584, 0, False, True), 'gemm8/int_mm/p8/256x256'),
    (Case('gemm8', 'int_mm', 257, 16400, 4096, 0, False, True), 'gemm8/int_mm/p8/256x256'),
    (Case('gemm8', 'int_mm', 513, 8192, 1024, 0, False, True), 'gemm8/int_mm/p8h/256x128'),
    (Case('gemm8', 'int_mm', 129, 16400, 4096, 0, False, True), 'gemm8/int_mm/p8h/256x128'),
    (Case('gemm8', 'int_mm', 257, 4096, 10240, 0, False, True), 'gemm8/int_mm/p8h/256x128/kparts'),
    (Case('gemm8', 'int_mm', 4096, 208, 13824, 0, False, True), 'gemm8/int_mm/p8h/256x128/kparts'),
    (Case('gemm8', 'int_mm', 2048, 1280, 8192, 0, False, True), 'gemm8/int_mm/p8h/256x128/kparts'),
    (Case('gemm8', 'int_mm', 1280, 8192, 1024, 0, False, True), 'gemm8/int_mm/p8p/256x256'),
    (Case('gemm8', 'int_mm', 1, 4112, 1040, 0, False, True), 'gemm8/int_mm/regstage/128x128'),
    (Case('int4', 'mm', 5, 37888, 3584, 128, False, True), 'int4/g128/rb/w4/nt1/mt1'),
    (Case('int4', 'mm', 9, 8192, 1024, 128, False, True), 'int4/g128/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 5, 16400, 4096, 128, False, True), 'int4/g128/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 9, 12288, 4096, 128, False, True), 'int4/g128/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 17, 37888, 3584, 128, False, True), 'int4/g128/rb/w4/nt1/mt2'),
    (Case('int4', 'mm', 17, 48, 4096, 128, False, True), 'int4/g128/rb/w4/nt1/mt2/kparts'),
    (Case('int4', 'mm', 17, 208, 1152, 128, False, True), 'int4/g128/rb/w4/nt1/mt2/kparts'),
    (Case('int4', 'mm', 33, 208, 1152, 128, False, True), 'int4/g128/rb/w4/nt1/mt4'),
    (Case('int4', 'mm', 33, 48, 4096, 128, False, True), 'int4/g128/rb/w4/nt1/mt4/kparts'),
    (Case('int4', 'mm', 33, 208, 13824, 128, False, True), 'int4/g128/rb/w4/nt1/mt4/kparts'),
    (Case('int4', 'mm', 65, 208, 1152, 128, False, True), 'int4/g128/rb/w4/nt1/mt8/prod'),
    (Case('int4', 'mm', 65, 48, 4096, 128, False, True), 'int4/g128/rb/w4/nt1/mt8/prod/kparts'),
    (Case('int4', 'mm', 65, 208, 13824, 128, False, True), 'int4/g128/rb/w4/nt1/mt8/prod/kparts'),
    (Case('int4', 'mm', 33, 28672, 4096, 128, False, True), 'int4/g128/rb/w8/nt1/mt4'),
    (Case('int4', 'mm', 1, 8192, 1024, 128, False, True), 'int4/g128/tile/r1/d2/straight'),
    (Case('int4', 'mm', 1, 208, 1152, 128, False, True), 'int4/g128/tile/r1/d4'),
    (Case('int4', 'mm', 1, 48, 4096, 128, False, True), 'int4/g128/tile/r1/d4/straight'),
    (Case('int4', 'mm', 1, 4096, 14336, 128, False, True), 'int4/g128/tile/r1/d7/straight'),
    (Case('int4', 'mm', 1, 48, 16384, 128, False, True), 'int4/g128/tile/r1/d8/straight'),
    (Case('int4', 'mm', 1, 208, 13824, 128, False, True), 'int4/g128/tile/r1/d9/straight'),
    (Case('int4', 'mm', 9, 48, 4096, 128, False, True), 'int4/g128/tile/r16/d4'),
    (Case('int4', 'mm', 2, 48, 4096, 128, False, True), 'int4/g128/tile/r4/d4'),
    (Case('int4', 'mm', 5, 48, 4096, 128, False, True), 'int4/g128/tile/r8/d4'),
    (Case('int4', 'mm', 257, 8192, 1024, 128, False, True), 'int4/g128/w32/cg1/prod'),
    (Case('int4', 'mm', 65, 16400, 4096, 128, False, True), 'int4/g128/w32/cg1/prod'),
    (Case('int4', 'mm', 129, 48, 4096, 128, False, True), 'int4/g128/w32/cg1/prod/kparts'),
    (Case('int4', 'mm', 129, 208, 1152, 128, False, True), 'int4/g128/w32/cg1/prod/kparts'),
    (Case('int4', 'mm', 513, 8192, 1024, 128, False, True), 'int4/g128/w32/cg2/prod'),
    (Case('int4', 'mm', 4096, 1040, 2560, 128, False, True), 'int4/g128/w32/cg2/prod'),
    (Case('int4', 'mm', 5, 37888, 3584, 256, False, True), 'int4/g256/rb/w4/nt1/mt1'),
    (Case('int4', 'mm', 9, 8192, 1024, 256, False, True), 'int4/g256/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 5, 16400, 4096, 256, False, True), 'int4/g256/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 9, 12288, 4096, 256, False, True), 'int4/g256/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 17, 37888, 3584, 256, False, True), 'int4/g256/rb/w4/nt1/mt2'),
    (Case('int4', 'mm', 17, 48, 4096, 256, False, True), 'int4/g256/rb/w4/nt1/mt2/kparts'),
    (Case('int4', 'mm', 17, 208, 13824, 256, False, True), 'int4/g256/rb/w4/nt1/mt2/kparts'),
    (Case('int4', 'mm', 33, 8192, 1024, 256, False, True), 'int4/g256/rb/w4/nt1/mt4'),
    (Case('int4', 'mm', 33, 16400, 4096, 256, False, True), 'int4/g256/rb/w4/nt1/mt4'),
    (Case('int4', 'mm', 33, 48, 4096, 256, False, True), 'int4/g256/rb/w4/nt1/mt4/kparts'),
    (Case('int4', 'mm', 33, 208, 13824, 256, False, True), 'int4/g256/rb/w4/nt1/mt4/kparts'),
    (Case('int4', 'mm', 65, 48, 4096, 256, False, True), 'int4/g256/rb/w4/nt1/mt8/prod/kparts'),
    (Case('int4', 'mm', 65, 208, 13824, 256, False, True), 'int4/g256/rb/w4/nt1/mt8/prod/kparts'),
    (Case('int4', 'mm', 33, 28672, 4096, 256, False, True), 'int4/g256/rb/w8/nt1/mt4'),
    (Case('int4', 'mm', 1, 8192, 1024, 256, False, True), 'int4/g256/tile/r1/d2/straight'),
    (Case('int4', 'mm', 1, 3584, 18944, 256, False, True), 'int4/g256/tile/r1/d4'),
    (Case('int4', 'mm', 1, 48, 4096, 256, False, True), 'int4/g256/tile/r1/d4/straight'),
    (Case('int4', 'mm', 1, 4096, 14336, 256, False, True), 'int4/g256/tile/r1/d7/straight'),
    (Case('int4', 'mm', 1, 48, 16384, 256, False, True), 'int4/g256/tile/r1/d8/straight'),
    (Case('int4', 'mm', 1, 208, 13824, 256, False, True), 'int4/g256/tile/r1/d9/straight'),
    (Case('int4', 'mm', 9, 48, 4096, 256, False, True), 'int4/g256/tile/r16/d4'),
    (Case('int4', 'mm', 2, 48, 4096, 256, False, True), 'int4/g256/tile/r4/d4'),
    (Case('int4', 'mm', 5, 48, 4096, 256, False, True), 'int4/g256/tile/r8/d4'),
    (Case('int4', 'mm', 257, 8192, 1024, 256, False, True), 'int4/g256/w32/cg1/prod'),
    (Case('int4', 'mm', 65, 16400, 4096, 256, False, True), 'int4/g256/w32/cg1/prod'),
    (Case('int4', 'mm', 129, 48, 4096, 256, False, True), 'int4/g256/w32/cg1/prod/kparts'),
    (Case('int4', 'mm', 129, 208, 13824, 256, False, True), 'int4/g256/w32/cg1/prod/kparts'),
    (Case('int4', 'mm', 513, 8192, 1024, 256, False, True), 'int4/g256/w32/cg2/prod'),
    (Case('int4', 'mm', 4096, 1040, 2560, 256, False, True), 'int4/g256/w32/cg2/prod'),
    (Case('int4', 'mm', 5, 37888, 3584, 32, False, True), 'int4/g32/rb/w4/nt1/mt1'),
    (Case('int4', 'mm', 9, 8192, 1024, 32, False, True), 'int4/g32/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 5, 16400, 4096, 32, False, True), 'int4/g32/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 9, 12288, 4096, 32, False, True), 'int4/g32/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 17, 37888, 3584, 32, False, True), 'int4/g32/rb/w4/nt1/mt2'),
    (Case('int4', 'mm', 17, 48, 4096, 32, False, True), 'int4/g32/rb/w4/nt1/mt2/kparts'),
    (Case('int4', 'mm', 17, 208, 1152, 32, False, True), 'int4/g32/rb/w4/nt1/mt2/kparts'),
    (Case('int4', 'mm', 33, 208, 1152, 32, False, True), 'int4/g32/rb/w4/nt1/mt4'),
    (Case('int4', 'mm', 33, 48, 4096, 32, False, True), 'int4/g32/rb/w4/nt1/mt4/kparts'),
    (Case('int4', 'mm', 33, 208, 13824, 32, False, True), 'int4/g32/rb/w4/nt1/mt4/kparts'),
    (Case('int4', 'mm', 65, 208, 1152, 32, False, True), 'int4/g32/rb/w4/nt1/mt8/prod'),
    (Case('int4', 'mm', 65, 48, 4096, 32, False, True), 'int4/g32/rb/w4/nt1/mt8/prod/kparts'),
    (Case('int4', 'mm', 65, 208, 13824, 32, False, True), 'int4/g32/rb/w4/nt1/mt8/prod/kparts'),
    (Case('int4', 'mm', 33, 28672, 4096, 32, False, True), 'int4/g32/rb/w8/nt1/mt4'),
    (Case('int4', 'mm', 1, 8192, 1024, 32, False, True), 'int4/g32/tile/r1/d2/straight'),
    (Case('int4', 'mm', 1, 208, 1152, 32, False, True), 'int4/g32/tile/r1/d4'),
    (Case('int4', 'mm', 1, 48, 4096, 32, False, True), 'int4/g32/tile/r1/d4/straight'),
    (Case('int4', 'mm', 1, 4096, 14336, 32, False, True), 'int4/g32/tile/r1/d7/straight'),
    (Case('int4', 'mm', 1, 48, 16384, 32, False, True), 'int4/g32/tile/r1/d8/straight'),
    (Case('int4', 'mm', 1, 208, 13824, 32, False, True), 'int4/g32/tile/r1/d9/straight'),
    (Case('int4', 'mm', 9, 48, 4096, 32, False, True), 'int4/g32/tile/r16/d4'),
    (Case('int4', 'mm', 2, 48, 4096, 32, False, True), 'int4/g32/tile/r4/d4'),
    (Case('int4', 'mm', 5, 48, 4096, 32, False, True), 'int4/g32/tile/r8/d4'),
    (Case('int4', 'mm', 257, 8192, 1024, 32, False, True), 'int4/g32/w32/cg1/prod'),
    (Case('int4', 'mm', 65, 16400, 4096, 32, False, True), 'int4/g32/w32/cg1/prod'),
    (Case('int4', 'mm', 129, 48, 4096, 32, False, True), 'int4/g32/w32/cg1/prod/kparts'),
    (Case('int4', 'mm', 129, 208, 1152, 32, False, True), 'int4/g32/w32/cg1/prod/kparts'),
    (Case('int4', 'mm', 5, 37888, 3584, 64, False, True), 'int4/g64/rb/w4/nt1/mt1'),
    (Case('int4', 'mm', 9, 8192, 1024, 64, False, True), 'int4/g64/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 5, 16400, 4096, 64, False, True), 'int4/g64/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 9, 12288, 4096, 64, False, True), 'int4/g64/rb/w4/nt1/mt1/kparts'),
    (Case('int4', 'mm', 17, 37888, 3584, 64, False, True), 'int4/g64/rb/w4/nt1/mt2'),
    (Case('int4', 'mm', 17, 48, 4096, 64, False, True), 'int4/g64/rb/w4/nt1/mt2/kparts'),
    (Case('int4', 'mm', 17, 208, 1152, 64, False, True), 'int4/g64/rb/w4/nt1/mt2/kparts'),
    (Case('int4', 'mm', 33, 208, 1152, 64, False, True), 'int4/g64/rb/w4/nt1/mt4'),
    (Case('int4', 'mm', 33, 48, 4096, 64, False, True), 'int4/g64/rb/w4/nt1/mt4/kparts'),
    (Case('int4', 'mm', 33, 208, 13824, 64, False, True), 'int4/g64/rb/w4/nt1/mt4/kparts'),
    (Case('int4', 'mm', 65, 208, 1152, 64, False, True), 'int4/g64/rb/w4/nt1/mt8/prod'),
    (Case('int4', 'mm', 65, 48, 4096, 64, False, True), 'int4/g64/rb/w4/nt1/mt8/prod/kparts'),
    (Case('int4', 'mm', 65, 208, 13824, 64, False, True), 'int4/g64/rb/w4/nt1/mt8/prod/kparts'),
    (Case('int4', 'mm', 33, 28672, 4096, 64, False, True), 'int4/g64/rb/w8/nt1/mt4'),
    (Case('int4', 'mm', 1, 8192, 1024, 64, False, True), 'int4/g64/tile/r1/d2/straight'),
    (Case('int4', 'mm', 1, 208, 1152, 64, False, True), 'int4/g64/tile/r1/d4'),
    (Case('int4', 'mm', 1, 48, 4096, 64, False, True), 'int4/g64/tile/r1/d4/straight'),
    (Case('int4', 'mm', 1, 4096, 14336, 64, False, True), 'int4/g64/tile/r1/d7/straight'),
    (Case('int4', 'mm', 1, 48, 16384, 64, False, True), 'int4/g64/tile/r1/d8/straight'),
    (Case('int4', 'mm', 1, 208, 13824, 64, False, True), 'int4/g64/tile/r1/d9/straight'),
    (Case('int4', 'mm', 9, 48, 4096, 64, False, True), 'int4/g64/tile/r16/d4'),
    (Case('int4', 'mm', 2, 48, 4096, 64, False, True), 'int4/g64/tile/r4/d4'),
    (Case('int4', 'mm', 5, 48, 4096, 64, False, True), 'int4/g64/tile/r8/d4'),
    (Case('int4', 'mm', 257, 8192, 1024, 64, False, True), 'int4/g64/w32/cg1/prod'),
    (Case('int4', 'mm', 65, 16400, 4096, 64, False, True), 'int4/g64/w32/cg1/prod'),
    (Case('int4', 'mm', 129, 48, 4096, 64, False, True), 'int4/g64/w32/cg1/prod/kparts'),
    (Case('int4', 'mm', 129, 208, 1152, 64, False, True), 'int4/g64/w32/cg1/prod/kparts'),
    (Case('mx', 'e2m1_codes', 1, 16, 32, 0, False, True), 'mx/e2m1_codes/stream/w1/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 32, 0, True, True), 'mx/e2m1_codes/stream/w1/mt1'),
    (Case('mx', 'e2m1_codes', 1, 17, 32, 0, False, True), 'mx/e2m1_codes/stream/w1/mt1'),
    (Case('mx', 'e2m1_codes', 1, 17, 32, 0, True, True), 'mx/e2m1_codes/stream/w1/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 32, 0, False, False), 'mx/e2m1_codes/stream/w1/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 32, 0, True, False), 'mx/e2m1_codes/stream/w1/mt1'),
    (Case('mx', 'e2m1_codes', 17, 16, 32, 0, False, True), 'mx/e2m1_codes/stream/w1/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16, 32, 0, True, True), 'mx/e2m1_codes/stream/w1/mt2'),
    (Case('mx', 'e2m1_codes', 17, 17, 32, 0, False, True), 'mx/e2m1_codes/stream/w1/mt2'),
    (Case('mx', 'e2m1_codes', 17, 17, 32, 0, True, True), 'mx/e2m1_codes/stream/w1/mt2'),
    (Case('mx', 'e2m1_codes', 1, 16, 4096, 0, False, True), 'mx/e2m1_codes/stream/w16/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 4096, 0, True, True), 'mx/e2m1_codes/stream/w16/mt1'),
    (Case('mx', 'e2m1_codes', 1, 17, 4096, 0, False, True), 'mx/e2m1_codes/stream/w16/mt1'),
    (Case('mx', 'e2m1_codes', 1, 17, 4096, 0, True, True), 'mx/e2m1_codes/stream/w16/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 4160, 0, False, True), 'mx/e2m1_codes/stream/w16/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 4160, 0, True, True), 'mx/e2m1_codes/stream/w16/mt1'),
    (Case('mx', 'e2m1_codes', 17, 16, 4096, 0, False, True), 'mx/e2m1_codes/stream/w16/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16, 4096, 0, True, True), 'mx/e2m1_codes/stream/w16/mt2'),
    (Case('mx', 'e2m1_codes', 17, 17, 4096, 0, False, True), 'mx/e2m1_codes/stream/w16/mt2'),
    (Case('mx', 'e2m1_codes', 17, 17, 4096, 0, True, True), 'mx/e2m1_codes/stream/w16/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16, 4160, 0, False, True), 'mx/e2m1_codes/stream/w16/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16, 4160, 0, True, True), 'mx/e2m1_codes/stream/w16/mt2'),
    (Case('mx', 'e2m1_codes', 1, 16, 160, 0, False, True), 'mx/e2m1_codes/stream/w2/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 160, 0, True, True), 'mx/e2m1_codes/stream/w2/mt1'),
    (Case('mx', 'e2m1_codes', 1, 17, 160, 0, False, True), 'mx/e2m1_codes/stream/w2/mt1'),
    (Case('mx', 'e2m1_codes', 1, 17, 160, 0, True, True), 'mx/e2m1_codes/stream/w2/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 384, 0, False, True), 'mx/e2m1_codes/stream/w2/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 384, 0, True, True), 'mx/e2m1_codes/stream/w2/mt1'),
    (Case('mx', 'e2m1_codes', 17, 16, 160, 0, False, True), 'mx/e2m1_codes/stream/w2/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16, 160, 0, True, True), 'mx/e2m1_codes/stream/w2/mt2'),
    (Case('mx', 'e2m1_codes', 17, 17, 160, 0, False, True), 'mx/e2m1_codes/stream/w2/mt2'),
    (Case('mx', 'e2m1_codes', 17, 17, 160, 0, True, True), 'mx/e2m1_codes/stream/w2/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16, 384, 0, False, True), 'mx/e2m1_codes/stream/w2/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16, 384, 0, True, True), 'mx/e2m1_codes/stream/w2/mt2'),
    (Case('mx', 'e2m1_codes', 1, 16384, 1024, 0, False, True), 'mx/e2m1_codes/stream/w4/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16384, 1024, 0, True, True), 'mx/e2m1_codes/stream/w4/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16384, 4160, 0, False, True), 'mx/e2m1_codes/stream/w4/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16384, 4160, 0, True, True), 'mx/e2m1_codes/stream/w4/mt1'),
    (Case('mx', 'e2m1_codes', 17, 16384, 1024, 0, False, True), 'mx/e2m1_codes/stream/w4/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16384, 1024, 0, True, True), 'mx/e2m1_codes/stream/w4/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16384, 4160, 0, False, True), 'mx/e2m1_codes/stream/w4/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16384, 4160, 0, True, True), 'mx/e2m1_codes/stream/w4/mt2'),
    (Case('mx', 'e2m1_codes', 1, 16, 1024, 0, False, True), 'mx/e2m1_codes/stream/w8/mt1'),
    (Case('mx', 'e2m1_codes', 1, 16, 1024, 0, True, True), 'mx/e2m1_codes/stream/w8/mt1'),
    (Case('mx', 'e2m1_codes', 1, 17, 1024, 0, False, True), 'mx/e2m1_codes/stream/w8/mt1'),
    (Case('mx', 'e2m1_codes', 1, 17, 1024, 0, True, True), 'mx/e2m1_codes/stream/w8/mt1'),
    (Case('mx', 'e2m1_codes', 1, 4096, 4160, 0, False, True), 'mx/e2m1_codes/stream/w8/mt1'),
    (Case('mx', 'e2m1_codes', 1, 4096, 4160, 0, True, True), 'mx/e2m1_codes/stream/w8/mt1'),
    (Case('mx', 'e2m1_codes', 17, 16, 1024, 0, False, True), 'mx/e2m1_codes/stream/w8/mt2'),
    (Case('mx', 'e2m1_codes', 17, 16, 1024, 0, True, True), 'mx/e2m1_codes/stream/w8/mt2'),
    (Case('mx', 'e2m1_codes', 17, 17, 1024, 0, False, True), 'mx/e2m1_codes/stream/w8/mt2'),
    (Case('mx', 'e2m1_codes', 17, 17, 1024, 0, True, True), 'mx/e2m1_codes/stream/w8/mt2'),
    (Case('mx', 'e2m1_codes', 17, 4096, 4160, 0, False, True), 'mx/e2m1_codes/stream/w8/mt2'),
    (Case('mx', 'e2m1_codes', 17, 4096, 4160, 0, True, True), 'mx/e2m1_codes/stream/w8/mt2'),
    (Case('mx', 'e2m1_codes', 33, 16, 32, 0, False, True), 'mx/e2m1_codes/tile/w4/mt4'),
    (Case('mx', 'e2m1_codes', 33, 16, 32, 0, True, True), 'mx/e2m1_codes/tile/w4/mt4'),
    (Case('mx', 'e2m1_codes', 33, 257, 32, 0, False, True), 'mx/e2m1_codes/tile/w4/mt4'),
    (Case('mx', 'e2m1_codes', 33, 257, 32, 0, True, True), 'mx/e2m1_codes/tile/w4/mt4'),
    (Case('mx', 'e2m1_codes', 33, 16, 32, 0, False, False), 'mx/e2m1_codes/tile/w4/mt4'),
    (Case('mx', 'e2m1_codes', 33, 16, 32, 0, True, False), 'mx/e2m1_codes/tile/w4/mt4'),
    (Case('mx', 'e2m1_fused', 1, 16, 32, 0, False, True), 'mx/e2m1_fused/stream/w1/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 32, 0, True, True), 'mx/e2m1_fused/stream/w1/mt1'),
    (Case('mx', 'e2m1_fused', 1, 17, 32, 0, False, True), 'mx/e2m1_fused/stream/w1/mt1'),
    (Case('mx', 'e2m1_fused', 1, 17, 32, 0, True, True), 'mx/e2m1_fused/stream/w1/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 32, 0, False, False), 'mx/e2m1_fused/stream/w1/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 32, 0, True, False), 'mx/e2m1_fused/stream/w1/mt1'),
    (Case('mx', 'e2m1_fused', 17, 16, 32, 0, False, True), 'mx/e2m1_fused/stream/w1/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16, 32, 0, True, True), 'mx/e2m1_fused/stream/w1/mt2'),
    (Case('mx', 'e2m1_fused', 17, 17, 32, 0, False, True), 'mx/e2m1_fused/stream/w1/mt2'),
    (Case('mx', 'e2m1_fused', 17, 17, 32, 0, True, True), 'mx/e2m1_fused/stream/w1/mt2'),
    (Case('mx', 'e2m1_fused', 1, 16, 4096, 0, False, True), 'mx/e2m1_fused/stream/w16/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 4096, 0, True, True), 'mx/e2m1_fused/stream/w16/mt1'),
    (Case('mx', 'e2m1_fused', 1, 17, 4096, 0, False, True), 'mx/e2m1_fused/stream/w16/mt1'),
    (Case('mx', 'e2m1_fused', 1, 17, 4096, 0, True, True), 'mx/e2m1_fused/stream/w16/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 4160, 0, False, True), 'mx/e2m1_fused/stream/w16/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 4160, 0, True, True), 'mx/e2m1_fused/stream/w16/mt1'),
    (Case('mx', 'e2m1_fused', 17, 16, 4096, 0, False, True), 'mx/e2m1_fused/stream/w16/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16, 4096, 0, True, True), 'mx/e2m1_fused/stream/w16/mt2'),
    (Case('mx', 'e2m1_fused', 17, 17, 4096, 0, False, True), 'mx/e2m1_fused/stream/w16/mt2'),
    (Case('mx', 'e2m1_fused', 17, 17, 4096, 0, True, True), 'mx/e2m1_fused/stream/w16/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16, 4160, 0, False, True), 'mx/e2m1_fused/stream/w16/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16, 4160, 0, True, True), 'mx/e2m1_fused/stream/w16/mt2'),
    (Case('mx', 'e2m1_fused', 1, 16, 160, 0, False, True), 'mx/e2m1_fused/stream/w2/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 160, 0, True, True), 'mx/e2m1_fused/stream/w2/mt1'),
    (Case('mx', 'e2m1_fused', 1, 17, 160, 0, False, True), 'mx/e2m1_fused/stream/w2/mt1'),
    (Case('mx', 'e2m1_fused', 1, 17, 160, 0, True, True), 'mx/e2m1_fused/stream/w2/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 384, 0, False, True), 'mx/e2m1_fused/stream/w2/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 384, 0, True, True), 'mx/e2m1_fused/stream/w2/mt1'),
    (Case('mx', 'e2m1_fused', 17, 16, 160, 0, False, True), 'mx/e2m1_fused/stream/w2/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16, 160, 0, True, True), 'mx/e2m1_fused/stream/w2/mt2'),
    (Case('mx', 'e2m1_fused', 17, 17, 160, 0, False, True), 'mx/e2m1_fused/stream/w2/mt2'),
    (Case('mx', 'e2m1_fused', 17, 17, 160, 0, True, True), 'mx/e2m1_fused/stream/w2/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16, 384, 0, False, True), 'mx/e2m1_fused/stream/w2/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16, 384, 0, True, True), 'mx/e2m1_fused/stream/w2/mt2'),
    (Case('mx', 'e2m1_fused', 1, 16384, 1024, 0, False, True), 'mx/e2m1_fused/stream/w4/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16384, 1024, 0, True, True), 'mx/e2m1_fused/stream/w4/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16384, 4160, 0, False, True), 'mx/e2m1_fused/stream/w4/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16384, 4160, 0, True, True), 'mx/e2m1_fused/stream/w4/mt1'),
    (Case('mx', 'e2m1_fused', 17, 16384, 1024, 0, False, True), 'mx/e2m1_fused/stream/w4/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16384, 1024, 0, True, True), 'mx/e2m1_fused/stream/w4/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16384, 4160, 0, False, True), 'mx/e2m1_fused/stream/w4/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16384, 4160, 0, True, True), 'mx/e2m1_fused/stream/w4/mt2'),
    (Case('mx', 'e2m1_fused', 1, 16, 1024, 0, False, True), 'mx/e2m1_fused/stream/w8/mt1'),
    (Case('mx', 'e2m1_fused', 1, 16, 1024, 0, True, True), 'mx/e2m1_fused/stream/w8/mt1'),
    (Case('mx', 'e2m1_fused', 1, 17, 1024, 0, False, True), 'mx/e2m1_fused/stream/w8/mt1'),
    (Case('mx', 'e2m1_fused', 1, 17, 1024, 0, True, True), 'mx/e2m1_fused/stream/w8/mt1'),
    (Case('mx', 'e2m1_fused', 1, 4096, 4160, 0, False, True), 'mx/e2m1_fused/stream/w8/mt1'),
    (Case('mx', 'e2m1_fused', 1, 4096, 4160, 0, True, True), 'mx/e2m1_fused/stream/w8/mt1'),
    (Case('mx', 'e2m1_fused', 17, 16, 1024, 0, False, True), 'mx/e2m1_fused/stream/w8/mt2'),
    (Case('mx', 'e2m1_fused', 17, 16, 1024, 0, True, True), 'mx/e2m1_fused/stream/w8/mt2'),
    (Case('mx', 'e2m1_fused', 17, 17, 1024, 0, False, True), 'mx/e2m1_fused/stream/w8/mt2'),
    (Case('mx', 'e2m1_fused', 17, 17, 1024, 0, True, True), 'mx/e2m1_fused/stream/w8/mt2'),
    (Case('mx', 'e2m1_fused', 17, 4096, 4160, 0, False, True), 'mx/e2m1_fused/stream/w8/mt2'),
    (Case('mx', 'e2m1_fused', 17, 4096, 4160, 0, True, True), 'mx/e2m1_fused/stream/w8/mt2'),
    (Case('mx', 'e4m3_codes', 1, 16, 32, 0, False, True), 'mx/e4m3_codes/stream/w1/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 32, 0, True, True), 'mx/e4m3_codes/stream/w1/mt1'),
    (Case('mx', 'e4m3_codes', 1, 17, 32, 0, False, True), 'mx/e4m3_codes/stream/w1/mt1'),
    (Case('mx', 'e4m3_codes', 1, 17, 32, 0, True, True), 'mx/e4m3_codes/stream/w1/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 32, 0, False, False), 'mx/e4m3_codes/stream/w1/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 32, 0, True, False), 'mx/e4m3_codes/stream/w1/mt1'),
    (Case('mx', 'e4m3_codes', 17, 16, 32, 0, False, True), 'mx/e4m3_codes/stream/w1/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16, 32, 0, True, True), 'mx/e4m3_codes/stream/w1/mt2'),
    (Case('mx', 'e4m3_codes', 17, 17, 32, 0, False, True), 'mx/e4m3_codes/stream/w1/mt2'),
    (Case('mx', 'e4m3_codes', 17, 17, 32, 0, True, True), 'mx/e4m3_codes/stream/w1/mt2'),
    (Case('mx', 'e4m3_codes', 33, 16, 32, 0, False, True), 'mx/e4m3_codes/stream/w1/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16, 32, 0, True, True), 'mx/e4m3_codes/stream/w1/mt4'),
    (Case('mx', 'e4m3_codes', 33, 17, 32, 0, False, True), 'mx/e4m3_codes/stream/w1/mt4'),
    (Case('mx', 'e4m3_codes', 33, 17, 32, 0, True, True), 'mx/e4m3_codes/stream/w1/mt4'),
    (Case('mx', 'e4m3_codes', 1, 16, 4096, 0, False, True), 'mx/e4m3_codes/stream/w16/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 4096, 0, True, True), 'mx/e4m3_codes/stream/w16/mt1'),
    (Case('mx', 'e4m3_codes', 1, 17, 4096, 0, False, True), 'mx/e4m3_codes/stream/w16/mt1'),
    (Case('mx', 'e4m3_codes', 1, 17, 4096, 0, True, True), 'mx/e4m3_codes/stream/w16/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 4160, 0, False, True), 'mx/e4m3_codes/stream/w16/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 4160, 0, True, True), 'mx/e4m3_codes/stream/w16/mt1'),
    (Case('mx', 'e4m3_codes', 17, 16, 4096, 0, False, True), 'mx/e4m3_codes/stream/w16/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16, 4096, 0, True, True), 'mx/e4m3_codes/stream/w16/mt2'),
    (Case('mx', 'e4m3_codes', 17, 17, 4096, 0, False, True), 'mx/e4m3_codes/stream/w16/mt2'),
    (Case('mx', 'e4m3_codes', 17, 17, 4096, 0, True, True), 'mx/e4m3_codes/stream/w16/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16, 4160, 0, False, True), 'mx/e4m3_codes/stream/w16/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16, 4160, 0, True, True), 'mx/e4m3_codes/stream/w16/mt2'),
    (Case('mx', 'e4m3_codes', 1, 16, 160, 0, False, True), 'mx/e4m3_codes/stream/w2/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 160, 0, True, True), 'mx/e4m3_codes/stream/w2/mt1'),
    (Case('mx', 'e4m3_codes', 1, 17, 160, 0, False, True), 'mx/e4m3_codes/stream/w2/mt1'),
    (Case('mx', 'e4m3_codes', 1, 17, 160, 0, True, True), 'mx/e4m3_codes/stream/w2/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 384, 0, False, True), 'mx/e4m3_codes/stream/w2/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 384, 0, True, True), 'mx/e4m3_codes/stream/w2/mt1'),
    (Case('mx', 'e4m3_codes', 17, 16, 160, 0, False, True), 'mx/e4m3_codes/stream/w2/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16, 160, 0, True, True), 'mx/e4m3_codes/stream/w2/mt2'),
    (Case('mx', 'e4m3_codes', 17, 17, 160, 0, False, True), 'mx/e4m3_codes/stream/w2/mt2'),
    (Case('mx', 'e4m3_codes', 17, 17, 160, 0, True, True), 'mx/e4m3_codes/stream/w2/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16, 384, 0, False, True), 'mx/e4m3_codes/stream/w2/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16, 384, 0, True, True), 'mx/e4m3_codes/stream/w2/mt2'),
    (Case('mx', 'e4m3_codes', 33, 16, 160, 0, False, True), 'mx/e4m3_codes/stream/w2/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16, 160, 0, True, True), 'mx/e4m3_codes/stream/w2/mt4'),
    (Case('mx', 'e4m3_codes', 33, 17, 160, 0, False, True), 'mx/e4m3_codes/stream/w2/mt4'),
    (Case('mx', 'e4m3_codes', 33, 17, 160, 0, True, True), 'mx/e4m3_codes/stream/w2/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16, 384, 0, False, True), 'mx/e4m3_codes/stream/w2/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16, 384, 0, True, True), 'mx/e4m3_codes/stream/w2/mt4'),
    (Case('mx', 'e4m3_codes', 1, 16384, 1024, 0, False, True), 'mx/e4m3_codes/stream/w4/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16384, 1024, 0, True, True), 'mx/e4m3_codes/stream/w4/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16384, 4160, 0, False, True), 'mx/e4m3_codes/stream/w4/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16384, 4160, 0, True, True), 'mx/e4m3_codes/stream/w4/mt1'),
    (Case('mx', 'e4m3_codes', 17, 16384, 1024, 0, False, True), 'mx/e4m3_codes/stream/w4/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16384, 1024, 0, True, True), 'mx/e4m3_codes/stream/w4/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16384, 4160, 0, False, True), 'mx/e4m3_codes/stream/w4/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16384, 4160, 0, True, True), 'mx/e4m3_codes/stream/w4/mt2'),
    (Case('mx', 'e4m3_codes', 33, 16384, 1024, 0, False, True), 'mx/e4m3_codes/stream/w4/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16384, 1024, 0, True, True), 'mx/e4m3_codes/stream/w4/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16384, 4160, 0, False, True), 'mx/e4m3_codes/stream/w4/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16384, 4160, 0, True, True), 'mx/e4m3_codes/stream/w4/mt4'),
    (Case('mx', 'e4m3_codes', 1, 16, 1024, 0, False, True), 'mx/e4m3_codes/stream/w8/mt1'),
    (Case('mx', 'e4m3_codes', 1, 16, 1024, 0, True, True), 'mx/e4m3_codes/stream/w8/mt1'),
    (Case('mx', 'e4m3_codes', 1, 17, 1024, 0, False, True), 'mx/e4m3_codes/stream/w8/mt1'),
    (Case('mx', 'e4m3_codes', 1, 17, 1024, 0, True, True), 'mx/e4m3_codes/stream/w8/mt1'),
    (Case('mx', 'e4m3_codes', 1, 4096, 4160, 0, False, True), 'mx/e4m3_codes/stream/w8/mt1'),
    (Case('mx', 'e4m3_codes', 1, 4096, 4160, 0, True, True), 'mx/e4m3_codes/stream/w8/mt1'),
    (Case('mx', 'e4m3_codes', 17, 16, 1024, 0, False, True), 'mx/e4m3_codes/stream/w8/mt2'),
    (Case('mx', 'e4m3_codes', 17, 16, 1024, 0, True, True), 'mx/e4m3_codes/stream/w8/mt2'),
    (Case('mx', 'e4m3_codes', 17, 17, 1024, 0, False, True), 'mx/e4m3_codes/stream/w8/mt2'),
    (Case('mx', 'e4m3_codes', 17, 17, 1024, 0, True, True), 'mx/e4m3_codes/stream/w8/mt2'),
    (Case('mx', 'e4m3_codes', 17, 4096, 4160, 0, False, True), 'mx/e4m3_codes/stream/w8/mt2'),
    (Case('mx', 'e4m3_codes', 17, 4096, 4160, 0, True, True), 'mx/e4m3_codes/stream/w8/mt2'),
    (Case('mx', 'e4m3_codes', 33, 16, 1024, 0, False, True), 'mx/e4m3_codes/stream/w8/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16, 1024, 0, True, True), 'mx/e4m3_codes/stream/w8/mt4'),
    (Case('mx', 'e4m3_codes', 33, 17, 1024, 0, False, True), 'mx/e4m3_codes/stream/w8/mt4'),
    (Case('mx', 'e4m3_codes', 33, 17, 1024, 0, True, True), 'mx/e4m3_codes/stream/w8/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16, 4160, 0, False, True), 'mx/e4m3_codes/stream/w8/mt4'),
    (Case('mx', 'e4m3_codes', 33, 16, 4160, 0, True, True), 'mx/e4m3_codes/stream/w8/mt4'),
    (Case('mx', 'e4m3_codes', 65, 16, 32, 0, False, True), 'mx/e4m3_codes/tile/w4/mt4'),
    (Case('mx', 'e4m3_codes', 65, 16, 32, 0, True, True), 'mx/e4m3_codes/tile/w4/mt4'),
    (Case('mx', 'e4m3_codes', 65, 257, 32, 0, False, True), 'mx/e4m3_codes/tile/w4/mt4'),
    (Case('mx', 'e4m3_codes', 65, 257, 32, 0, True, True), 'mx/e4m3_codes/tile/w4/mt4'),
    (Case('mx', 'e4m3_codes', 65, 16, 32, 0, False, False), 'mx/e4m3_codes/tile/w4/mt4'),
    (Case('mx', 'e4m3_codes', 65, 16, 32, 0, True, False), 'mx/e4m3_codes/tile/w4/mt4'),
    (Case('mx', 'e4m3_fused', 1, 16, 32, 0, False, True), 'mx/e4m3_fused/stream/w1/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 32, 0, True, True), 'mx/e4m3_fused/stream/w1/mt1'),
    (Case('mx', 'e4m3_fused', 1, 17, 32, 0, False, True), 'mx/e4m3_fused/stream/w1/mt1'),
    (Case('mx', 'e4m3_fused', 1, 17, 32, 0, True, True), 'mx/e4m3_fused/stream/w1/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 32, 0, False, False), 'mx/e4m3_fused/stream/w1/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 32, 0, True, False), 'mx/e4m3_fused/stream/w1/mt1'),
    (Case('mx', 'e4m3_fused', 17, 16, 32, 0, False, True), 'mx/e4m3_fused/stream/w1/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16, 32, 0, True, True), 'mx/e4m3_fused/stream/w1/mt2'),
    (Case('mx', 'e4m3_fused', 17, 17, 32, 0, False, True), 'mx/e4m3_fused/stream/w1/mt2'),
    (Case('mx', 'e4m3_fused', 17, 17, 32, 0, True, True), 'mx/e4m3_fused/stream/w1/mt2'),
    (Case('mx', 'e4m3_fused', 33, 16, 32, 0, False, True), 'mx/e4m3_fused/stream/w1/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16, 32, 0, True, True), 'mx/e4m3_fused/stream/w1/mt4'),
    (Case('mx', 'e4m3_fused', 33, 17, 32, 0, False, True), 'mx/e4m3_fused/stream/w1/mt4'),
    (Case('mx', 'e4m3_fused', 33, 17, 32, 0, True, True), 'mx/e4m3_fused/stream/w1/mt4'),
    (Case('mx', 'e4m3_fused', 1, 16, 4096, 0, False, True), 'mx/e4m3_fused/stream/w16/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 4096, 0, True, True), 'mx/e4m3_fused/stream/w16/mt1'),
    (Case('mx', 'e4m3_fused', 1, 17, 4096, 0, False, True), 'mx/e4m3_fused/stream/w16/mt1'),
    (Case('mx', 'e4m3_fused', 1, 17, 4096, 0, True, True), 'mx/e4m3_fused/stream/w16/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 4160, 0, False, True), 'mx/e4m3_fused/stream/w16/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 4160, 0, True, True), 'mx/e4m3_fused/stream/w16/mt1'),
    (Case('mx', 'e4m3_fused', 17, 16, 4096, 0, False, True), 'mx/e4m3_fused/stream/w16/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16, 4096, 0, True, True), 'mx/e4m3_fused/stream/w16/mt2'),
    (Case('mx', 'e4m3_fused', 17, 17, 4096, 0, False, True), 'mx/e4m3_fused/stream/w16/mt2'),
    (Case('mx', 'e4m3_fused', 17, 17, 4096, 0, True, True), 'mx/e4m3_fused/stream/w16/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16, 4160, 0, False, True), 'mx/e4m3_fused/stream/w16/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16, 4160, 0, True, True), 'mx/e4m3_fused/stream/w16/mt2'),
    (Case('mx', 'e4m3_fused', 1, 16, 160, 0, False, True), 'mx/e4m3_fused/stream/w2/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 160, 0, True, True), 'mx/e4m3_fused/stream/w2/mt1'),
    (Case('mx', 'e4m3_fused', 1, 17, 160, 0, False, True), 'mx/e4m3_fused/stream/w2/mt1'),
    (Case('mx', 'e4m3_fused', 1, 17, 160, 0, True, True), 'mx/e4m3_fused/stream/w2/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 384, 0, False, True), 'mx/e4m3_fused/stream/w2/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 384, 0, True, True), 'mx/e4m3_fused/stream/w2/mt1'),
    (Case('mx', 'e4m3_fused', 17, 16, 160, 0, False, True), 'mx/e4m3_fused/stream/w2/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16, 160, 0, True, True), 'mx/e4m3_fused/stream/w2/mt2'),
    (Case('mx', 'e4m3_fused', 17, 17, 160, 0, False, True), 'mx/e4m3_fused/stream/w2/mt2'),
    (Case('mx', 'e4m3_fused', 17, 17, 160, 0, True, True), 'mx/e4m3_fused/stream/w2/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16, 384, 0, False, True), 'mx/e4m3_fused/stream/w2/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16, 384, 0, True, True), 'mx/e4m3_fused/stream/w2/mt2'),
    (Case('mx', 'e4m3_fused', 33, 16, 160, 0, False, True), 'mx/e4m3_fused/stream/w2/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16, 160, 0, True, True), 'mx/e4m3_fused/stream/w2/mt4'),
    (Case('mx', 'e4m3_fused', 33, 17, 160, 0, False, True), 'mx/e4m3_fused/stream/w2/mt4'),
    (Case('mx', 'e4m3_fused', 33, 17, 160, 0, True, True), 'mx/e4m3_fused/stream/w2/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16, 384, 0, False, True), 'mx/e4m3_fused/stream/w2/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16, 384, 0, True, True), 'mx/e4m3_fused/stream/w2/mt4'),
    (Case('mx', 'e4m3_fused', 1, 16384, 1024, 0, False, True), 'mx/e4m3_fused/stream/w4/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16384, 1024, 0, True, True), 'mx/e4m3_fused/stream/w4/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16384, 4160, 0, False, True), 'mx/e4m3_fused/stream/w4/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16384, 4160, 0, True, True), 'mx/e4m3_fused/stream/w4/mt1'),
    (Case('mx', 'e4m3_fused', 17, 16384, 1024, 0, False, True), 'mx/e4m3_fused/stream/w4/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16384, 1024, 0, True, True), 'mx/e4m3_fused/stream/w4/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16384, 4160, 0, False, True), 'mx/e4m3_fused/stream/w4/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16384, 4160, 0, True, True), 'mx/e4m3_fused/stream/w4/mt2'),
    (Case('mx', 'e4m3_fused', 33, 16384, 1024, 0, False, True), 'mx/e4m3_fused/stream/w4/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16384, 1024, 0, True, True), 'mx/e4m3_fused/stream/w4/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16384, 4160, 0, False, True), 'mx/e4m3_fused/stream/w4/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16384, 4160, 0, True, True), 'mx/e4m3_fused/stream/w4/mt4'),
    (Case('mx', 'e4m3_fused', 1, 16, 1024, 0, False, True), 'mx/e4m3_fused/stream/w8/mt1'),
    (Case('mx', 'e4m3_fused', 1, 16, 1024, 0, True, True), 'mx/e4m3_fused/stream/w8/mt1'),
    (Case('mx', 'e4m3_fused', 1, 17, 1024, 0, False, True), 'mx/e4m3_fused/stream/w8/mt1'),
    (Case('mx', 'e4m3_fused', 1, 17, 1024, 0, True, True), 'mx/e4m3_fused/stream/w8/mt1'),
    (Case('mx', 'e4m3_fused', 1, 4096, 4160, 0, False, True), 'mx/e4m3_fused/stream/w8/mt1'),
    (Case('mx', 'e4m3_fused', 1, 4096, 4160, 0, True, True), 'mx/e4m3_fused/stream/w8/mt1'),
    (Case('mx', 'e4m3_fused', 17, 16, 1024, 0, False, True), 'mx/e4m3_fused/stream/w8/mt2'),
    (Case('mx', 'e4m3_fused', 17, 16, 1024, 0, True, True), 'mx/e4m3_fused/stream/w8/mt2'),
    (Case('mx', 'e4m3_fused', 17, 17, 1024, 0, False, True), 'mx/e4m3_fused/stream/w8/mt2'),
    (Case('mx', 'e4m3_fused', 17, 17, 1024, 0, True, True), 'mx/e4m3_fused/stream/w8/mt2'),
    (Case('mx', 'e4m3_fused', 17, 4096, 4160, 0, False, True), 'mx/e4m3_fused/stream/w8/mt2'),
    (Case('mx', 'e4m3_fused', 17, 4096, 4160, 0, True, True), 'mx/e4m3_fused/stream/w8/mt2'),
    (Case('mx', 'e4m3_fused', 33, 16, 1024, 0, False, True), 'mx/e4m3_fused/stream/w8/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16, 1024, 0, True, True), 'mx/e4m3_fused/stream/w8/mt4'),
    (Case('mx', 'e4m3_fused', 33, 17, 1024, 0, False, True), 'mx/e4m3_fused/stream/w8/mt4'),
    (Case('mx', 'e4m3_fused', 33, 17, 1024, 0, True, True), 'mx/e4m3_fused/stream/w8/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16, 4160, 0, False, True), 'mx/e4m3_fused/stream/w8/mt4'),
    (Case('mx', 'e4m3_fused', 33, 16, 4160, 0, True, True), 'mx/e4m3_fused/stream/w8/mt4'),
]

# signature -> cells of the grid that reach it: a moved band constant changes these counts
REACH = {
    'fp8_int4/dyn_asym/g128/fused_priv': 28,
    'fp8_int4/dyn_asym/g128/fused_wg': 285,
    'fp8_int4/dyn_asym/g256/fused_priv': 27,
    'fp8_int4/dyn_asym/g256/fused_wg': 270,
    'fp8_int4/dyn_asym/g32/fused_priv': 28,
    'fp8_int4/dyn_asym/g32/fused_wg': 285,
    'fp8_int4/dyn_asym/g64/fused_priv': 28,
    'fp8_int4/dyn_asym/g64/fused_wg': 285,
    'fp8_int4/dyn_sym/g128/fused_priv': 28,
    'fp8_int4/dyn_sym/g128/fused_wg': 285,
    'fp8_int4/dyn_sym/g256/fused_priv': 27,
    'fp8_int4/dyn_sym/g256/fused_wg': 270,
    'fp8_int4/dyn_sym/g32/fused_priv': 28,
    'fp8_int4/dyn_sym/g32/fused_wg': 285,
    'fp8_int4/dyn_sym/g64/fused_priv': 28,
    'fp8_int4/dyn_sym/g64/fused_wg': 285,
    'fp8_int4/linear_asym/g128/<1x1>': 464,
    'fp8_int4/linear_asym/g128/<2x1>': 330,
    'fp8_int4/linear_asym/g128/<2x2>': 569,
    'fp8_int4/linear_asym/g256/<1x1>': 448,
    'fp8_int4/linear_asym/g256/<2x1>': 299,
    'fp8_int4/linear_asym/g256/<2x2>': 569,
    'fp8_int4/linear_asym/g32/<1x1>': 464,
    'fp8_int4/linear_asym/g32/<2x1>': 899,
    'fp8_int4/linear_asym/g64/<1x1>': 464,
    'fp8_int4/linear_asym/g64/<2x1>': 899,
    'fp8_int4/linear_sym/g128/<1x1>': 464,
    'fp8_int4/linear_sym/g128/<2x1>': 330,
    'fp8_int4/linear_sym/g128/<2x2>': 569,
    'fp8_int4/linear_sym/g256/<1x1>': 448,
    'fp8_int4/linear_sym/g256/<2x1>': 299,
    'fp8_int4/linear_sym/g256/<2x2>': 569,
    'fp8_int4/linear_sym/g32/<1x1>': 464,
    'fp8_int4/linear_sym/g32/<2x1>': 899,
    'fp8_int4/linear_sym/g64/<1x1>': 464,
    'fp8_int4/linear_sym/g64/<2x1>': 899,
    'gemm8/fp8_dyn/dec8/w1/d8': 4,
    'gemm8/fp8_dyn/dec8/w10/d2/rows8': 8,
    'gemm8/fp8_dyn/dec8/w10/d4': 13,
    'gemm8/fp8_dyn/dec8/w10/d8': 6,
    'gemm8/fp8_dyn/dec8/w12/d8': 5,
    'gemm8/fp8_dyn/dec8/w14/d2': 9,
    'gemm8/fp8_dyn/dec8/w14/d8': 4,
    'gemm8/fp8_dyn/dec8/w16/d4': 9,
    'gemm8/fp8_dyn/dec8/w16/d4/loop': 11,
    'gemm8/fp8_dyn/dec8/w16/d4/rows8': 3,
    'gemm8/fp8_dyn/dec8/w16/d8': 3,
    'gemm8/fp8_dyn/dec8/w16/d8/rows8': 3,
    'gemm8/fp8_dyn/dec8/w2/d4': 4,
    'gemm8/fp8_dyn/dec8/w4/d2': 8,
    'gemm8/fp8_dyn/dec8/w4/d7': 32,
    'gemm8/fp8_dyn/dec8/w4/d8': 54,
    'gemm8/fp8_dyn/dec8/w4/d8/rows8': 4,
    'gemm8/fp8_dyn/dec8/w5/d4/rows8': 8,
    'gemm8/fp8_dyn/dec8/w5/d8': 23,
    'gemm8/fp8_dyn/dec8/w7/d4': 23,
    'gemm8/fp8_dyn/dec8/w8/d4': 36,
    'gemm8/fp8_dyn/dec8/w8/d4/rows8': 11,
    'gemm8/fp8_dyn/dec8/w8/d8': 12,
    'gemm8/fp8_dyn/dec8/w8/d8/rows8': 4,
    'gemm8/fp8_dyn/dec8/w9/d1/rows8': 16,
    'gemm8/fp8_dyn/mid8/mt2': 8,
    'gemm8/fp8_dyn/mid8/mt2/kparts': 68,
    'gemm8/fp8_mm_f32/dma128/128x128': 1127,
    'gemm8/fp8_mm_f32/p8/256x256': 109,
    'gemm8/fp8_mm_f32/p8h/256x128': 93,
    'gemm8/fp8_mm_f32/p8h/256x128/kparts': 76,
    'gemm8/fp8_mm_f32/p8p/256x256': 52,
    'gemm8/fp8_mm_f32/regstage/128x128': 47,
    'gemm8/fp8_scaled/dec8/w1/d8': 8,
    'gemm8/fp8_scaled/dec8/w10/d2/rows8': 16,
    'gemm8/fp8_scaled/dec8/w10/d4': 50,
    'gemm8/fp8_scaled/dec8/w10/d8': 24,
    'gemm8/fp8_scaled/dec8/w12/d8': 20,
    'gemm8/fp8_scaled/dec8/w14/d2': 18,
    'gemm8/fp8_scaled/dec8/w14/d8': 16,
    'gemm8/fp8_scaled/dec8/w16/d4': 24,
    'gemm8/fp8_scaled/dec8/w16/d4/loop': 38,
    'gemm8/fp8_scaled/dec8/w16/d4/rows8': 8,
    'gemm8/fp8_scaled/dec8/w16/d8': 12,
    'gemm8/fp8_scaled/dec8/w16/d8/rows8': 12,
    'gemm8/fp8_scaled/dec8/w2/d4': 8,
    'gemm8/fp8_scaled/dec8/w4/d2': 16,
    'gemm8/fp8_scaled/dec8/w4/d7': 64,
    'gemm8/fp8_scaled/dec8/w4/d8': 118,
    'gemm8/fp8_scaled/dec8/w4/d8/rows8': 8,
    'gemm8/fp8_scaled/dec8/w5/d4/rows8': 16,
    'gemm8/fp8_scaled/dec8/w5/d8': 46,
    'gemm8/fp8_scaled/dec8/w7/d4': 46,
    'gemm8/fp8_scaled/dec8/w8/d4': 74,
    'gemm8/fp8_scaled/dec8/w8/d4/rows8': 24,
    'gemm8/fp8_scaled/dec8/w8/d8': 72,
    'gemm8/fp8_scaled/dec8/w8/d8/rows8': 24,
    'gemm8/fp8_scaled/dec8/w9/d1/rows8': 32,
    'gemm8/fp8_scaled/mid8/mt2': 16,
    'gemm8/fp8_scaled/mid8/mt2/kparts': 136,
    'gemm8/fp8_scaled/p8/256x256': 222,
    'gemm8/fp8_scaled/p8h/256x128': 186,
    'gemm8/fp8_scaled/p8h/256x128/kparts': 152,
    'gemm8/fp8_scaled/p8p/256x256': 52,
    'gemm8/fp8_scaled/rb8/128x128': 152,
    'gemm8/fp8_scaled/rb8/128x128/kparts': 40,
    'gemm8/fp8_scaled/rb8/128x32': 20,
    'gemm8/fp8_scaled/rb8/128x32/kparts': 44,
    'gemm8/fp8_scaled/rb8/128x64': 6,
    'gemm8/fp8_scaled/rb8/128x64/kparts': 14,
    'gemm8/fp8_scaled/rb8/64x128': 174,
    'gemm8/fp8_scaled/rb8/64x128/kparts': 156,
    'gemm8/fp8_scaled/rb8/64x32': 56,
    'gemm8/fp8_scaled/rb8/64x32/kparts': 118,
    'gemm8/fp8_scaled/rb8/64x64': 60,
    'gemm8/fp8_scaled/rb8/64x64/kparts': 252,
    'gemm8/fp8_scaled/regstage/128x128': 94,
    'gemm8/fp8_scaled/stream8': 76,
    'gemm8/int8_dyn/dec8/w1/d8': 4,
    'gemm8/int8_dyn/dec8/w10/d2/rows8': 8,
    'gemm8/int8_dyn/dec8/w10/d4': 13,
    'gemm8/int8_dyn/dec8/w10/d8': 6,
    'gemm8/int8_dyn/dec8/w12/d8': 5,
    'gemm8/int8_dyn/dec8/w14/d2': 9,
    'gemm8/int8_dyn/dec8/w14/d8': 4,
    'gemm8/int8_dyn/dec8/w16/d4': 9,
    'gemm8/int8_dyn/dec8/w16/d4/loop': 11,
    'gemm8/int8_dyn/dec8/w16/d4/rows8': 3,
    'gemm8/int8_dyn/dec8/w16/d8': 3,
    'gemm8/int8_dyn/dec8/w16/d8/rows8': 3,
    'gemm8/int8_dyn/dec8/w2/d4': 4,
    'gemm8/int8_dyn/dec8/w4/d2': 8,
    'gemm8/int8_dyn/dec8/w4/d7': 32,
    'gemm8/int8_dyn/dec8/w4/d8': 54,
    'gemm8/int8_dyn/dec8/w4/d8/rows8': 4,
    'gemm8/int8_dyn/dec8/w5/d4/rows8': 8,
    'gemm8/int8_dyn/dec8/w5/d8': 23,
    'gemm8/int8_dyn/dec8/w7/d4': 23,
    'gemm8/int8_dyn/dec8/w8/d4': 36,
    'gemm8/int8_dyn/dec8/w8/d4/rows8': 11,
    'gemm8/int8_dyn/dec8/w8/d8': 12,
    'gemm8/int8_dyn/dec8/w8/d8/rows8': 4,
    'gemm8/int8_dyn/dec8/w9/d1/rows8': 16,
    'gemm8/int8_dyn/mid8/mt2': 8,
    'gemm8/int8_dyn/mid8/mt2/kparts': 68,
    'gemm8/int8_scaled/dec8/w1/d8': 8,
    'gemm8/int8_scaled/dec8/w10/d2/rows8': 16,
    'gemm8/int8_scaled/dec8/w10/d4': 50,
    'gemm8/int8_scaled/dec8/w10/d8': 24,
    'gemm8/int8_scaled/dec8/w12/d8': 20,
    'gemm8/int8_scaled/dec8/w14/d2': 18,
    'gemm8/int8_scaled/dec8/w14/d8': 16,
    'gemm8/int8_scaled/dec8/w16/d4': 24,
    'gemm8/int8_scaled/dec8/w16/d4/loop': 38,
    'gemm8/int8_scaled/dec8/w16/d4/rows8': 8,
    'gemm8/int8_scaled/dec8/w16/d8': 12,
    'gemm8/int8_scaled/dec8/w16/d8/rows8': 12,
    'gemm8/int8_scaled/dec8/w2/d4': 8,
    'gemm8/int8_scaled/dec8/w4/d2': 16,
    'gemm8/int8_scaled/dec8/w4/d7': 64,
    'gemm8/int8_scaled/dec8/w4/d8': 118,
    'gemm8/int8_scaled/dec8/w4/d8/rows8': 8,
    'gemm8/int8_scaled/dec8/w5/d4/rows8': 16,
    'gemm8/int8_scaled/dec8/w5/d8': 46,
    'gemm8/int8_scaled/dec8/w7/d4': 46,
    'gemm8/int8_scaled/dec8/w8/d4': 74,
    'gemm8/int8_scaled/dec8/w8/d4/rows8': 24,
    'gemm8/int8_scaled/dec8/w8/d8': 72,
    'gemm8/int8_scaled/dec8/w8/d8/rows8': 24,
    'gemm8/int8_scaled/dec8/w9/d1/rows8': 32,
    'gemm8/int8_scaled/dma128/128x128': 188,
    'gemm8/int8_scaled/mid8/mt2': 16,
    'gemm8/int8_scaled/mid8/mt2/kparts': 136,
    'gemm8/int8_scaled/p8/256x256': 222,
    'gemm8/int8_scaled/p8h/256x128': 186,
    'gemm8/int8_scaled/p8h/256x128/kparts': 152,
    'gemm8/int8_scaled/p8p/256x256': 52,
    'gemm8/int8_scaled/rb8/128x128': 152,
    'gemm8/int8_scaled/rb8/128x128/kparts': 40,
    'gemm8/int8_scaled/rb8/128x32': 20,
    'gemm8/int8_scaled/rb8/128x32/kparts': 44,
    'gemm8/int8_scaled/rb8/128x64': 6,
    'gemm8/int8_scaled/rb8/128x64/kparts': 14,
    'gemm8/int8_scaled/rb8/64x128': 174,
    'gemm8/int8_scaled/rb8/64x128/kparts': 156,
    'gemm8/int8_scaled/rb8/64x32': 56,
    'gemm8/int8_scaled/rb8/64x32/kparts': 118,
    'gemm8/int8_scaled/rb8/64x64': 60,
    'gemm8/int8_scaled/rb8/64x64/kparts': 252,
    'gemm8/int8_scaled/regstage/128x128': 94,
    'gemm8/int8_scaled/stream8': 76,
    'gemm8/int_mm/dma128/128x128': 1127,
    'gemm8/int_mm/p8/256x256': 109,
    'gemm8/int_mm/p8h/256x128': 93,
    'gemm8/int_mm/p8h/256x128/kparts': 76,
    'gemm8/int_mm/p8p/256x256': 52,
    'gemm8/int_mm/regstage/128x128': 47,
    'int4/g128/rb/w4/nt1/mt1': 12,
    'int4/g128/rb/w4/nt1/mt1/kparts': 132,
    'int4/g128/rb/w4/nt1/mt2': 4,
    'int4/g128/rb/w4/nt1/mt2/kparts': 112,
    'int4/g128/rb/w4/nt1/mt4': 12,
    'int4/g128/rb/w4/nt1/mt4/kparts': 92,
    'int4/g128/rb/w4/nt1/mt8/prod': 4,
    'int4/g128/rb/w4/nt1/mt8/prod/kparts': 68,
    'int4/g128/rb/w8/nt1/mt4': 12,
    'int4/g128/tile/r1/d2/straight': 1,
    'int4/g128/tile/r1/d4': 2,
    'int4/g128/tile/r1/d4/straight': 19,
    'int4/g128/tile/r1/d7/straight': 1,
    'int4/g128/tile/r1/d8/straight': 4,
    'int4/g128/tile/r1/d9/straight': 2,
    'int4/g128/tile/r16/d4': 104,
    'int4/g128/tile/r4/d4': 87,
    'int4/g128/tile/r8/d4': 100,
    'int4/g128/w32/cg1/prod': 199,
    'int4/g128/w32/cg1/prod/kparts': 245,
    'int4/g128/w32/cg2/prod': 151,
    'int4/g256/rb/w4/nt1/mt1': 12,
    'int4/g256/rb/w4/nt1/mt1/kparts': 132,
    'int4/g256/rb/w4/nt1/mt2': 4,
    'int4/g256/rb/w4/nt1/mt2/kparts': 108,
    'int4/g256/rb/w4/nt1/mt4': 8,
    'int4/g256/rb/w4/nt1/mt4/kparts': 92,
    'int4/g256/rb/w4/nt1/mt8/prod/kparts': 68,
    'int4/g256/rb/w8/nt1/mt4': 12,
    'int4/g256/tile/r1/d2/straight': 1,
    'int4/g256/tile/r1/d4': 1,
    'int4/g256/tile/r1/d4/straight': 19,
    'int4/g256/tile/r1/d7/straight': 1,
    'int4/g256/tile/r1/d8/straight': 4,
    'int4/g256/tile/r1/d9/straight': 2,
    'int4/g256/tile/r16/d4': 96,
    'int4/g256/tile/r4/d4': 84,
    'int4/g256/tile/r8/d4': 96,
    'int4/g256/w32/cg1/prod': 199,
    'int4/g256/w32/cg1/prod/kparts': 226,
    'int4/g256/w32/cg2/prod': 151,
    'int4/g32/rb/w4/nt1/mt1': 12,
    'int4/g32/rb/w4/nt1/mt1/kparts': 132,
    'int4/g32/rb/w4/nt1/mt2': 4,
    'int4/g32/rb/w4/nt1/mt2/kparts': 112,
    'int4/g32/rb/w4/nt1/mt4': 12,
    'int4/g32/rb/w4/nt1/mt4/kparts': 92,
    'int4/g32/rb/w4/nt1/mt8/prod': 4,
    'int4/g32/rb/w4/nt1/mt8/prod/kparts': 68,
    'int4/g32/rb/w8/nt1/mt4': 12,
    'int4/g32/tile/r1/d2/straight': 1,
    'int4/g32/tile/r1/d4': 2,
    'int4/g32/tile/r1/d4/straight': 19,
    'int4/g32/tile/r1/d7/straight': 1,
    'int4/g32/tile/r1/d8/straight': 4,
    'int4/g32/tile/r1/d9/straight': 2,
    'int4/g32/tile/r16/d4': 104,
    'int4/g32/tile/r4/d4': 87,
    'int4/g32/tile/r8/d4': 100,
    'int4/g32/w32/cg1/prod': 350,
    'int4/g32/w32/cg1/prod/kparts': 245,
    'int4/g64/rb/w4/nt1/mt1': 12,
    'int4/g64/rb/w4/nt1/mt1/kparts': 132,
    'int4/g64/rb/w4/nt1/mt2': 4,
    'int4/g64/rb/w4/nt1/mt2/kparts': 112,
    'int4/g64/rb/w4/nt1/mt4': 12,
    'int4/g64/rb/w4/nt1/mt4/kparts': 92,
    'int4/g64/rb/w4/nt1/mt8/prod': 4,
    'int4/g64/rb/w4/nt1/mt8/prod/kparts': 68,
    'int4/g64/rb/w8/nt1/mt4': 12,
    'int4/g64/tile/r1/d2/straight': 1,
    'int4/g64/tile/r1/d4': 2,
    'int4/g64/tile/r1/d4/straight': 19,
    'int4/g64/tile/r1/d7/straight': 1,
    'int4/g64/tile/r1/d8/straight': 4,
    'int4/g64/tile/r1/d9/straight': 2,
    'int4/g64/tile/r16/d4': 104,
    'int4/g64/tile/r4/d4': 87,
    'int4/g64/tile/r8/d4': 100,
    'int4/g64/w32/cg1/prod': 350,
    'int4/g64/w32/cg1/prod/kparts': 245,
    'mx/e2m1_codes/stream/w1/mt1': 864,
    'mx/e2m1_codes/stream/w1/mt2': 216,
    'mx/e2m1_codes/stream/w16/mt1': 384,
    'mx/e2m1_codes/stream/w16/mt2': 96,
    'mx/e2m1_codes/stream/w2/mt1': 576,
    'mx/e2m1_codes/stream/w2/mt2': 144,
    'mx/e2m1_codes/stream/w4/mt1': 256,
    'mx/e2m1_codes/stream/w4/mt2': 64,
    'mx/e2m1_codes/stream/w8/mt1': 512,
    'mx/e2m1_codes/stream/w8/mt2': 128,
    'mx/e2m1_codes/tile/w4/mt4': 4374,
    'mx/e2m1_fused/stream/w1/mt1': 864,
    'mx/e2m1_fused/stream/w1/mt2': 216,
    'mx/e2m1_fused/stream/w16/mt1': 384,
    'mx/e2m1_fused/stream/w16/mt2': 96,
    'mx/e2m1_fused/stream/w2/mt1': 576,
    'mx/e2m1_fused/stream/w2/mt2': 144,
    'mx/e2m1_fused/stream/w4/mt1': 256,
    'mx/e2m1_fused/stream/w4/mt2': 64,
    'mx/e2m1_fused/stream/w8/mt1': 512,
    'mx/e2m1_fused/stream/w8/mt2': 128,
    'mx/e4m3_codes/stream/w1/mt1': 864,
    'mx/e4m3_codes/stream/w1/mt2': 216,
    'mx/e4m3_codes/stream/w1/mt4': 216,
    'mx/e4m3_codes/stream/w16/mt1': 384,
    'mx/e4m3_codes/stream/w16/mt2': 96,
    'mx/e4m3_codes/stream/w2/mt1': 576,
    'mx/e4m3_codes/stream/w2/mt2': 144,
    'mx/e4m3_codes/stream/w2/mt4': 144,
    'mx/e4m3_codes/stream/w4/mt1': 256,
    'mx/e4m3_codes/stream/w4/mt2': 64,
    'mx/e4m3_codes/stream/w4/mt4': 64,
    'mx/e4m3_codes/stream/w8/mt1': 512,
    'mx/e4m3_codes/stream/w8/mt2': 128,
    'mx/e4m3_codes/stream/w8/mt4': 224,
    'mx/e4m3_codes/tile/w4/mt4': 3726,
    'mx/e4m3_fused/stream/w1/mt1': 864,
    'mx/e4m3_fused/stream/w1/mt2': 216,
    'mx/e4m3_fused/stream/w1/mt4': 216,
    'mx/e4m3_fused/stream/w16/mt1': 384,
    'mx/e4m3_fused/stream/w16/mt2': 96,
    'mx/e4m3_fused/stream/w2/mt1': 576,
    'mx/e4m3_fused/stream/w2/mt2': 144,
    'mx/e4m3_fused/stream/w2/mt4': 144,
    'mx/e4m3_fused/stream/w4/mt1': 256,
    'mx/e4m3_fused/stream/w4/mt2': 64,
    'mx/e4m3_fused/stream/w4/mt4': 64,
    'mx/e4m3_fused/stream/w8/mt1': 512,
    'mx/e4m3_fused/stream/w8/mt2': 128,
    'mx/e4m3_fused/stream/w8/mt4': 224,
}

# (case, signature): what derive_grouped_cases(lib) picks on the grid, and the grid cells per signature
GROUPED_CASES = [
    (GCase('grouped', 'fp8', 48, 16, 128, 1, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 1, 208, 128, 1, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 1, 16, 2048, 1, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 1, 16, 128, 2, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 1, 16, 128, 8, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 17, 16, 128, 8, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 65, 16, 128, 2, True, 'one', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 1, 16, 128, 65, True, 'one', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 1, 16, 128, 1, False, 'spread', ''), 'grouped/fp8/rb8/w4/mt4/qs1'),
    (GCase('grouped', 'fp8', 49, 16, 128, 1, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'fp8', 49, 208, 128, 1, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'fp8', 49, 16, 2048, 1, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'fp8', 97, 16, 128, 2, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'fp8', 385, 16, 128, 8, True, 'spread', ''), 'grouped/fp8/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'fp8', 129, 16, 128, 1, True, 'one', ''), 'grouped/fp8/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'fp8', 3073, 16, 128, 64, True, 'spread', ''), 'grouped/fp8/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'fp8', 3073, 208, 128, 64, True, 'spread', ''), 'grouped/fp8/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'fp8', 3073, 16, 2048, 64, True, 'spread', ''), 'grouped/fp8/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'fp8', 3073, 16, 128, 64, True, 'one', ''), 'grouped/fp8/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'fp8', 3121, 16, 128, 65, True, 'one', ''), 'grouped/fp8/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'mx', 48, 16, 512, 1, True, 'spread', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 1, 1024, 512, 1, True, 'spread', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 1, 16, 2048, 1, True, 'spread', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 1, 16, 512, 2, True, 'spread', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 1, 16, 512, 8, True, 'spread', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 17, 16, 512, 8, True, 'spread', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 65, 16, 512, 2, True, 'one', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 127, 16, 512, 16, True, 'spread', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 1, 16, 14336, 1, True, 'spread', ''), 'grouped/mx/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx', 48, 16, 128, 1, True, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 1, 208, 128, 1, True, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 1, 16, 2048, 1, False, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 1, 16, 128, 2, True, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 1, 16, 128, 8, True, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 17, 16, 128, 8, True, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 65, 16, 128, 2, True, 'one', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 127, 16, 384, 16, True, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 1, 16, 4096, 1, False, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 1, 16, 14336, 1, False, 'spread', ''), 'grouped/mx/mx_stream/w8/qs1/sw3'),
    (GCase('grouped', 'mx', 3120, 16, 512, 65, True, 'spread', ''), 'grouped/mx/rb8/w4/mt4/qs4'),
    (GCase('grouped', 'mx', 1, 208, 512, 65, True, 'spread', ''), 'grouped/mx/rb8/w4/mt4/qs4'),
    (GCase('grouped', 'mx', 1, 16, 2048, 65, True, 'spread', ''), 'grouped/mx/rb8/w4/mt4/qs4'),
    (GCase('grouped', 'mx', 1, 16, 512, 65, True, 'one', ''), 'grouped/mx/rb8/w4/mt4/qs4'),
    (GCase('grouped', 'mx', 3120, 16, 128, 65, True, 'spread', ''), 'grouped/mx/rb8/w4/mt4/slim/qs1'),
    (GCase('grouped', 'mx', 1, 208, 128, 65, True, 'spread', ''), 'grouped/mx/rb8/w4/mt4/slim/qs1'),
    (GCase('grouped', 'mx', 1, 16, 2048, 65, False, 'spread', ''), 'grouped/mx/rb8/w4/mt4/slim/qs1'),
    (GCase('grouped', 'mx', 1, 16, 128, 65, True, 'one', ''), 'grouped/mx/rb8/w4/mt4/slim/qs1'),
    (GCase('grouped', 'mx', 49, 16, 128, 1, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'mx', 49, 208, 128, 1, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'mx', 49, 16, 2048, 1, False, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'mx', 97, 16, 128, 2, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'mx', 385, 16, 128, 8, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'mx', 129, 16, 128, 1, True, 'one', ''), 'grouped/mx/rb8/w4/mt8/qs1'),
    (GCase('grouped', 'mx', 49, 16, 512, 1, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs4'),
    (GCase('grouped', 'mx', 49, 208, 512, 1, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs4'),
    (GCase('grouped', 'mx', 49, 16, 2048, 1, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs4'),
    (GCase('grouped', 'mx', 97, 16, 512, 2, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs4'),
    (GCase('grouped', 'mx', 385, 16, 512, 8, True, 'spread', ''), 'grouped/mx/rb8/w4/mt8/qs4'),
    (GCase('grouped', 'mx', 129, 16, 512, 1, True, 'one', ''), 'grouped/mx/rb8/w4/mt8/qs4'),
    (GCase('grouped', 'mx', 3073, 16, 128, 64, True, 'spread', ''), 'grouped/mx/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'mx', 3073, 208, 128, 64, True, 'spread', ''), 'grouped/mx/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'mx', 3073, 16, 2048, 64, False, 'spread', ''), 'grouped/mx/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'mx', 3073, 16, 128, 64, True, 'one', ''), 'grouped/mx/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'mx', 3121, 16, 128, 65, True, 'one', ''), 'grouped/mx/rb8/w8/mt8/qs1'),
    (GCase('grouped', 'mx', 3073, 16, 512, 64, True, 'spread', ''), 'grouped/mx/rb8/w8/mt8/qs4'),
    (GCase('grouped', 'mx', 3073, 208, 512, 64, True, 'spread', ''), 'grouped/mx/rb8/w8/mt8/qs4'),
    (GCase('grouped', 'mx', 3073, 16, 2048, 64, True, 'spread', ''), 'grouped/mx/rb8/w8/mt8/qs4'),
    (GCase('grouped', 'mx', 3073, 16, 512, 64, True, 'one', ''), 'grouped/mx/rb8/w8/mt8/qs4'),
    (GCase('grouped', 'mx', 3121, 16, 512, 65, True, 'one', ''), 'grouped/mx/rb8/w8/mt8/qs4'),
    (GCase('grouped', 'mx_dyn', 48, 16, 512, 1, True, 'spread', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 48, 16, 512, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 1024, 512, 1, True, 'spread', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 1024, 512, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 16, 2048, 1, True, 'spread', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 16, 2048, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 16, 512, 2, True, 'spread', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 16, 512, 2, True, 'spread', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 16, 512, 8, True, 'spread', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 16, 512, 8, True, 'spread', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 17, 16, 512, 8, True, 'spread', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 17, 16, 512, 8, True, 'spread', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 65, 16, 512, 2, True, 'one', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 65, 16, 512, 2, True, 'one', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 127, 16, 512, 16, True, 'spread', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 127, 16, 512, 16, True, 'spread', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 16, 14336, 1, True, 'spread', 'floor'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn', 1, 16, 14336, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 48, 16, 512, 1, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 48, 16, 512, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 1024, 512, 1, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 1024, 512, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 2048, 1, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 2048, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 512, 2, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 512, 2, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 512, 8, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 512, 8, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 17, 16, 512, 8, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 17, 16, 512, 8, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 65, 16, 512, 2, True, 'one', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 65, 16, 512, 2, True, 'one', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 127, 16, 512, 8, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 127, 16, 512, 8, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 4096, 1, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 4096, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 14336, 1, True, 'spread', 'floor'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_dyn_pair', 1, 16, 14336, 1, True, 'spread', 'rceil'), 'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2'),
    (GCase('grouped', 'mx_pair', 48, 16, 512, 1, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 1, 1024, 512, 1, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 1, 16, 2048, 1, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 1, 16, 512, 2, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 1, 16, 512, 8, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 17, 16, 512, 8, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 65, 16, 512, 2, True, 'one', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 127, 16, 512, 8, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 1, 16, 4096, 1, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
    (GCase('grouped', 'mx_pair', 1, 16, 14336, 1, True, 'spread', ''), 'grouped/mx_pair/mx_stream/w16/qs4/sw3'),
]
GROUPED_REACH = {
    'grouped/fp8/rb8/w4/mt4/qs1': 4536,
    'grouped/fp8/rb8/w4/mt8/qs1': 1008,
    'grouped/fp8/rb8/w8/mt8/qs1': 336,
    'grouped/mx/mx_stream/w16/qs4/sw3': 1004,
    'grouped/mx/mx_stream/w8/qs1/sw3': 2008,
    'grouped/mx/rb8/w4/mt4/qs4': 508,
    'grouped/mx/rb8/w4/mt4/slim/qs1': 1016,
    'grouped/mx/rb8/w4/mt8/qs1': 672,
    'grouped/mx/rb8/w4/mt8/qs4': 336,
    'grouped/mx/rb8/w8/mt8/qs1': 224,
    'grouped/mx/rb8/w8/mt8/qs4': 112,
    'grouped/mx_dyn/mx_stream/w16/qs4/sw3/cast2': 1004,
    'grouped/mx_dyn_pair/mx_stream/w16/qs4/sw3/cast2': 972,
    'grouped/mx_pair/mx_stream/w16/qs4/sw3': 972,
}

if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from ao_amd import _lib

    lib = _lib.lib()
    print("CASES = [")
    for c, sig in derive_cases(lib):
        print("    (Case%r, %r)," % (tuple(c), sig))
    print("]")
    print("REACH = {")
    for sig, items in sorted(reachable(lib).items()):
        print("    %r: %d," % (sig, len(items)))
    print("}")
    print("GROUPED_CASES = [")
    for c, sig in derive_grouped_cases(lib):
        print("    (GCase%r, %r)," % (tuple(c), sig))
    print("]")
    print("GROUPED_REACH = {")
    for sig, items in sorted(grouped_reachable(lib).items()):
        print("    %r: %d," % (sig, len(items)))
    print("}")
