"""The parity case list covers every GEMM route (CPU only): every signature the product reaches on the discovery grid has cases at its
edges, and the parity checker rejects the faults it exists to catch."""
import numpy as np
import pytest
import torch

import _parity
import route_cases as rc
from ao_amd import _lib
from oracle import bf16, int4_ref


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@pytest.fixture(scope="module")
def grid(lib):
    return rc.reachable(lib)


def _smallest(items):
    return min((c for c, _, _ in items), key=rc.cost)


def test_every_reachable_signature_has_a_case(grid):
    covered = {sig for _, sig in rc.CASES}
    missing = {sig: _smallest(items) for sig, items in grid.items() if sig not in covered}
    assert not missing, "routes without a parity case (signature: smallest grid shape):\n" + "\n".join(
        "  %s: %r" % kv for kv in sorted(missing.items()))


def test_every_case_reaches_its_signature(lib):
    wrong = [(c, sig, rc.signature(lib, c)) for c, sig in rc.CASES if rc.signature(lib, c) != sig]
    assert not wrong, "cases that no longer reach their recorded route (case, recorded, now):\n" + "\n".join("  %r" % (w,) for w in wrong)


def test_cases_meet_the_edge_requirements(lib, grid):
    """Band edge, ragged M, ragged N, uneven K parts and an unaligned-scale route change: each signature has a case for every one of
    them that some grid shape of that signature meets, each (entry, kernel) of the scaled entries runs once on unaligned scales, and
    every case of an entry that takes a bias runs without and with one."""
    have = {}
    for c, sig in rc.CASES:
        have.setdefault(sig, set()).update(rc.properties(lib, c))
    unmet = []
    for sig, items in sorted(grid.items()):
        reqs, props = rc.needed(lib, sig, items)
        for q in reqs:
            if q == "unaligned":
                continue
            if q not in have.get(sig, ()):
                shape = next(c for c, p in props if q in p)
                unmet.append("  %s: no %s case (smallest: %r)" % (sig, q, shape))
    unaligned_have = {tuple(sig.split("/")[1:3]) for c, sig in rc.CASES if not c.aligned}
    unaligned_need = {tuple(sig.split("/")[1:3]) for sig, items in grid.items() if sig.startswith(("gemm8/", "mx/"))
                      and any(not c.aligned for c, _, _ in items)}
    unmet += ["  %s / %s: no unaligned-scale case" % k for k in sorted(unaligned_need - unaligned_have)]
    # an entry that takes a bias runs every case of every signature both without and with one
    cases = {tuple(c) for c, _ in rc.CASES}
    for c, sig in rc.CASES:
        if c.entry in rc.WITH_BIAS and tuple(c[:6]) + (not c.bias, c.aligned) not in cases:
            unmet.append("  %s: %r has no twin %s a bias" % (sig, c, "without" if c.bias else "with"))
    assert not unmet, "edge requirements without a case:\n" + "\n".join(unmet)


def test_committed_cases_are_what_the_grid_derives(lib):
    """The committed list is derive_cases's pick: a route change shows up as a diff to review (`python tests/route_cases.py`)."""
    assert [(tuple(c), s) for c, s in rc.derive_cases(lib)] == [(tuple(c), s) for c, s in rc.CASES]


def test_cases_are_valid_and_small(lib):
    for c, _ in rc.CASES:
        assert c.M >= 1
        if c.family == "mx":  # the MX dense linears: K in 32-blocks, any N
            assert c.K % 32 == 0 and c.N >= 1, c
        else:
            assert c.K % 16 == 0
            if c.family != "gemm8" or c.entry not in ("int8_scaled", "int_mm"):
                assert c.N % 16 == 0, c
        assert c.M * c.N * c.K <= 2048 * 1280 * 8192, c  # the largest shape a signature needs today
    for c, _ in rc.GROUPED_CASES:
        assert c.M >= 1 and c.K % 128 == 0 and c.N % 16 == 0, c
        assert c.M * c.N * c.K <= 2048 * 1280 * 8192, c
        assert c.E * c.N * c.K <= 2 ** 24, c  # the expert weights


# ---- the grouped GEMMs ----

@pytest.fixture(scope="module")
def ggrid(lib):
    return rc.grouped_reachable(lib)


def test_every_grouped_signature_has_a_case(ggrid):
    covered = {sig for _, sig in rc.GROUPED_CASES}
    missing = {sig: min((c for c, _, _ in items), key=rc.grouped_cost) for sig, items in ggrid.items() if sig not in covered}
    assert not missing, "grouped routes without a parity case (signature: smallest grid shape):\n" + "\n".join(
        "  %s: %r" % kv for kv in sorted(missing.items()))


def test_every_grouped_case_reaches_its_signature(lib):
    wrong = [(c, sig, rc.grouped_route_of(lib, c)) for c, sig in rc.GROUPED_CASES]
    wrong = [(c, sig, r and r["sig"]) for c, sig, r in wrong if r is None or r["sig"] != sig]
    assert not wrong, "grouped cases that no longer reach their recorded route (case, recorded, now):\n" + "\n".join("  %r" % (w,) for w in wrong)


def test_grouped_cases_meet_the_edge_requirements(lib, ggrid):
    """Band edge, ragged M and N, more than one column tile, every group-offsets requirement the signature admits (empty experts first,
    middle and last, a one-row group, a group starting inside an m-tile, a group larger than one slab, all rows on one expert, rows
    past offs[-1], tokens on experts >= 64, stream-K shares over two experts and cut tiles), one unaligned case per (entry, kernel),
    and both scaling modes of every fused-cast case."""
    have = {}
    for c, sig in rc.GROUPED_CASES:
        have.setdefault(sig, set()).update(rc.grouped_properties(lib, c))
    unmet = []
    for sig, items in sorted(ggrid.items()):
        reqs, props = rc.grouped_needed(lib, sig, items)
        for q in reqs:
            if q != "unaligned" and q not in have.get(sig, ()):
                unmet.append("  %s: no %s case (smallest: %r)" % (sig, q, next(c for c, p in props if q in p)))
    unaligned_have = {tuple(sig.split("/")[1:3]) for c, sig in rc.GROUPED_CASES if not c.aligned}
    unaligned_need = {tuple(sig.split("/")[1:3]) for sig, items in ggrid.items() if any(not c.aligned for c, _, _ in items)}
    unmet += ["  %s / %s: no unaligned case" % k for k in sorted(unaligned_need - unaligned_have)]
    cases = {tuple(c) for c, _ in rc.GROUPED_CASES}
    for c, sig in rc.GROUPED_CASES:
        if c.entry in rc.FUSED:
            twin = tuple(c[:8]) + ({"floor": "rceil", "rceil": "floor"}[c.mode],)
            if twin not in cases:
                unmet.append("  %s: %r has no twin in the other scaling mode" % (sig, c))
    assert not unmet, "grouped edge requirements without a case:\n" + "\n".join(unmet)


def test_committed_grouped_cases_are_what_the_grid_derives(lib):
    assert [(tuple(c), s) for c, s in rc.derive_grouped_cases(lib)] == [(tuple(c), s) for c, s in rc.GROUPED_CASES]


def test_grouped_bands_have_not_moved(ggrid):
    """grouped8_route's bands (the decode-size bound, the 8-wave threshold, the stream-K bounds ...): regenerate GROUPED_CASES /
    GROUPED_REACH (`python tests/route_cases.py`) after reviewing the cases a moved band needs."""
    now = {sig: len(items) for sig, items in ggrid.items()}
    moved = {sig: (rc.GROUPED_REACH.get(sig, 0), now.get(sig, 0)) for sig in set(now) | set(rc.GROUPED_REACH)
             if rc.GROUPED_REACH.get(sig, 0) != now.get(sig, 0)}
    assert not moved, "grouped signatures whose reach on the grid changed (committed, now):\n" + "\n".join(
        "  %s: %d -> %d" % (sig, a, b) for sig, (a, b) in sorted(moved.items()))


def test_group_sizes_patterns():
    """The offsets patterns: the rows they place, and the requirements they are built to meet."""
    for E in rc.E_GRID:
        for M in rc.gm_grid(E):
            for pat in rc.OFFS:
                sizes = rc.group_sizes(E, M, pat)
                assert len(sizes) == E and min(sizes) >= 0 and sum(sizes) <= M
                assert sum(sizes) == M if pat == "one" else sum(sizes) == M - (M >= 2)
    s = rc.group_sizes(8, 129, "spread")
    assert s[0] == 0 and s[4] == 0 and s[7] == 0 and s[1] == 1 and s[2] == 99 and sum(s) == 128


# ---- the checker, on oracle outputs and injected faults ----

def _fp8_problem(seed=0, M=40, N=48, K=512, parts=4):
    """A float64 reference of an fp8 scaled GEMM with spread scales, and fp32 sums of the same products in other orders."""
    g = torch.Generator().manual_seed(seed)
    e4 = torch.from_numpy(__import__("oracle.fp8_ref", fromlist=["E4M3"]).E4M3.astype(np.float64))
    finite = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF)])
    a = e4[finite[torch.randint(0, 254, (M, K), generator=g)]]
    b = e4[finite[torch.randint(0, 254, (N, K), generator=g)]]
    sa = torch.exp2(torch.rand(M, generator=g, dtype=torch.float64) * 14 - 10).float().double()
    sb = torch.exp2(torch.rand(N, generator=g, dtype=torch.float64) * 14 - 10).float().double()
    ref = (a @ b.T) * sa[:, None] * sb[None, :]
    S = (a.abs() @ b.abs().T) * sa[:, None] * sb[None, :]
    perm = torch.randperm(K, generator=g)
    shuffled = (a[:, perm].float()[:, :, None] * b[:, perm].float().T[None]).cumsum(1)[:, -1]  # fp32, another order
    kb = K // parts
    blocks = [(a[:, p * kb:(p + 1) * kb].float() @ b[:, p * kb:(p + 1) * kb].float().T) for p in range(parts)]
    split = sum(blocks[1:], blocks[0])
    return a, b, sa, sb, ref, S, shuffled, split, blocks


def _buf_with(y, dtype=torch.bfloat16):
    M, N = y.shape
    buf = _parity.Guarded(M, N, dtype, "cpu")
    buf.out.copy_(y.to(dtype))
    return buf


def _scaled(acc, sa, sb):
    return (acc.float() * sa.float()[:, None] * sb.float()[None, :])


def test_checker_accepts_oracle_and_fp32_orders():
    a, b, sa, sb, ref, S, shuffled, split, _ = _fp8_problem()
    K = a.shape[1]
    for y in (_parity.oracle_round(ref, torch.bfloat16), _scaled(shuffled, sa, sb), _scaled(split, sa, sb)):
        _parity.check(_buf_with(y), ref64=ref, S=S, K=K)
    _parity.check(_buf_with(shuffled, torch.float32), ref64=a @ b.T, S=a.abs() @ b.abs().T, K=K)
    _parity.check(_buf_with(split, torch.float32), ref64=a @ b.T, S=a.abs() @ b.abs().T, K=K)


def _rejects(buf, **kw):
    msgs = _parity.problems(buf, **kw)
    assert msgs, "the checker accepted an injected fault"
    return msgs


def test_checker_rejects_injected_faults():
    a, b, sa, sb, ref, S, _, split, blocks = _fp8_problem()
    K = a.shape[1]
    kw = dict(ref64=ref, S=S, K=K)
    good = _parity.oracle_round(ref, torch.bfloat16)

    # one element off by 4 bf16 ulp (the largest one: no accumulation slack there hides it)
    y = good.clone()
    i, j = divmod(int(ref.abs().argmax()), ref.shape[1])
    y.view(torch.int16)[i, j] += 4
    assert "row %d, column %d" % (i, j) in " ".join(_rejects(_buf_with(y), **kw))
    # a 16-column strip of one row zeroed
    y = good.clone()
    y[7, 16:32] = 0
    _rejects(_buf_with(y), **kw)
    # one row scale swapped with its neighbour
    sa2 = sa.clone()
    sa2[[3, 4]] = sa2[[4, 3]]
    _rejects(_buf_with(_scaled(split, sa2, sb)), **kw)
    # one K part dropped
    _rejects(_buf_with(_scaled(split - blocks[2], sa, sb)), **kw)
    # the sentinel left in one element
    buf = _buf_with(good)
    buf.bits()[5, 9] = buf.sentinel
    assert "unwritten" in " ".join(_rejects(buf, **kw))
    # one write into the guard rows
    buf = _buf_with(good)
    buf.raw[-3] = 0
    assert "guard rows" in " ".join(_rejects(buf, **kw))
    buf = _buf_with(good)
    buf.raw[2] = 0
    assert "guard bytes" in " ".join(_rejects(buf, **kw))


def test_checker_rejects_the_next_int4_group():
    """One group of an int4 weight dequantised with the next group's scale and zero."""
    g = torch.Generator().manual_seed(1)
    M, N, K, G = 8, 32, 512, 64
    q = torch.randint(0, 16, (N, K), generator=g)
    s = torch.exp2(torch.rand(K // G, N, generator=g) * 8 - 6).bfloat16().float()
    z = (torch.exp2(torch.rand(K // G, N, generator=g) * 8 - 6) * (torch.randint(0, 2, (K // G, N), generator=g) * 2 - 1)).bfloat16().float()
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.rand(M, 1, generator=g) * 16 - 8)).bfloat16().float()

    def deq(s, z):
        w = ((q - 8).float().view(N, K // G, G) * s.T[:, :, None]).bfloat16().float() + z.T[:, :, None]
        return w.bfloat16().double().view(N, K)

    w = deq(s, z)
    ref = x.double() @ w.T
    S = x.double().abs() @ w.abs().T
    _parity.check(_buf_with(ref.float()), ref64=ref, S=S, K=K)
    s2, z2 = s.clone(), z.clone()
    s2[3], z2[3] = s[4], z[4]
    _rejects(_buf_with((x.double() @ deq(s2, z2).T).float()), ref64=ref, S=S, K=K)


def test_checker_exact_mode():
    y = torch.randint(-1000, 1000, (20, 24), dtype=torch.int32)
    buf = _buf_with(y, torch.int32)
    _parity.check(buf, ref_bits=y)
    y2 = y.clone()
    y2[11, 5] += 1
    assert "row 11, column 5" in " ".join(_rejects(buf, ref_bits=y2))


def test_torch_int4_pack_and_dequant_match_the_oracle():
    """The GPU test packs and dequantises int4 weights in torch: the same bits as oracle.int4_ref on one case per group size."""
    from test_route_parity_gpu import dequant_tinygemm, pack_int4

    rng = np.random.default_rng(3)
    N, K = 48, 512
    q = rng.integers(0, 16, (N, K))
    want = int4_ref.convert_weight_to_int4pack(int4_ref.nibble_pack(q))
    got = pack_int4(torch.from_numpy(q))
    assert np.array_equal(got.numpy(), want)
    for G in rc.GROUPS:
        sz = bf16.bf16_round(rng.standard_normal((K // G, N, 2)).astype(np.float32) * 4)
        want = int4_ref.dequantize_tinygemm(q, sz, G)
        got = dequant_tinygemm(torch.from_numpy(q), torch.from_numpy(sz).bfloat16(), G)
        assert np.array_equal(got.float().numpy(), want)


def test_bands_have_not_moved(grid):
    """A route band that moved (a changed rule constant) shows as a signature reaching another number of grid cells: review the cases
    it needs and regenerate CASES / REACH (`python tests/route_cases.py`)."""
    now = {sig: len(items) for sig, items in grid.items()}
    moved = {sig: (rc.REACH.get(sig, 0), now.get(sig, 0)) for sig in set(now) | set(rc.REACH) if rc.REACH.get(sig, 0) != now.get(sig, 0)}
    assert not moved, "signatures whose reach on the grid changed (committed, now):\n" + "\n".join(
        "  %s: %d -> %d" % (sig, a, b) for sig, (a, b) in sorted(moved.items()))


# ---- the checker on the MX and grouped families' faults ----

def _mx_problem(M=40, N=48, K=512, seed=5):
    """e4m3 codes and E8M0 scales drawn as on the GPU, the float64 product and S."""
    from test_route_parity_gpu import Draw, mx_dequant

    d = Draw(seed, "cpu")
    a, sa, b, sb = d.fp8(M, K), d.e8m0(M, K // 32), d.fp8(N, K), d.e8m0(N, K // 32)
    A, B = mx_dequant(a, sa, "e4m3"), mx_dequant(b, sb, "e4m3")
    return a, sa, b, sb, A @ B.T, A.abs() @ B.abs().T


def test_checker_rejects_mx_dense_faults():
    """One block's scale read from its neighbour; the e4m3 lane map with its halves swapped (lane group kq's scale applied to
    k = 64 + 16 kq .. and 16 kq .., i.e. blocks (0, 1) and (2, 3) of every k step trading scales)."""
    from test_route_parity_gpu import K_FLOOR_MX, mx_dequant

    a, sa, b, sb, ref, S = _mx_problem()
    K = a.shape[1]
    kw = dict(ref64=ref, S=S, K=K, k_floor=K_FLOOR_MX["e4m3"])
    _parity.check(_buf_with(_parity.oracle_round(ref, torch.bfloat16)), **kw)

    def out(sa2, sb2):
        return _buf_with(mx_dequant(a, sa2, "e4m3") @ mx_dequant(b, sb2, "e4m3").T)

    sa2 = sa.clone()
    sa2[7, 5] = sa[7, 6]
    assert "row 7" in " ".join(_rejects(out(sa2, sb), **kw))
    swap = torch.arange(K // 32).view(-1, 4)[:, [2, 3, 0, 1]].flatten()
    _rejects(out(sa[:, swap], sb[:, swap]), **kw)


def test_checker_rejects_grouped_faults():
    """A small MX grouped problem (an empty first expert, a one-row group, a group over a 64-row slab, one row past offs[-1]): the next
    expert's weights for one group, a row past offs[-1] written, a row inside a group left at the sentinel, pair outputs swapped."""
    from test_route_parity_gpu import mx_dequant
    from test_route_parity_grouped_gpu import K_FLOOR_GROUPED, GRun

    case = rc.GCase("grouped", "mx_pair", 130, 32, 256, 5, True, "spread", "")
    run = GRun(case, 9, "cpu")
    sizes, w = run.sizes, run.written
    assert sizes[0] == 0 and 1 in sizes and max(sizes) > 64 and w == case.M - 1
    A = mx_dequant(run.a, run.sa, "e4m3")

    def outputs(swap=False, wrong_group=None):
        ys = []
        for i in range(2):
            y = torch.zeros(case.M, case.N, dtype=torch.float64)
            lo = 0
            for e, n in enumerate(sizes):
                if n:
                    ew = e + 1 if e == wrong_group else e
                    W = mx_dequant(run.b[i][ew], run.sb[i][ew], "e4m3")
                    y[lo:lo + n] = A[lo:lo + n] @ W.T
                lo += n
            buf = _parity.Guarded(case.M, case.N, torch.bfloat16, "cpu")
            buf.out[:w].copy_(y[:w].to(torch.bfloat16))
            ys.append(buf)
        return ys[::-1] if swap else ys

    for buf, kw in zip(outputs(), run.refs):
        assert kw["k_floor"] == K_FLOOR_GROUPED["mx"]
        _parity.check(buf, **kw)
    g = next(e for e, n in enumerate(sizes) if n > 1 and e + 1 < len(sizes))
    _rejects(outputs(wrong_group=g)[0], **run.refs[0])
    buf = outputs()[0]
    buf.bits()[w, 3] = 0
    assert "past %d" % w in " ".join(_rejects(buf, **run.refs[0]))
    buf = outputs()[0]
    buf.bits()[w - 1, 5] = buf.sentinel
    assert "unwritten" in " ".join(_rejects(buf, **run.refs[0]))
    y1, y3 = outputs(swap=True)
    _rejects(y1, **run.refs[0])
    _rejects(y3, **run.refs[1])
