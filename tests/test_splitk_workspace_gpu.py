"""The split-K workspace table (csrc/runtime.hip: one parts area + ticket array per (device, stream), 8 slots, grown on demand, outgrown
buffers retired, the least recently used slot evicted by a ninth stream) under what a serving process does with it: several streams at
once, captured graphs across a growth, more streams than slots, ao_splitk_reserve, host threads.

Operands and references are those of the route-parity tests (Run / GRun); no tolerance is added here.  Every case of USERS is launched
once, alone, on the default stream and held to its float64 reference (_parity.check / GRun.check): those output bits are the case's
"solo bits".  The meetings add their parts in part order, so every later launch of the case -- on any stream, next to anything -- must
give exactly those bits with clean guards: the rule the parity tests already hold their second launch to.  ao_splitk_query shows each
test the table state it claims to exercise (who holds a slot, its capacity and base, the retired buffers).

torch.cuda.Stream() deals from a pool of 32 per device, so a "fresh" stream is manufactured, not assumed: the tests share 12 distinct
streams, and one holds no slot once 8 others have launched after it (_hand_over_a_minimum_slot, which also puts an 8 MiB slot last in
the eviction order, whatever earlier tests left in the table).  The two tests that read absolute capacities run first.
"""
import ctypes
import threading
import time

import pytest
import torch

import _parity
import route_cases as rc
from ao_amd import _lib
from test_route_parity_gpu import _SPLIT, Run
from test_route_parity_grouped_gpu import GRun

MIB = 1 << 20
MIN_BYTES = 8 * MIB    # runtime.hip kSplitMinFloats * 4
CAP_BYTES = 128 * MIB  # splitk.h kSplitSlotFloats * 4
SLOTS = 8              # splitk.h kSplitSlots
ROUNDS, PER_ROUND, PER_THREAD = 20, 8, 25
P8_PARTS = 16
# what the forced 16-part 256 x 128 form parks at 300 x 528 (launch_p8h): 2 x 5 tiles x (16 parts + 4 group sums) x 256 x 128 floats
P8_PARK_BYTES = 2 * 5 * (P8_PARTS + 4) * 256 * 128 * 4


class User:
    """One workspace user: a committed case (dense Run or grouped GRun), launched under an ao_gemm8_* override if `forced`."""

    def __init__(self, name, case, sig=None, forced=None):
        self.name, self.case, self.sig, self.forced = name, case, sig, forced
        self.grouped = isinstance(case, rc.GCase)

    def run(self, seed, dev):
        return (GRun if self.grouped else Run)(self.case, seed, dev)

    def buffers(self, run, sentinel=None):
        bufs = run.buffers() if self.grouped else [_parity.Guarded(self.case.M, self.case.N, run.out_dtype, run.dev)]
        if sentinel is not None:
            for b in bufs:
                b.poison(sentinel)
        return bufs

    def rows(self, run):
        return run.written if self.grouped else self.case.M

    def route(self, lib):
        if self.forced:  # the route query answers for the product dispatch; the forced form's tile and parts are the override's
            return {"rows": 256, "cols": 128, "parts": P8_PARTS}
        return rc.grouped_route_of(lib, self.case) if self.grouped else rc.route_of(lib, self.case)

    def launch(self, run, bufs, sync=True):
        lib = _lib.lib()
        try:
            if self.forced:
                lib.ao_gemm8_set_variant(self.forced[0])
                lib.ao_gemm8_set_tuning(*self.forced[1])
            run.launch(bufs if self.grouped else bufs[0], sync=sync)
        finally:
            if self.forced:
                lib.ao_gemm8_set_variant(0)
                lib.ao_gemm8_set_tuning(self.forced[1][0], 0)

    def check(self, run, bufs, lib):
        route = self.route(lib)
        if self.grouped:
            run.check(bufs, route)
        else:
            _parity.check(bufs[0], route=route, **run.ref)


def _dense(name, sig, M, N, K):
    """The smallest committed case of a signature; the shape is stated so that a moved band shows here, not as a silent other case."""
    case = min((c for c, s in rc.CASES if s == sig), key=rc.cost)
    assert (case.M, case.N, case.K) == (M, N, K), (sig, tuple(case))
    return User(name, case, sig)


def _stream_cases():
    return [(c, s) for c, s in sorted(rc.GROUPED_CASES, key=lambda cs: rc.grouped_cost(cs[0])) if "/mx_stream/" in s]


def _cut_stream_case():
    """The cheapest mx_stream case whose shares cut a tile (route_cases.stream_partition): the cheapest case of all runs one share,
    which asks for the workspace but never meets in it."""
    lib = _lib.lib()  # the route query is host-only
    for c, s in _stream_cases():
        raw = rc.grouped_route_of(lib, c)["raw"]
        if rc.stream_partition(raw, c.N, c.K, rc.group_sizes(c.E, c.M, c.offs), c.entry in rc.PAIRS)[1] >= 2:
            return User("mx_stream_cut", c, s)
    raise AssertionError("no committed mx_stream case cuts a tile")


# neighbours in this list are different kernels with different ticket layouts (the ten-stream test cycles it)
USERS = [
    _dense("mid8_int8", "gemm8/int8_scaled/mid8/mt2/kparts", 17, 48, 4096),
    _dense("int4_rb", "int4/g128/rb/w4/nt1/mt2/kparts", 17, 48, 4096),
    _dense("mid8_fp8", "gemm8/fp8_scaled/mid8/mt2/kparts", 17, 48, 4096),
    User("mx_stream", *_stream_cases()[0]),
    _dense("mid8_dyn", "gemm8/fp8_dyn/mid8/mt2/kparts", 17, 48, 4096),  # its cast codes and scales live behind the parts
    _dense("int4_w32", "int4/g128/w32/cg1/prod/kparts", 129, 48, 4096),
    _dense("rb8", "gemm8/fp8_scaled/rb8/64x32/kparts", 33, 48, 4096),
    _cut_stream_case(),
    # gemm8_p8h_kernel with 16 K parts, as test_8bit_gpu.test_gemm8_p8_split_k_every_part_count forces it
    User("p8_forced", rc.Case("gemm8", "fp8_scaled", 300, 528, 2048, 0, True, True), forced=(33, (7, P8_PARTS))),
]
BY_NAME = {u.name: u for u in USERS}
SMALL = BY_NAME["mid8_fp8"]
# what owners launch to take or keep a slot: the split-K case the parity tests put between their two launches
BETWEEN = User("between", _SPLIT["gemm8"], dict(rc.CASES)[_SPLIT["gemm8"]])
_SEED_ORDER = [u.name for u in USERS] + [BETWEEN.name]

_SOLO = {}
_CYCLES_PER_MS = None


def _solo(user, dev, seed=0):
    """(run, solo bits per output) of a case: one launch alone on the default stream, held to float64.  Computed once and shared."""
    key = (user.name, seed)
    if key not in _SOLO:
        lib = _lib.lib()
        if user.sig is not None:
            assert user.route(lib)["sig"] == user.sig, (user.name, user.route(lib)["sig"])
        run = user.run(4000 + 16 * _SEED_ORDER.index(user.name) + seed, dev)
        bufs = user.buffers(run)
        torch.cuda.synchronize()
        user.launch(run, bufs)
        user.check(run, bufs, lib)
        _SOLO[key] = (run, [b.bits().clone() for b in bufs])
    return _SOLO[key]


def _assert_solo_bits(user, run, bufs, want, stream_index, what):
    """Clean guards, the written rows equal to the solo bits, the rows past them (grouped: past offs[-1]) still poisoned."""
    rows = user.rows(run)
    for i, (b, w) in enumerate(zip(bufs, want)):
        where = "%s on stream %d, %s, output %d" % (user.name, stream_index, what, i)
        assert not b.guard_problems(), "%s: %s" % (where, "; ".join(b.guard_problems()))
        same = b.bits()[:rows] == w[:rows]
        if not bool(same.all()):
            r, c = (int(v) for v in torch.nonzero(~same)[0])
            raise AssertionError("%s: %d elements differ from the solo launch, first at row %d, column %d%s"
                                 % (where, int((~same).sum()), r, c, _parity.locate(r, c, user.route(_lib.lib()))))
        assert not bool((b.bits()[rows:] != b.sentinel).any()), "%s: wrote rows past %d" % (where, rows)


def _query(stream):
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.lib().ao_splitk_query(ctypes.c_void_p(stream.cuda_stream), out))
    return tuple(out)


def _reserve(stream, nbytes):
    _lib.check(_lib.lib().ao_splitk_reserve(ctypes.c_void_p(stream.cuda_stream), nbytes))


def _launch_checked(user, dev, stream, index, what, seed=0):
    """One launch on `stream` into fresh poisoned buffers, a stream synchronise, the solo bits."""
    run, want = _solo(user, dev, seed)
    with torch.cuda.stream(stream):
        bufs = user.buffers(run)
        user.launch(run, bufs, sync=False)
    stream.synchronize()
    _assert_solo_bits(user, run, bufs, want, index, what)


def _hold(stream, ms):
    """Keep `stream` busy for about `ms` with torch's bounded spin kernel, so that what the host queues behind it is all in the queue
    before any of it starts (the spin counts clock ticks: calibrated once against events)."""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)  # the spin kernel's first launch loads it
        a.record()
        torch.cuda._sleep(1000000)
        b.record()
        b.synchronize()
        _CYCLES_PER_MS = 1000000 / max(a.elapsed_time(b), 1e-3)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(_CYCLES_PER_MS * ms))


def _gate(streams, ms=2.0):
    """All of `streams` start what is queued behind the gate at the same moment: the first spins, the others wait for its event."""
    _hold(streams[0], ms)
    ev = torch.cuda.Event()
    ev.record(streams[0])
    for s in streams[1:]:
        s.wait_event(ev)


def _hand_over_a_minimum_slot(target, others, dev):
    """Make `target` a stream without a slot whose next request takes over a slot of exactly 8 MiB: the 8 `others` launch (they are then
    the 8 owners, whatever the table held), and all but one 8 MiB owner launch again, which leaves that one least recently used.
    -> that owner's (held, capacity, base, retired)."""
    assert len(others) == SLOTS and target not in others
    for i, s in enumerate(others):
        _launch_checked(BETWEEN, dev, s, i, "taking a slot")
    assert _query(target)[0] == 0, "a stream still holds a slot after %d others launched" % SLOTS
    held = [_query(s) for s in others]
    assert all(q[0] for q in held) and len({q[2] for q in held}) == SLOTS, held
    k = next((i for i, q in enumerate(held) if q[1] == MIN_BYTES), None)
    assert k is not None, "every slot of the table has been grown past 8 MiB: %r" % ([q[1] // MIB for q in held],)
    for i, s in enumerate(others):
        if i != k:
            _launch_checked(BETWEEN, dev, s, i, "staying ahead in the eviction order")
    return held[k]


@pytest.fixture(scope="module")
def ws():
    """(library, device, 12 distinct streams).  The launches take the product dispatch unless a case forces a form around its own
    launch: no override may be set when the module starts, and none is left when it ends."""
    lib = _lib.lib()
    assert not lib.ao_gemm8_overridden() and not lib.ao_int4_overridden(), "an earlier test left an ao_gemm8_* / ao_int4_set_tuning override set"
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(12)]
    assert len({s.cuda_stream for s in streams}) == 12 and all(s.cuda_stream for s in streams)
    try:
        yield lib, dev, streams
    finally:
        torch.cuda.synchronize()
        assert not lib.ao_gemm8_overridden() and not lib.ao_int4_overridden()


@pytest.mark.gpu
def test_growth_retires_the_old_buffer_under_a_captured_graph(ws):
    """A graph captured at 8 MiB keeps replaying into the retired buffer after the forced 16-part p8h launch (6 553 600 parked floats:
    the route does not clamp the forced split, so no ao_splitk_reserve is needed to grow) moved the stream to a 32 MiB buffer; replay,
    eager launch (new buffer) and replay again run back to back on the stream without a host wait."""
    lib, dev, S = ws
    s, big = S[8], BY_NAME["p8_forced"]
    run, want = _solo(SMALL, dev)
    brun, bwant = _solo(big, dev)
    _hand_over_a_minimum_slot(s, S[:8], dev)
    _launch_checked(SMALL, dev, s, 8, "first launch")
    q0 = _query(s)
    assert q0[0] == 1 and q0[1] == MIN_BYTES, q0
    gbuf, snap, eager = SMALL.buffers(run), SMALL.buffers(run), SMALL.buffers(run)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        SMALL.launch(run, gbuf, sync=False)
    with torch.cuda.stream(s):
        graph.replay()
    s.synchronize()
    _assert_solo_bits(SMALL, run, gbuf, want, 8, "graph replay before the growth")
    assert _query(s) == q0

    with torch.cuda.stream(s):
        bbuf = big.buffers(brun)
        big.launch(brun, bbuf, sync=False)
    s.synchronize()
    q1 = _query(s)
    print("growth: %d -> %d MiB, retired %d -> %d" % (q0[1] // MIB, q1[1] // MIB, q0[3], q1[3]))
    assert q1[0] == 1 and q1[1] > q0[1] and q1[1] >= P8_PARK_BYTES and q1[2] != q0[2] and q1[3] == q0[3] + 1, (q0, q1)
    big.check(brun, bbuf, lib)
    _assert_solo_bits(big, brun, bbuf, bwant, 8, "the launch that grew the workspace")

    with torch.cuda.stream(s):
        for b in gbuf:
            b.poison(_parity.SENTINEL2)
        graph.replay()  # the retired buffer
        for a, b in zip(snap, gbuf):
            a.raw.copy_(b.raw)
            a.sentinel = b.sentinel
            b.poison()
        SMALL.launch(run, eager, sync=False)  # the new buffer
        graph.replay()
    s.synchronize()
    _assert_solo_bits(SMALL, run, snap, want, 8, "graph replay into the retired buffer")
    _assert_solo_bits(SMALL, run, eager, want, 8, "eager launch after the growth")
    _assert_solo_bits(SMALL, run, gbuf, want, 8, "second graph replay after the growth")
    assert _query(s) == q1


@pytest.mark.gpu
def test_reserve_sizes_the_slot_and_makes_a_cold_shape_capturable(ws):
    """ao_splitk_reserve rounds to powers of two from 8 MiB, never shrinks, caps at 128 MiB; after it a split-K case that never ran on
    the stream (its kernel has, on the default stream, so its LDS attribute is set) is captured without a warm-up and replays to the
    solo bits.  One stream only: slots are never freed."""
    lib, dev, S = ws
    s, user = S[9], BY_NAME["int4_w32"]
    run, want = _solo(user, dev)
    _hand_over_a_minimum_slot(s, S[:8], dev)
    _reserve(s, 8 * MIB + 4)
    q = _query(s)
    assert q[0] == 1 and q[1] == 16 * MIB, q
    _reserve(s, MIB)
    assert _query(s) == q
    _reserve(s, 0)
    qc = _query(s)
    assert qc[0] == 1 and qc[1] == CAP_BYTES and qc[2] != q[2] and qc[3] == q[3] + 1, (q, qc)
    _reserve(s, CAP_BYTES + 4096)
    assert _query(s) == qc

    b1, b2 = user.buffers(run), user.buffers(run, _parity.SENTINEL2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        user.launch(run, b1, sync=False)
        user.launch(run, b2, sync=False)
    for rep, sentinels in enumerate(((None, _parity.SENTINEL2), (_parity.SENTINEL2, None))):
        with torch.cuda.stream(s):
            if rep:
                for bufs, sent in zip((b1, b2), sentinels):
                    for b in bufs:
                        b.poison(sent)
            graph.replay()
        s.synchronize()
        _assert_solo_bits(user, run, b1, want, 9, "replay %d of a graph captured cold, first buffer" % rep)
        _assert_solo_bits(user, run, b2, want, 9, "replay %d of a graph captured cold, second buffer" % rep)
    assert _query(s) == qc


def _run_rounds(dev, streams, users, seeds, rounds, per_round):
    """`rounds` times: behind one gate, `per_round` unsynchronised launches per stream alternating its two buffers, no host wait between
    the streams, one device synchronise, then every buffer against its solo bits.  Each buffer is written per_round / 2 times a round
    and only its last write is compared: an earlier launch that went wrong shows through the tickets or parts it leaves to the later
    ones (a ticket left above zero keeps every later launch of that tile from storing), not through its own output."""
    pairs, solos = [], []
    for u, seed in zip(users, seeds):
        run, want = _solo(u, dev, seed)
        solos.append((run, want))
        pairs.append((u.buffers(run), u.buffers(run, _parity.SENTINEL2)))
    torch.cuda.synchronize()
    for i, (s, u) in enumerate(zip(streams, users)):
        _launch_checked(u, dev, s, i, "warm-up", seeds[i])
    bases = [_query(s) for s in streams]
    assert all(q[0] for q in bases) and len({q[2] for q in bases}) == len(streams), "the streams do not hold distinct workspaces: %r" % (bases,)
    t0 = time.perf_counter()
    for rnd in range(rounds):
        _gate(streams)
        for s, u, (run, _), pair in zip(streams, users, solos, pairs):
            with torch.cuda.stream(s):
                for k, bufs in enumerate(pair):
                    for b in bufs:
                        b.poison(_parity.SENTINEL2 if (rnd + k) & 1 else None)
                for j in range(per_round):
                    u.launch(run, pair[j & 1], sync=False)
        torch.cuda.synchronize()
        for i, (u, (run, want), pair) in enumerate(zip(users, solos, pairs)):
            for k, bufs in enumerate(pair):
                _assert_solo_bits(u, run, bufs, want, i, "round %d, buffer %d" % (rnd, k))
    print("%d rounds of %d x %d launches (%s): %.1f ms, the gate's spin at %.0f ticks per ms"
          % (rounds, len(streams), per_round, ", ".join(u.name for u in users), 1e3 * (time.perf_counter() - t0), _CYCLES_PER_MS))
    assert [_query(s) for s in streams] == bases


@pytest.mark.gpu
@pytest.mark.parametrize("same_case", (False, True), ids=("four_families", "one_case_four_seeds"))
def test_streams_do_not_share_a_workspace(ws, same_case):
    """Four streams (GPU_MAX_HW_QUEUES hardware queues: more would serialise) launch at once, each round behind a device-side gate so
    that all 32 launches are queued before the first starts: (a) four kernel families, (b) one case under four seeds, whose tile and
    ticket indices coincide -- the worst case if two streams shared a slot.

    That the streams really overlap at these shapes, so that the test can fail, was settled by two mutations (not committed; this file
    as committed, each run once in a process of its own on an MI355X, outputs in profiles/pytest_gpu_splitk_workspace.log).  A library
    whose slot lookup ignores the stream fails the distinct-bases assertion after the warm-ups (three of the four streams hold
    nothing).  A library whose table and query stay as they are but whose splitk_workspace hands every request slot 0's memory gets
    past that assertion and fails both forms in round 0, all 816 elements of mid8_dyn on stream 0 differing from the solo launch."""
    lib, dev, S = ws
    if same_case:
        users, seeds = [BY_NAME["mid8_dyn"]] * 4, [1, 2, 3, 4]
    else:
        users, seeds = [BY_NAME[n] for n in ("mid8_dyn", "rb8", "int4_w32", "mx_stream_cut")], [0, 0, 0, 0]
    _run_rounds(dev, S[:4], users, seeds, ROUNDS, PER_ROUND)


@pytest.mark.gpu
def test_a_ninth_stream_evicts_and_every_owner_still_gets_its_bits(ws):
    """Ten streams over eight slots, neighbours on different kernels: in order, in order again, reversed; every launch its solo bits.
    After the first pass exactly 8 of the ten hold a slot (each launch makes its stream the most recent owner, so the last 8 are in,
    whatever the table held before); after every later launch the stream just used holds one."""
    lib, dev, S = ws
    ten = S[:10]
    users = [USERS[i % len(USERS)] for i in range(10)]
    for u in USERS:  # the solo launches run on the default stream, which takes a slot for them: all of them before the count starts
        _solo(u, dev)
    for i, (s, u) in enumerate(zip(ten, users)):
        _launch_checked(u, dev, s, i, "pass 1")
    held = [_query(s)[0] for s in ten]
    assert sum(held) == SLOTS, held
    for what, order in (("pass 2", range(10)), ("pass 3", reversed(range(10)))):
        for i in order:
            _launch_checked(users[i], dev, ten[i], i, what)
            assert _query(ten[i])[0] == 1, (what, i)
    assert sum(_query(s)[0] for s in S) == SLOTS


@pytest.mark.gpu
def test_eviction_waits_for_the_evicted_streams_work(ws):
    """Stream A queues 16 unsynchronised launches behind a 2 ms hold; its seven fellow owners then launch (no eviction: A becomes the
    least recently used) and a ninth stream C asks for a slot: A's slot changes owner, at A's base, while A's launches are still
    queued.  C waits on an event recorded on A right after the hold, so without the device synchronise inside the eviction C's 8
    kernels (the same case, other operands: the same tiles and tickets) would start in A's buffer together with A's 16; with it the
    event has long fired when C's first kernel is queued.
    Settled the same way (profiles/pytest_gpu_splitk_workspace.log): against a library whose eviction does not synchronise, this test,
    run once on an MI355X, failed with all 816 elements of C's first launch differing from the solo launch."""
    lib, dev, S = ws
    A, B, C = S[8], S[:7], S[9]
    user = BY_NAME["mid8_dyn"]
    run, want = _solo(user, dev, 1)
    crun, cwant = _solo(user, dev, 2)
    srun, swant = _solo(SMALL, dev)
    _launch_checked(user, dev, A, 8, "taking a slot", 1)
    for i, s in enumerate(B):
        _launch_checked(SMALL, dev, s, i, "taking a slot")
    qa = _query(A)
    assert qa[0] == 1 and all(_query(s)[0] for s in B) and _query(C)[0] == 0, "A and its seven fellows are not the owners"
    abufs = [user.buffers(run, _parity.SENTINEL2 if j & 1 else None) for j in range(16)]
    bbufs = [SMALL.buffers(srun) for _ in B]
    cbufs = [user.buffers(crun, _parity.SENTINEL2 if j & 1 else None) for j in range(8)]
    torch.cuda.synchronize()
    _hold(A, 2.0)
    released = torch.cuda.Event()
    released.record(A)
    C.wait_event(released)  # C's kernels may start when A's queued launches do, not before
    with torch.cuda.stream(A):
        for bufs in abufs:
            user.launch(run, bufs, sync=False)
    for s, bufs in zip(B, bbufs):
        with torch.cuda.stream(s):
            SMALL.launch(srun, bufs, sync=False)
    with torch.cuda.stream(C):
        for bufs in cbufs:  # the first of them evicts A
            user.launch(crun, bufs, sync=False)
    qa1, qc = _query(A), _query(C)
    assert qa1[0] == 0 and qc[0] == 1 and qc[2] == qa[2], (qa, qa1, qc)
    torch.cuda.synchronize()
    for j, bufs in enumerate(abufs):
        _assert_solo_bits(user, run, bufs, want, 8, "launch %d queued before the eviction" % j)
    for i, bufs in enumerate(bbufs):
        _assert_solo_bits(SMALL, srun, bufs, swant, i, "a fellow owner's launch")
    for j, bufs in enumerate(cbufs):
        _assert_solo_bits(user, crun, bufs, cwant, 9, "the new owner's launch %d" % j)
    _launch_checked(user, dev, A, 8, "back after the eviction", 1)
    assert _query(A)[0] == 1


@pytest.mark.gpu
def test_host_threads_on_their_own_streams(ws):
    """Four host threads, each on its own stream with its own case and buffers, 25 launches each, synchronised on the thread's stream:
    ctypes releases the GIL, so splitk_workspace is entered concurrently.  The main thread makes the four streams the most recent
    owners first, so no eviction can happen while the threads run (the library hands out a slot before the caller launches)."""
    lib, dev, S = ws
    streams = S[:4]
    users = [BY_NAME[n] for n in ("int4_rb", "mid8_int8", "mx_stream_cut", "rb8")]
    solos = [_solo(u, dev, 5 + i) for i, u in enumerate(users)]
    pairs = [(u.buffers(run), u.buffers(run, _parity.SENTINEL2)) for u, (run, _) in zip(users, solos)]
    for i, (s, u) in enumerate(zip(streams, users)):
        _launch_checked(u, dev, s, i, "warm-up", 5 + i)
    bases = [_query(s) for s in streams]
    assert all(q[0] for q in bases) and len({q[2] for q in bases}) == 4, bases
    torch.cuda.synchronize()
    errors = [None] * 4

    def body(i):
        try:
            torch.cuda.set_device(dev)
            u, (run, want), s = users[i], solos[i], streams[i]
            with torch.cuda.stream(s):
                for j in range(PER_THREAD):
                    bufs = pairs[i][j & 1]
                    for b in bufs:
                        b.poison(_parity.SENTINEL2 if j & 2 else None)
                    u.launch(run, bufs, sync=False)
                    s.synchronize()
                    _assert_solo_bits(u, run, bufs, want, i, "launch %d of its thread" % j)
        except BaseException as e:  # noqa: BLE001 -- re-raised by the main thread
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads), "a launching thread did not finish"
    for e in errors:
        if e is not None:
            raise e
    torch.cuda.synchronize()
    assert [_query(s) for s in streams] == bases
