"""Twin int4 linears in one launch: int4_mm_pair_kernel runs, per workgroup, exactly what int4_mm_kernel runs for one row on
one of two problems, so every check here is an equality of bytes against two single launches.  The pair is reached two ways: the public
entry ao_int4_weight_int4pack_mm_pair, and ao_int4_weight_int4pack_mm under stream capture, which folds a call into the kernel node of the
call before it when the capture has seen nothing in between and the two problems are independent (ao_int4_pair_fusions counts).

K = 1792 (14 k-blocks) is kept as a case of its own: the route takes it as 7 waves x 2 blocks, a straight-line form, so it runs the pair
kernel; K = 1664 (13 k-blocks, a prime) and M = 4 are the cases no straight-line form takes and that go through the two single launches."""
import ctypes
import functools

import pytest
import torch

from ao_amd import _lib

pytestmark = pytest.mark.gpu

NEVER, HALVES = 985, 986  # ao_int4_set_tuning: never fuse / the pair grid with each problem's balanced halves (product: one workgroup per tile)
# (N, K): the smallest 4-deep form (4 waves); 384 tiles, the balanced halves live on 256 CUs; 16 waves x 7; then at N = 32 one K per depth
# 2 (8 k-blocks), 8 (80), 9 (108), 14 (126), and 14 k-blocks = 7 waves x 2
STRAIGHT = [(64, 2048, 4), (6144, 4096, 4), (32, 14336, 7), (32, 1024, 2), (32, 10240, 8), (32, 13824, 9), (32, 16128, 14), (32, 1792, 2)]
GROUPS = (32, 128)


def _route(lib, m, n, k, g):
    out = (ctypes.c_int32 * 11)()
    assert lib.ao_int4_mm_route(m, n, k, g, out, 11) == 0
    return list(out)


@functools.lru_cache(maxsize=None)
def _weight(n, k, g, seed):
    from ao_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16, generator=gen) * 0.02
    return ops.int4_quantize_tinygemm(w, g)


def _x(m, k, seed):
    gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
    return torch.randn(m, k, device="cuda", dtype=torch.bfloat16, generator=gen)


def _single(x, w, g):
    """One eager launch (eager launches never fuse)."""
    from ao_amd import ops

    y = ops.weight_int4pack_mm(x, w[0], g, w[1])
    torch.cuda.synchronize()
    return y


def _raw(lib, x, w, y, g):
    """ao_int4_weight_int4pack_mm on the current stream into a buffer the test owns (y: a flat bf16 view of M N elements)."""
    n, k = w[0].shape[0] * 8, w[0].shape[1] * 128
    m = x.numel() // k
    assert y.numel() == m * n
    _lib.check(lib.ao_int4_weight_int4pack_mm(x.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), y.data_ptr(), m, n, k, g,
                                              torch.cuda.current_stream().cuda_stream))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _captured(body):
    """Capture body() on a side stream; returns (graph, stream, fusions counted during the capture)."""
    lib = _lib.lib()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        before = lib.ao_int4_pair_fusions()
        with torch.cuda.graph(graph, stream=stream):
            body()
        fused = lib.ao_int4_pair_fusions() - before
    return graph, stream, fused


def _replay(graph, stream):
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()


# ---- the public entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("n,k,depth", STRAIGHT)
@pytest.mark.parametrize("same_x", [True, False])
def test_pair_entry_equals_two_single_calls(n, k, depth, g, same_x):
    from ao_amd import ops

    lib = _lib.lib()
    r = _route(lib, 1, n, k, g)
    assert r[0] == 0 and r[1] == 1 and r[3] == 1 and r[2] == depth, r  # a one-row straight-line form of the depth the case is named for
    if (n, k) == (6144, 4096) and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert r[10] == 128, "the balanced halves are live on this shape"
    w0, w1 = _weight(n, k, g, 1), _weight(n, k, g, 2)
    x0 = _x(1, k, 0)
    x1 = x0 if same_x else _x(1, k, 1)
    want0, want1 = _bits(_single(x0, w0, g)), _bits(_single(x1, w1, g))
    for mode in (0, HALVES):
        lib.ao_int4_set_tuning(0, mode)
        try:
            y0, y1 = ops.int4_mm_pair(x0, w0[0], w0[1], x1, w1[0], w1[1], g)
            torch.cuda.synchronize()
        finally:
            lib.ao_int4_set_tuning(0, 0)
        assert torch.equal(_bits(y0), want0), f"mode {mode}: {int((_bits(y0) != want0).sum())} of {n} outputs of problem 0 differ"
        assert torch.equal(_bits(y1), want1), f"mode {mode}: {int((_bits(y1) != want1).sum())} of {n} outputs of problem 1 differ"
    if r[10] > 0:  # the halves' meeting: a race shows as a launch that differs from the first
        lib.ao_int4_set_tuning(0, HALVES)
        try:
            for i in range(10):
                y0, y1 = ops.int4_mm_pair(x0, w0[0], w0[1], x1, w1[0], w1[1], g)
                torch.cuda.synchronize()
                assert torch.equal(_bits(y0), want0) and torch.equal(_bits(y1), want1), f"launch {i + 2}"
        finally:
            lib.ao_int4_set_tuning(0, 0)


@pytest.mark.parametrize("m,n,k", [(1, 32, 1664), (4, 64, 2048)])
def test_pair_entry_falls_back_where_the_route_is_not_straight_line(m, n, k):
    from ao_amd import ops

    lib = _lib.lib()
    r = _route(lib, m, n, k, 128)
    assert not (r[1] == 1 and r[3] == 1), r
    w0, w1 = _weight(n, k, 128, 1), _weight(n, k, 128, 2)
    x = _x(m, k, 0)
    y0, y1 = ops.int4_mm_pair(x, w0[0], w0[1], x, w1[0], w1[1], 128)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y0), _bits(_single(x, w0, 128))) and torch.equal(_bits(y1), _bits(_single(x, w1, 128)))


def test_pair_entry_runs_a_dependent_second_problem_after_the_first():
    lib = _lib.lib()
    n = k = 2048
    w0, w1 = _weight(n, k, 128, 1), _weight(n, k, 128, 2)
    x = _x(1, k, 0)
    mid = _single(x, w0, 128)
    want = _bits(_single(mid, w1, 128))
    y0, y1 = torch.zeros(1, n, device="cuda", dtype=torch.bfloat16), torch.zeros(1, n, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.ao_int4_weight_int4pack_mm_pair(x.data_ptr(), w0[0].data_ptr(), w0[1].data_ptr(), y0.data_ptr(), y0.data_ptr(), w1[0].data_ptr(),
                                                   w1[1].data_ptr(), y1.data_ptr(), 1, n, k, 128, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(_bits(y0), _bits(mid)) and torch.equal(_bits(y1), want)


# ---- capture: the fusing case ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(64, 2048), (6144, 4096), (32, 14336)])
def test_two_adjacent_twins_fuse_and_replay_reads_pointers(n, k):
    from ao_amd import ops

    g = 128
    w0, w1 = _weight(n, k, g, 1), _weight(n, k, g, 2)
    x = _x(1, k, 0).clone()
    want0, want1 = _bits(_single(x, w0, g)), _bits(_single(x, w1, g))
    out = {}

    def body():
        out["y0"] = ops.weight_int4pack_mm(x, w0[0], g, w0[1])
        out["y1"] = ops.weight_int4pack_mm(x, w1[0], g, w1[1])

    graph, stream, fused = _captured_after_warmup(body, x, (w0, w1), g)
    assert fused == 1
    for i in range(3):  # (the halves' tickets are left ready for the next replay)
        out["y0"].zero_()
        out["y1"].zero_()
        torch.cuda.synchronize()
        _replay(graph, stream)
        assert torch.equal(_bits(out["y0"]), want0) and torch.equal(_bits(out["y1"]), want1), f"replay {i + 1}"
    x.copy_(_x(1, k, 7))
    torch.cuda.synchronize()
    _replay(graph, stream)
    assert torch.equal(_bits(out["y0"]), _bits(_single(x, w0, g))) and torch.equal(_bits(out["y1"]), _bits(_single(x, w1, g)))
    assert not torch.equal(_bits(out["y0"]), want0)


def _captured_after_warmup(body, x, weights, g):
    """The split-K workspace of a stream is allocated outside capture: one eager call per weight on the capture's stream first."""
    from ao_amd import ops

    lib = _lib.lib()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        for w in weights:
            ops.weight_int4pack_mm(x, w[0], g, w[1])
        stream.synchronize()
        before = lib.ao_int4_pair_fusions()
        with torch.cuda.graph(graph, stream=stream):
            body()
        fused = lib.ao_int4_pair_fusions() - before
    return graph, stream, fused


# ---- capture: the cases that must not fuse ----------------------------------------------------------------------------------------------
def _buffers(*sizes):
    return [torch.zeros(s, device="cuda", dtype=torch.bfloat16) for s in sizes]


def test_true_dependency_is_not_fused():
    lib = _lib.lib()
    n = k = 2048
    w0, w1 = _weight(n, k, 128, 1), _weight(n, k, 128, 2)
    x = _x(1, k, 0)
    mid = _single(x, w0, 128)
    want = _bits(_single(mid, w1, 128))
    y0, y1 = _buffers(n, n)

    def body():
        _raw(lib, x, w0, y0, 128)
        _raw(lib, y0, w1, y1, 128)  # x1 aliases y0

    graph, stream, fused = _captured(body)
    assert fused == 0
    _replay(graph, stream)
    assert torch.equal(_bits(y0), _bits(mid).view(-1)) and torch.equal(_bits(y1), want.view(-1)), "the second result reflects the first"


def test_overlapping_outputs_are_not_fused():
    lib = _lib.lib()
    n, k = 64, 2048
    w0, w1 = _weight(n, k, 128, 1), _weight(n, k, 128, 2)
    x = _x(1, k, 0)
    a, b = _bits(_single(x, w0, 128)).view(-1), _bits(_single(x, w1, 128)).view(-1)
    (buf,) = _buffers(n + n // 2)

    def body():
        _raw(lib, x, w0, buf[:n], 128)
        _raw(lib, x, w1, buf[n // 2:], 128)  # y1 starts inside y0: sequential execution leaves y0's first half and all of y1

    graph, stream, fused = _captured(body)
    assert fused == 0
    _replay(graph, stream)
    assert torch.equal(_bits(buf)[: n // 2], a[: n // 2]) and torch.equal(_bits(buf)[n // 2:], b)


@pytest.mark.parametrize("what", ["n", "g", "m", "op_between", "other_stream", "never"])
def test_calls_that_are_not_adjacent_twins_are_not_fused(what):
    lib = _lib.lib()
    n, k, g = 64, 2048, 128
    m = 4 if what == "m" else 1
    n1 = 128 if what == "n" else n
    g1 = 32 if what == "g" else g
    w0, w1 = _weight(n, k, g, 1), _weight(n1, k, g1, 2)
    x = _x(m, k, 0)
    want0, want1 = _bits(_single(x, w0, g)).view(-1), _bits(_single(x, w1, g1)).view(-1)
    y0, y1, t = _buffers(m * n, m * n1, m * n)
    side = torch.cuda.Stream()

    def body():
        _raw(lib, x, w0, y0, g)
        if what == "op_between":
            torch.mul(y0, 2.0, out=t)
        if what == "other_stream":
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                _raw(lib, x, w1, y1, g1)
            torch.cuda.current_stream().wait_stream(side)
        else:
            _raw(lib, x, w1, y1, g1)

    lib.ao_int4_set_tuning(0, NEVER if what == "never" else 0)
    try:
        graph, stream, fused = _captured(body)
    finally:
        lib.ao_int4_set_tuning(0, 0)
    assert fused == 0
    _replay(graph, stream)
    assert torch.equal(_bits(y0), want0) and torch.equal(_bits(y1), want1)
    if what == "op_between":
        assert torch.equal(t, y0 * 2.0)


@pytest.mark.parametrize("twins,fusions", [(3, 1), (4, 2)])
def test_a_pair_takes_no_third(twins, fusions):
    lib = _lib.lib()
    n, k, g = 64, 2048, 128
    ws = [_weight(n, k, g, 1 + i) for i in range(twins)]
    x = _x(1, k, 0)
    want = [_bits(_single(x, w, g)).view(-1) for w in ws]
    ys = _buffers(*([n] * twins))

    def body():
        for w, y in zip(ws, ys):
            _raw(lib, x, w, y, g)

    graph, stream, fused = _captured(body)
    assert fused == fusions
    _replay(graph, stream)
    for i in range(twins):
        assert torch.equal(_bits(ys[i]), want[i]), f"twin {i}"


def test_no_record_survives_its_capture():
    lib = _lib.lib()
    n, k, g = 64, 2048, 128
    w0, w1 = _weight(n, k, g, 1), _weight(n, k, g, 2)
    x = _x(1, k, 0)
    want0, want1 = _bits(_single(x, w0, g)).view(-1), _bits(_single(x, w1, g)).view(-1)
    y0, y1 = _buffers(n, n)
    first, s0, fused0 = _captured(lambda: _raw(lib, x, w0, y0, g))  # ends in an unpaired twin
    second, s1, fused1 = _captured(lambda: _raw(lib, x, w1, y1, g))  # its first call finds that record: another capture's
    assert fused0 == 0 and fused1 == 0
    _replay(second, s1)
    assert torch.equal(_bits(y1), want1) and not y0.any(), "the second graph holds its own launch and nothing of the first's"
    _replay(first, s0)
    assert torch.equal(_bits(y0), want0)
