"""Host-only half of the twin-linear pair: the independence rule on hand-written intervals, and the exports.  No GPU:
ao_int4_pair_independent is arithmetic on addresses and dereferences nothing."""
import ctypes

from ao_amd import _lib

BASE = 1 << 20  # any address: never dereferenced


def _ind(x0, y0, x1, y1, m=1, n=64, k=256):
    """Element offsets (bf16: 2 bytes) from BASE."""
    p = lambda e: ctypes.c_void_p(BASE + 2 * e)  # noqa: E731
    return _lib.lib().ao_int4_pair_independent(p(x0), p(y0), p(x1), p(y1), m, n, k)


def test_exports_and_abi_version():
    lib = _lib.lib()
    names = _lib.declared_symbols()
    for name in ("ao_int4_weight_int4pack_mm_pair", "ao_int4_pair_independent", "ao_int4_pair_fusions"):
        assert name in names and hasattr(lib, name) and name in _lib._SIGNATURES
    # the pair entry is an addition: every earlier export keeps its signature, so the ABI version stays the one tests/test_abi.py pins
    assert lib.ao_abi_version() == 2
    assert lib.ao_int4_pair_fusions() >= 0


def test_shared_activation_and_disjoint_outputs_are_independent():
    # x at 0 .. 256, y0 at 1000 .. 1064, y1 at 2000 .. 2064
    assert _ind(0, 1000, 0, 2000) == 1  # x0 == x1: the expected case
    assert _ind(0, 1000, 500, 2000) == 1  # distinct activations


def test_touching_intervals_are_independent():
    assert _ind(0, 1000, 0, 1064) == 1  # y1 begins where y0 ends
    assert _ind(0, 1000, 0, 936) == 1  # y1 ends where y0 begins
    assert _ind(0, 1000, 0, 256) == 1  # y1 begins where x0 ends
    assert _ind(64, 1000, 64, 0) == 1  # y1 ends where x0 begins
    assert _ind(0, 1000, 1064, 2000) == 1  # x1 begins where y0 ends
    assert _ind(0, 1000, 744, 2000) == 1  # x1 ends where y0 begins


def test_one_element_of_overlap_is_a_dependency():
    assert _ind(0, 1000, 0, 1063) == 0  # y1's first element is y0's last
    assert _ind(0, 1000, 0, 937) == 0  # y1's last element is y0's first
    assert _ind(0, 1000, 0, 1000) == 0  # the same output
    assert _ind(0, 1000, 0, 255) == 0  # y1's first element is x0's last
    assert _ind(64, 1000, 64, 1) == 0  # y1's last element is x0's first
    assert _ind(0, 1000, 1063, 2000) == 0  # x1's first element is y0's last
    assert _ind(0, 1000, 745, 2000) == 0  # x1's last element is y0's first
    assert _ind(0, 1000, 1000, 2000, n=256) == 0  # x1 is y0: the second linear consumes the first


def test_rows_scale_the_intervals():
    # M = 4: x spans 1024 elements, y 256
    assert _ind(0, 2000, 0, 2256, m=4) == 1 and _ind(0, 2000, 0, 2255, m=4) == 0
    assert _ind(0, 2000, 0, 1024, m=4) == 1 and _ind(0, 2000, 0, 1023, m=4) == 0
    assert _ind(0, 2000, 0, 3000, m=0) == 0  # nothing to pair


def test_never_fuse_is_a_tuning_mode_that_leaves_the_route_alone():
    lib = _lib.lib()
    out, ref = (ctypes.c_int32 * 11)(), (ctypes.c_int32 * 11)()
    assert lib.ao_int4_mm_route(1, 14336, 4096, 128, ref, 11) == 0
    for mode in (985, 986):
        lib.ao_int4_set_tuning(0, mode)
        try:
            assert lib.ao_int4_overridden() == 1
            assert lib.ao_int4_mm_route(1, 14336, 4096, 128, out, 11) == 0 and list(out) == list(ref)
        finally:
            lib.ao_int4_set_tuning(0, 0)
    assert lib.ao_int4_overridden() == 0
