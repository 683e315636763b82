"""The refusals of the K-sharded casts, the scale epilogues, the static / asymmetric casts, the row sums and the row copies (quant_kernels.hip,
moe_permute_kernels.hip), through the C ABI with null pointers: every shape check runs before a pointer is looked at and before a launch, so
none of this needs a GPU.  And the one refusal the Python wrapper of the row gather makes itself."""
import pytest
import torch

from ao_amd import _lib, ops

INV, OK = _lib.AO_ERR_INVALID_ARGUMENT, _lib.AO_OK


def refused(rc, reason):
    assert rc == INV, rc
    assert reason in _lib.last_error(), (reason, _lib.last_error())


def strided_entries():
    lib = _lib.lib()
    return [("ao_rowwise_amax", lambda M, K, ldx: lib.ao_rowwise_amax(None, ldx, None, M, K, None)),
            ("ao_int8_quantize_rowwise_amax", lambda M, K, ldx: lib.ao_int8_quantize_rowwise_amax(None, ldx, None, None, None, M, K, None)),
            ("ao_fp8_quantize_rowwise_amax", lambda M, K, ldx: lib.ao_fp8_quantize_rowwise_amax(None, ldx, None, None, None, M, K, None))]


def epilogue_entries():
    lib = _lib.lib()
    return [("ao_int8_scale_epilogue", lambda M, N: lib.ao_int8_scale_epilogue(None, None, None, None, None, M, N, None)),
            ("ao_fp8_scale_epilogue", lambda M, N: lib.ao_fp8_scale_epilogue(None, None, None, None, None, M, N, None)),
            ("ao_int8_scale_epilogue_asym", lambda M, N: lib.ao_int8_scale_epilogue_asym(None, None, None, None, None, None, None, M, N, None))]


@pytest.mark.parametrize("M,K,ldx,reason", [
    (4, 12, 16, "K=12 must be a multiple of 8"),
    (4, 0, 8, "bad shape M=4 K=0"),
    (-1, 64, 64, "bad shape M=-1 K=64"),
    (1 << 31, 64, 64, "M=2147483648 too large"),
    (4, 64, 56, "row stride 56 must be >= K=64"),
    (4, 64, 68, "row stride 68 must be >= K=64 and a multiple of 8"),
])
def test_the_k_sharded_casts_refuse_bad_rows_and_strides(M, K, ldx, reason):
    for name, call in strided_entries():
        refused(call(M, K, ldx), reason)
        assert _lib.last_error().startswith(name + ":")


@pytest.mark.parametrize("M,N", [(4, 0), (-1, 16), (65535 * 65535 + 1, 16)])
def test_the_scale_epilogues_refuse_bad_shapes(M, N):
    for name, call in epilogue_entries():
        refused(call(M, N), "%s: bad shape M=%d N=%d" % (name, M, N))


def test_the_row_sums_and_the_static_and_asymmetric_casts_refuse_bad_k():
    lib = _lib.lib()
    refused(lib.ao_int8_row_sums(None, None, 4, 24, None), "ao_int8_row_sums: K=24 must be a multiple of 16")
    refused(lib.ao_int8_row_sums(None, None, 4, (1 << 24) + 16, None), "ao_int8_row_sums: K=16777232 too large for an int32 row sum")
    refused(lib.ao_int8_quantize_static(None, None, None, 1, None, 4, 12, None), "ao_int8_quantize_static: K=12 must be a multiple of 8")
    refused(lib.ao_int8_quantize_rowwise_asym(None, None, None, None, 4, 12, None), "ao_int8_quantize_rowwise_asym: K=12 must be a multiple of 8")


def test_the_row_copies_refuse_empty_rows_and_negative_counts():
    lib = _lib.lib()
    for name in ("ao_moe_gather_rows", "ao_moe_scatter_rows"):
        fn = getattr(lib, name)
        refused(fn(None, None, None, 4, 4, 0, None), name + ": bad shape in=4 out=4 row_bytes=0")
        refused(fn(None, None, None, -1, 4, 16, None), name + ": bad shape in=-1 out=4 row_bytes=16")
        refused(fn(None, None, None, 4, -1, 16, None), name + ": bad shape in=4 out=-1 row_bytes=16")


def test_no_rows_is_no_launch_and_no_pointer_is_read():
    lib = _lib.lib()
    for _, call in strided_entries():
        assert call(0, 64, 64) == OK
    for _, call in epilogue_entries():
        assert call(0, 16) == OK
    assert lib.ao_int8_row_sums(None, None, 0, 32, None) == OK
    assert lib.ao_int8_quantize_static(None, None, None, 1, None, 0, 16, None) == OK
    assert lib.ao_int8_quantize_rowwise_asym(None, None, None, None, 0, 16, None) == OK
    assert lib.ao_moe_gather_rows(None, None, None, 4, 0, 16, None) == OK
    assert lib.ao_moe_scatter_rows(None, None, None, 4, 0, 16, None) == OK


def test_gather_rows_refuses_more_output_rows_than_indices():
    """The kernel reads one index per output row: num_out past the indices would read them past their end.  Refused from the shapes alone,
    before a device is asked for."""
    x, idx = torch.zeros((4, 8), dtype=torch.uint8), torch.zeros((5,), dtype=torch.int32)
    with pytest.raises(ValueError, match=r"num_out=6 must be in \[0, 5\]"):
        ops.gather_rows(x, idx, 6)
    with pytest.raises(ValueError, match=r"num_out=-1 must be in \[0, 5\]"):
        ops.gather_rows(x, idx, -1)
