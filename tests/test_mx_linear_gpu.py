"""MXFP4 / MXFP8 dense linears on the GPU: the fp4 cast against the reference's bytes, the GEMM against a float64 oracle at every route
seam, the fused cast against cast + GEMM, the fp4 operand lane map, quantize_ and torch.compile (tests/mx_linear_ref.py, fixture
tests/golden/mx_linear.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_linear_ref as R  # noqa: E402
from _parity import Guarded, check  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mx_linear.npz"))
FMTS = [(R.FMT_E2M1, "fp4"), (R.FMT_E4M3, "fp8")]
MODES = [("floor", 0), ("rceil", 1)]


def _dev():
    return torch.device("cuda", 0)


def _bf16(bits_np):
    return torch.from_numpy(bits_np.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16).to(_dev())


def _np(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _cast(x, fmt, mode):
    from ao_amd import ops

    q, s = ops.mx_quantize(x, fmt, mode)
    return q.view(torch.uint8), s.view(torch.uint8)


@pytest.mark.parametrize("mode_name,mode", MODES)
@pytest.mark.parametrize("name", ["seeded", "edge"])
def test_fp4_cast_matches_reference_bytes(name, mode_name, mode):
    q, s = _cast(_bf16(GOLDEN[f"{name}_x"]), R.FMT_E2M1, mode_name)
    np.testing.assert_array_equal(_np(q), GOLDEN[f"{name}_fp4_{mode_name}_q"])
    np.testing.assert_array_equal(_np(s), GOLDEN[f"{name}_fp4_{mode_name}_s"])


@pytest.mark.parametrize("mode_name,mode", MODES)
def test_fp4_cast_exhaustive(mode_name, mode):
    """Every finite bf16 value beside a fixed amax (several amax values) equals the oracle's bytes."""
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    finite = (allb & 0x7F80) != 0x7F80
    vals = allb[finite]
    pad = (-len(vals)) % 31
    vals = np.concatenate([vals, np.zeros(pad, dtype=np.uint16)]).reshape(-1, 31)
    for amax in (6.0, 1.0, 5.0, 6.0 * 2.0 ** 40, 3.0 * 2.0 ** -100, 2.0 ** 120):
        ab = (np.array([amax], dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
        x = np.concatenate([np.full((vals.shape[0], 1), ab[0], dtype=np.uint16), vals], axis=1)
        q, s = _cast(_bf16(x), R.FMT_E2M1, mode_name)
        rq, rs = R.to_mx4(x, mode)
        np.testing.assert_array_equal(_np(s), rs, err_msg=f"amax {amax}")
        np.testing.assert_array_equal(_np(q), rq, err_msg=f"amax {amax}")


def _operands(fmt, M, N, K, seed, bias):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    b = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16) if bias else None
    return x.to(_dev()), w.to(_dev()), (b.to(_dev()) if b is not None else None)


def _run_codes(fmt, aq, a_s, wq, ws, bias, M, N, K):
    from ao_amd import _lib

    buf = Guarded(M, N, torch.bfloat16, _dev())
    _lib.check(_lib.lib().ao_mx_linear(fmt, aq.data_ptr(), a_s.data_ptr(), wq.data_ptr(), ws.data_ptr(),
                                       bias.data_ptr() if bias is not None else None, buf.out.data_ptr(), M, N, K,
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf


def _run_fused(fmt, x, wq, ws, bias, M, N, K, mode):
    from ao_amd import _lib

    buf = Guarded(M, N, torch.bfloat16, _dev())
    _lib.check(_lib.lib().ao_mx_dynamic_linear(fmt, x.data_ptr(), wq.data_ptr(), ws.data_ptr(), bias.data_ptr() if bias is not None else None,
                                               buf.out.data_ptr(), M, N, K, mode, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf


def _ref(fmt, aq, a_s, wq, ws, bias):
    b = bias.view(torch.int16).cpu().numpy().view(np.uint16) if bias is not None else None
    y, mag = R.linear_f64(_np(aq), _np(a_s), _np(wq), _np(ws), fmt, b)
    return torch.from_numpy(y).to(_dev()), torch.from_numpy(mag).to(_dev())


# The scaled MFMA adds e4m3 products less exactly than an fp32 chain: at (300, 64, 32) three of 19 200 elements of a sum with heavy
# cancellation (terms up to 0.064 summing to -4.4e-4) missed ulp + 2 K 2^-24 S by a quarter of the bound; e2m1 products (3 bits of
# mantissa) meet it.  fp8 cases get 4 S.
_S_FACTOR = {R.FMT_E2M1: 1.0, R.FMT_E4M3: 4.0}
SEAMS = {R.FMT_E4M3: 64, R.FMT_E2M1: 32}  # include/ao_mi355.h: the streaming form up to these rows, tiled beyond
CASES = [(0, 17, 64), (1, 17, 32), (1, 64, 96), (15, 33, 128), (16, 48, 256), (17, 40, 96), (31, 17, 160), (32, 130, 256),
         (33, 17, 96), (63, 17, 160), (64, 130, 256), (65, 17, 96), (129, 257, 384), (300, 64, 32)]


@pytest.mark.parametrize("fmt,tag", FMTS)
@pytest.mark.parametrize("M,N,K", CASES)
def test_gemm_parity_at_route_seams(fmt, tag, M, N, K):
    from ao_amd import ops

    for bias_on in (False, True):
        x, w, bias = _operands(fmt, M, N, K, 100 + M + N + K, bias_on)
        aq, a_s = _cast(x, fmt, "rceil")
        wq, ws = _cast(w, fmt, "rceil")
        want = "mx_linear_stream_kernel" if M <= SEAMS[fmt] else "mx_linear_tile_kernel"
        assert ops.mx_linear_kernel_name(fmt, M, N, K) == want
        buf = _run_codes(fmt, aq, a_s, wq, ws, bias, M, N, K)
        if M == 0:
            continue
        ref64, S = _ref(fmt, aq, a_s, wq, ws, bias)
        check(buf, ref64=ref64, S=S * _S_FACTOR[fmt], K=K)


FUSED = [(fmt, tag, M, N, K) for fmt, tag in FMTS for M, N, K in ((1, 33, 96), (5, 64, 4096), (24, 48, 160), (SEAMS[fmt], 17, 32))]


@pytest.mark.parametrize("mode_name,mode", MODES)
@pytest.mark.parametrize("fmt,tag,M,N,K", FUSED)
def test_fused_cast_bitwise_equals_cast_then_gemm(fmt, tag, mode_name, mode, M, N, K):
    x, w, bias = _operands(fmt, M, N, K, 7 + M, True)
    x[0, :min(K, 64)] = x[0, :min(K, 64)] * 1e30  # a block that saturates and one next to it
    wq, ws = _cast(w, fmt, "rceil")
    fused = _run_fused(fmt, x, wq, ws, bias, M, N, K, mode)
    aq, a_s = _cast(x, fmt, mode_name)
    two = _run_codes(fmt, aq, a_s, wq, ws, bias, M, N, K)
    assert torch.equal(fused.raw, two.raw)


def test_fp4_lane_map_one_hot():
    """A = one-hot asymmetric e2m1 operands at M = N = 16, K = 128: out[m][n] = sum over k of a[m][k] b[n][k] picks the single k where
    both rows are non-zero; distinct values per (row, k) pin which lane / nibble the kernel feeds to which row and k."""
    M = N = 16
    K = 128
    codes_a = np.zeros((M, K), dtype=np.uint8)
    codes_b = np.zeros((N, K), dtype=np.uint8)
    for m in range(M):
        codes_a[m, (7 * m + 3) % K] = 2 + (m % 6)  # 1.0 .. 6.0
    for n in range(N):
        for m in range(M):
            if (m + n) % 5 == 0:
                codes_b[n, (7 * m + 3) % K] = 2 + (n % 3)
    pack = lambda c: (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)  # noqa: E731
    sa = np.full((M, K // 32), 127, dtype=np.uint8)
    sb = np.full((N, K // 32), 127, dtype=np.uint8)
    sa[:, 1] = 128  # block 1 of A counts twice: the scale map is pinned too
    sb[:, 3] = 126
    t = lambda a: torch.from_numpy(a).to(_dev())  # noqa: E731
    buf = _run_codes(R.FMT_E2M1, t(pack(codes_a)), t(sa), t(pack(codes_b)), t(sb), None, M, N, K)
    y, _ = R.linear_f64(pack(codes_a), sa, pack(codes_b), sb, R.FMT_E2M1)
    assert torch.equal(buf.out.to(torch.float64).cpu(), torch.from_numpy(y))
    assert float(np.abs(y).sum()) > 0


def _sqnr(ref, y):
    ref, y = ref.float(), y.float()
    return (20 * torch.log10(torch.linalg.norm(ref) / torch.linalg.norm(ref - y))).item()


@pytest.mark.parametrize("elem,fmt,thr", [(torch.float8_e4m3fn, R.FMT_E4M3, 25.0), (torch.float4_e2m1fn_x2, R.FMT_E2M1, 12.0)])
@pytest.mark.parametrize("bias_on", [False, True])
def test_quantize_mlp(elem, fmt, thr, bias_on):
    from ao_amd.prototype.mx import MXDynamicActivationMXWeightConfig, MXTensor
    from ao_amd.quantization import KernelPreference, quantize_

    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(256, 192, bias=bias_on), torch.nn.ReLU(), torch.nn.Linear(192, 128, bias=bias_on))
    m = m.to(torch.bfloat16).to(_dev())
    x = torch.randn(9, 256, dtype=torch.bfloat16, device=_dev())
    with torch.no_grad():
        ref = m(x)
        first = m[0](x)
    quantize_(m, MXDynamicActivationMXWeightConfig(activation_dtype=elem, weight_dtype=elem))
    w = m[0].weight
    assert isinstance(w, MXTensor) and w.shape == (192, 256) and not w.is_swizzled_scales
    assert tuple(w.scale.shape) == (192, 8)
    with torch.no_grad():
        y = m(x)
        y0 = m[0](x)
    assert _sqnr(ref, y) >= thr
    assert _sqnr(first, y0) >= thr
    # the first linear against the oracle: float64 sum within the parity bound, and the oracle's EMULATED rounding of the same codes
    xb = x.view(torch.int16).cpu().numpy().view(np.uint16)
    aq, a_s = R.quantize(xb, fmt, 1)
    bias = m[0].bias.view(torch.int16).cpu().numpy().view(np.uint16) if bias_on else None
    ref64, S = R.linear_f64(aq, a_s, _np(w.qdata), _np(w.scale), fmt, bias)
    buf = Guarded(9, 192, torch.bfloat16, _dev())
    buf.out.copy_(y0)
    check(buf, ref64=torch.from_numpy(ref64).to(_dev()), S=torch.from_numpy(S).to(_dev()), K=256)
    emu = R.emulated_linear_bf16(aq, a_s, _np(w.qdata), _np(w.scale), fmt, bias)
    close = np.abs(emu.view(np.int16).astype(np.int32) - y0.view(torch.int16).cpu().numpy().astype(np.int32)) <= 1
    assert close.mean() > 0.97
    # the EMULATED preference runs the reference's arithmetic on the same weights
    w.kernel_preference = KernelPreference.EMULATED
    w.act_quant_kwargs.kernel_preference = KernelPreference.EMULATED
    with torch.no_grad():
        ye = m[0](x)
    np.testing.assert_array_equal(ye.view(torch.int16).cpu().numpy().view(np.uint16), emu)


@pytest.mark.parametrize("elem", [torch.float8_e4m3fn, torch.float4_e2m1fn_x2])
def test_oracle_matches_fixture_emulated(elem):
    tag = "fp4" if elem == torch.float4_e2m1fn_x2 else "fp8"
    fmt = R.FMT_E2M1 if tag == "fp4" else R.FMT_E4M3
    aq, a_s = R.quantize(GOLDEN["lin_x"], fmt, 1)
    wq, ws = R.quantize(GOLDEN["lin_w"], fmt, 1)
    np.testing.assert_array_equal(R.emulated_linear_bf16(aq, a_s, wq, ws, fmt), GOLDEN[f"lin_{tag}_nobias"])
    np.testing.assert_array_equal(R.emulated_linear_bf16(aq, a_s, wq, ws, fmt, GOLDEN["lin_b"]), GOLDEN[f"lin_{tag}_bias"])
    # and the GPU cast gives the oracle's codes for these operands
    q, s = _cast(_bf16(GOLDEN["lin_w"]), fmt, "rceil")
    np.testing.assert_array_equal(_np(q), wq)
    np.testing.assert_array_equal(_np(s), ws)


@pytest.mark.parametrize("elem", [torch.float8_e4m3fn, torch.float4_e2m1fn_x2])
def test_torch_compile_fullgraph_bitwise(elem):
    from ao_amd.prototype.mx import MXDynamicActivationMXWeightConfig
    from ao_amd.quantization import quantize_

    torch.manual_seed(5)
    lin = torch.nn.Linear(128, 96, bias=True).to(torch.bfloat16).to(_dev())
    quantize_(lin, MXDynamicActivationMXWeightConfig(activation_dtype=elem, weight_dtype=elem))
    x = torch.randn(3, 128, dtype=torch.bfloat16, device=_dev())
    with torch.no_grad():
        eager = lin(x)
        compiled = torch.compile(lin, fullgraph=True)(x)
    assert torch.equal(eager.view(torch.int16), compiled.view(torch.int16))


def test_dequantize_matches_reference_bits():
    from ao_amd.prototype.mx import MXTensor

    for elem, tag in ((torch.float4_e2m1fn_x2, "fp4"), (torch.float8_e4m3fn, "fp8")):
        for name, key in (("seeded", "dequant_"), ("edge", "dequant_edge_")):
            t = MXTensor.to_mx(_bf16(GOLDEN[f"{name}_x"]), elem, 32, scaling_mode=__import__("ao_amd.prototype.mx", fromlist=["x"]).ScaleCalculationMode.RCEIL)
            d = t.dequantize(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)
            ref = GOLDEN[key + tag]
            nan = lambda b: (b & 0x7FFF) > 0x7F80  # noqa: E731
            np.testing.assert_array_equal(nan(d), nan(ref))
            np.testing.assert_array_equal(np.where(nan(d), 0, d), np.where(nan(ref), 0, ref))
