"""GPU: the AWQ scale-search kernel against tests/awq_ref.py byte for byte, the observer, the search and AWQConfig end to end.

Layers.  (1) ops.awq_scaled_error on given (W, S): D equals the restatement's bytes for every group size, at one row and at the 64-row
marks, at K = g (a single group a row), at sizes whose vector count is no multiple of the 256-lane workgroup and at a row that spans more
than one workgroup; on values that reach the corners of the chain.  (2) the chain's middle, dq, is Int4Tensor.from_hp(W * S[r]).dequantize()
on the device: the search judges the codes `convert` stores.  (3) the observer's sums; the search's losses against the float64 value of
the reference's formula, and its pick.  (4) quantize_ prepare -> calibrate -> convert, and prepare_for_loading.
"""
import functools
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import awq_cases as C
import awq_ref as R
from oracle import bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"
NS = (1, 3, 4, 5, 63, 64, 65, 130)
RS = (1, 2, 20)


def _dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def _launch(Wnp, Snp, g):
    """D of fresh device copies, twice: into a buffer pre-filled with a sentinel, and into one the op allocates"""
    from ao_amd import ops

    W, S = _dev_bf16(Wnp), _dev_bf16(Snp)
    out = torch.full((Snp.shape[0],) + Wnp.shape, float("nan"), dtype=torch.float32, device=DEV)
    assert ops.awq_scaled_error(W, S, g, out=out) is out
    again = ops.awq_scaled_error(W, S, g)
    torch.cuda.synchronize()
    return out.cpu().numpy(), again.cpu().numpy()


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _check(Wnp, Snp, g):
    want = R.scaled_error(Wnp, Snp, g)
    assert np.isfinite(want).all()
    got, again = _launch(Wnp, Snp, g)
    assert _same(got, want), f"D differs in {(got.view(np.uint32) != want.view(np.uint32)).sum()} of {want.size} places"
    assert _same(again, got), "two launches gave different bytes"


KERNEL_CASES = [(g, K) for g in (32, 64, 128, 256) for K in sorted({g, 256, 384, 1024 + g}) if K % g == 0]


@pytest.mark.parametrize("g,K", KERNEL_CASES, ids=[f"g{g}-K{K}" for g, K in KERNEL_CASES])
def test_kernel_equals_the_restatement_byte_for_byte(g, K):
    """every N of the list at this (g, K); R walks 1, 2, 20 so that, over the cases, every N meets every R.  N K / 8 is no multiple of the
    256-lane workgroup for N = 1, 3, 5, 63, 65 at every K here (N = 1, K = 32: four lanes of one wave are live)."""
    for i, N in enumerate(NS):
        nr = RS[(i + KERNEL_CASES.index((g, K))) % 3]
        _check(C.weights(N, K, 31 * N + K), C.scales(nr, K, N + g), g)


def test_kernel_row_spans_workgroups():
    """K = 4352: 544 vectors a row, more than two workgroups of 256 lanes, and rows that start in the middle of one"""
    _check(C.weights(3, 4352, 7), C.scales(2, 4352, 7), 256)
    _check(C.weights(2, 4352, 8), C.scales(3, 4352, 8), 32)


def test_every_n_meets_every_r():
    seen = {(N, RS[(i + c) % 3]) for c in range(len(KERNEL_CASES)) for i, N in enumerate(NS)}
    assert seen == {(N, r) for N in NS for r in RS}


@pytest.mark.parametrize("g", (32, 64, 128, 256))
def test_kernel_corner_values(g):
    """rounding ties of (ws - m) / s (kept as ties by power-of-two scales), all-equal and all-zero groups and ranges below the 1e-6
    clamp, -0.0, scales at the 1e-4 clamp's value and over 2^-7 .. 2^7"""
    Wnp, Snp = C.corner_weights(g), C.corner_scales(g)
    c = R.chain(Wnp, Snp, g)
    t = (c["ws"].reshape(6, 8, 2, g) - c["ws"].reshape(6, 8, 2, g).min(axis=3, keepdims=True)) / c["scale"][..., None]
    assert (np.abs(t - np.floor(t) - 0.5) == 0).sum() >= 50, "the case lost its ties"
    assert (c["scale"] == np.float32(1e-6) / np.float32(15)).sum() >= 12, "the case lost its clamped groups"
    assert np.signbit(Wnp[Wnp == 0]).any() and Snp.min() <= 2.0 ** -7 and Snp.max() >= 2.0 ** 7
    _check(Wnp, Snp, g)


DQ_CASES = [(5, 384, 128, 11), (17, 256, 32, 12), (4, 512, 256, 13), (3, 192, 64, 14)]


@pytest.mark.parametrize("N,K,g,seed", DQ_CASES)
def test_dq_is_the_weight_convert_stores(N, K, g, seed):
    """the restatement's dq == Int4Tensor.from_hp(W * S[r], [1, g]).dequantize() on the device, byte for byte; so are the codes"""
    from ao_amd.quantization.int4_plain_tensor import Int4Tensor

    Wnp, Snp = C.weights(N, K, seed), C.scales(3, K, seed)
    if K == 2 * g:
        Wnp[:8], Snp = C.corner_weights(g)[:N], C.corner_scales(g)[:3]
    c = R.chain(Wnp, Snp, g)
    W, S = _dev_bf16(Wnp), _dev_bf16(Snp)
    for r in range(Snp.shape[0]):
        t = Int4Tensor.from_hp((W * S[r]).contiguous(), [1, g])
        dq = t.dequantize()
        assert dq.dtype == torch.bfloat16 and np.array_equal(bf16.to_bits(dq.float().cpu().numpy()), bf16.to_bits(c["dq"][r])), r
        q = t.qdata.cpu().numpy()
        lo, hi = (q & 0xF).astype(np.int8), (q >> 4).astype(np.int8)
        codes = np.stack([np.where(lo > 7, lo - 16, lo), np.where(hi > 7, hi - 16, hi)], axis=-1).reshape(N, K)
        assert np.array_equal(codes, c["q"][r]), r
        assert np.array_equal(bf16.to_bits(t.scale.float().cpu().numpy().T), bf16.to_bits(bf16.bf16_round(c["scale"][r])))
        assert np.array_equal(bf16.to_bits(t.zero_point.float().cpu().numpy().T), bf16.to_bits(bf16.bf16_round(c["zero"][r])))


def _base(g):
    from ao_amd.quantization.config import Int4WeightOnlyConfig

    return Int4WeightOnlyConfig(group_size=g, int4_packing_format="plain")


def test_observer_sums():
    """several batches of different row counts, 2-D and 3-D: gram and abs_sum are the float64 sums to fp32 summation error, x_mean is
    within one bf16 ulp of the float64 mean, and a forward never reads the device back"""
    from ao_amd.prototype.awq import AWQObserver

    K = 192
    W, X = C.calibration(8, K, 5 + 24 + 70 + 1, 21)
    obs = AWQObserver(W.to(DEV), None, _base(64))
    Xd = X.to(DEV)
    batches = [Xd[:5], Xd[5:29].reshape(2, 12, K), Xd[29:99].reshape(7, 10, K), Xd[99:]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for x in batches:
            obs(x, None)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert type(obs.rows) is int and obs.rows == 100
    X64 = X.double().numpy()
    u = 2.0 ** -24
    G, A = X64.T @ X64, np.abs(X64).sum(0)
    terms = X64.shape[0] + len(batches)  # additions behind one entry, in any order
    assert obs.gram.dtype == torch.float32 and obs.gram.device.type == "cuda"
    assert np.all(np.abs(obs.gram.cpu().numpy() - G) <= 2 * terms * u * (np.abs(X64).T @ np.abs(X64)))
    assert np.all(np.abs(obs.abs_sum.cpu().numpy() - A) <= 2 * terms * u * A)
    got = bf16.to_bits(obs.get_act_scale().float().cpu().numpy()).astype(np.int64)
    want = bf16.to_bits(bf16.bf16_round((A / 100).astype(np.float32))).astype(np.int64)
    assert np.abs(got - want).max() <= 1


@functools.lru_cache(maxsize=None)
def _searched(N, K, g, rows, seed):
    """one search on the device and the float64 losses of the same table, computed once"""
    from ao_amd.prototype.awq import AWQObserver

    W, X = C.calibration(N, K, rows, seed)
    obs = AWQObserver(W.to(DEV), None, _base(g))
    Xd = X.to(DEV)
    obs(Xd[: rows // 3], None)
    obs(Xd[rows // 3:].reshape(2, -1, K), None)
    best = obs.calculate_qparams()
    torch.cuda.synchronize()
    S = obs.scales.float().cpu().numpy()
    return obs, best, S, R.losses64(W.float().numpy(), S, g, X.float().numpy())


@pytest.mark.parametrize("N,K,g,rows,seed", C.SEARCH)
def test_search(N, K, g, rows, seed):
    obs, best, S, l64 = _searched(N, K, g, rows, seed)
    order = np.sort(l64)
    gap = (order[1] - order[0]) / order[0]
    assert gap >= 1e-3, f"the case's best two ratios are {gap:.2e} apart in float64: a tie could hide a wrong pick"
    losses = obs.losses.cpu().numpy()
    assert obs.losses.dtype == torch.float32 and losses.shape == (20,) and S.shape == (20, K) and np.all(S[0] == 1)
    rel = np.abs(losses.astype(np.float64) - l64) / l64
    print(f"\nawq search N={N} K={K} g={g} rows={rows}: max rel {rel.max():.2e}, best {int(np.argmin(l64))}, gap {gap:.2e}, "
          f"best/rtn {l64.min() / l64[0]:.3f}")
    assert rel.max() <= 2.0 ** -16                                           # (a)
    assert int(obs.best_index) == int(np.argmin(l64))                        # (b)
    assert losses[int(obs.best_index)] < 0.8 * losses[0]                     # (c)
    assert np.array_equal(bf16.to_bits(best.float().cpu().numpy()), bf16.to_bits(S[int(np.argmin(l64))]))


def test_search_chunks_give_the_same_losses(monkeypatch):
    """byte budgets that hold three ratios a launch (chunks of 3, .., 2) and one (the kernel runs with R = 1, twenty times): the losses
    keep the bound of test_search -- the matmul's summation order may change with its shape, the contract does not"""
    from ao_amd.prototype.awq import core

    N, K, g, rows, seed = C.SEARCH[2]
    obs, _, S, l64 = _searched(N, K, g, rows, seed)
    for budget in (3 * 8 * N * K, 1):
        monkeypatch.setattr(core, "AWQ_SEARCH_BYTES", budget)
        got = obs.search_losses(obs.weight.detach(), obs.scales, g).cpu().numpy()
        assert got.shape == (20,) and (np.abs(got.astype(np.float64) - l64) / l64).max() <= 2.0 ** -16
        assert int(np.argmin(got)) == int(np.argmin(l64))


def test_nan_losses_never_win():
    """a NaN loss is +inf to the argmin, and an all-NaN search keeps row 0"""
    from ao_amd.prototype.awq import AWQObserver

    W, X = C.calibration(4, 64, 16, 1)
    obs = AWQObserver(W.to(DEV), None, _base(32), 5)
    obs(X.to(DEV), None)
    obs.gram[0, 0] = float("nan")
    best = obs.calculate_qparams()
    assert torch.isnan(obs.losses).all() and int(obs.best_index) == 0 and torch.all(best == 1)


@functools.lru_cache(maxsize=None)
def _converted():
    from ao_amd.quantization import quantize_
    from ao_amd.prototype.awq import AWQConfig

    W1, X, W2, b1, b2 = C.two_linear_model(0)

    def fresh():
        m = nn.Sequential(nn.Linear(256, 128), nn.Linear(128, 64)).to(torch.bfloat16)
        with torch.no_grad():
            m[0].weight.copy_(W1), m[0].bias.copy_(b1), m[1].weight.copy_(W2), m[1].bias.copy_(b2)
        return m.to(DEV)

    base = _base(32)
    model = fresh()
    quantize_(model, AWQConfig(base, step="prepare"))
    observers = [model[0].act_obs, model[1].act_obs]
    Xd = X.to(DEV)
    for x in (Xd[:100], Xd[100:].reshape(2, 110, 256)):
        model(x)
    quantize_(model, AWQConfig(base, step="CONVERT"))
    rtn = fresh()
    quantize_(rtn, base)
    return model, observers, rtn, fresh, Xd, (W1, X, W2, b1, b2)


def test_quantize_end_to_end():
    from ao_amd.quantization.int4_plain_tensor import Int4Tensor

    model, observers, rtn, fresh, Xd, (W1, X, W2, b1, b2) = _converted()
    for lin, obs, W, b in ((model[0], observers[0], W1, b1), (model[1], observers[1], W2, b2)):
        assert type(lin) is nn.Linear and isinstance(lin.weight, Int4Tensor) and "Int4Tensor" in repr(lin)
        assert obs.gram is None and obs.abs_sum is None and obs.rows == 320  # the K x K buffer is released
        assert not any("act_obs" in k for k in model.state_dict())
        s = obs.scales[int(obs.best_index)]
        assert int(obs.best_index) > 0
        pre = lin.weight.act_pre_scale
        assert pre.dtype == torch.bfloat16 and pre.shape == (W.shape[1],) and torch.equal(pre, 1.0 / s)
        want = Int4Tensor.from_hp((W.to(DEV) * s).contiguous(), [1, 32])
        assert torch.equal(lin.weight.qdata, want.qdata) and torch.equal(lin.weight.scale, want.scale)
        assert torch.equal(lin.weight.zero_point, want.zero_point) and lin.weight.block_size == [1, 32]
        assert torch.equal(lin.bias.cpu(), b) and lin.bias.dtype == torch.bfloat16
    X64 = X.double()
    ref = F.linear(F.linear(X64, W1.double(), b1.double()), W2.double(), b2.double())
    e_awq = (model(Xd).double().cpu() - ref).pow(2).mean().item()
    e_rtn = (rtn(Xd).double().cpu() - ref).pow(2).mean().item()
    print(f"\nawq end to end: mse awq {e_awq:.4e}, round-to-nearest {e_rtn:.4e}, ratio {e_awq / e_rtn:.3f}")
    assert e_awq < 0.8 * e_rtn


def test_prepare_for_loading_takes_a_converted_state_dict():
    from ao_amd.quantization import quantize_
    from ao_amd.quantization.int4_plain_tensor import Int4Tensor
    from ao_amd.prototype.awq import AWQConfig

    model, _, _, fresh, Xd, _ = _converted()
    buf = io.BytesIO()
    torch.save(model.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    shell = fresh()
    with torch.no_grad():
        shell[0].weight.zero_(), shell[1].weight.zero_()
    quantize_(shell, AWQConfig(_base(32), step="prepare_for_loading"))
    mine = shell.state_dict()
    assert list(mine) == list(sd)
    for k in sd:
        a, b = mine[k], sd[k]
        assert type(a) is type(b) and a.shape == b.shape and a.dtype == b.dtype, k
        if isinstance(b, Int4Tensor):
            for f in ("qdata", "scale", "zero_point", "act_pre_scale"):
                assert getattr(a, f).shape == getattr(b, f).shape and getattr(a, f).dtype == getattr(b, f).dtype, (k, f)
            assert torch.all(a.act_pre_scale == 1) and a.block_size == b.block_size
            assert torch.equal(b.qdata, model.state_dict()[k].qdata) and torch.equal(b.act_pre_scale, model.state_dict()[k].act_pre_scale)
    shell.load_state_dict(sd, assign=True)
    assert torch.equal(shell(Xd), model(Xd))


def test_convert_needs_calibration_and_skips_plain_linears():
    from ao_amd.quantization import quantize_
    from ao_amd.prototype.awq import AWQConfig, AWQObservedLinear

    m = nn.Sequential(nn.Linear(64, 16)).to(torch.bfloat16).to(DEV)
    plain = m[0]
    quantize_(m, AWQConfig(_base(32), "convert"))
    assert m[0] is plain and type(m[0].weight) is nn.Parameter
    quantize_(m, AWQConfig(_base(32), "prepare"))
    with pytest.raises(ValueError, match="calibrate observer first by running model on exemplar data"):
        quantize_(m, AWQConfig(_base(32), "convert"))
    assert isinstance(m[0], AWQObservedLinear)


def test_op_refuses_bad_arguments():
    from ao_amd import ops

    W, S = torch.zeros(4, 128, dtype=torch.bfloat16, device=DEV), torch.ones(2, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="one of 32, 64, 128, 256"):
        ops.awq_scaled_error(W, S, 16)
    with pytest.raises(ValueError, match="multiple of group_size"):
        ops.awq_scaled_error(W[:, :96].contiguous(), S[:, :96].contiguous(), 64)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        ops.awq_scaled_error(W.float(), S, 32)
    with pytest.raises(RuntimeError, match=r"S must be a contiguous \[R, 128\]"):
        ops.awq_scaled_error(W, S[:, :64].contiguous(), 32)
    with pytest.raises(RuntimeError, match="out must be a contiguous float32 tensor of shape"):
        ops.awq_scaled_error(W, S, 32, out=torch.empty(2, 4, 64, device=DEV))
    assert ops.awq_scaled_error(W[:0], S, 32).shape == (2, 0, 128) and ops.awq_scaled_error(W, S[:0], 32).shape == (0, 4, 128)
