"""CPU: the inputs of tests/test_training_casts_gpu.py reach what they are built to reach.  No kernel runs here: the restatements alone cast
the same inputs (tests/training_cast_cases.py), and the conditions below are conditions on those inputs -- the launch forms the row-cast
list selects, the trips the NVFP4 amax shapes need, every amax present once, and, for the value-exhaustive inputs, every finite e4m3 code
(every e2m1 code) among the expected outputs, an exact rounding tie and a live clamp in each cast.
"""
import numpy as np
import pytest

import training_cast_cases as K
from oracle import mx_ref


# ---- 1. the one-launch row cast ------------------------------------------------------------------------------------------------------------
def test_the_row_cast_list_reaches_every_launch_form_at_its_full_and_a_ragged_extent():
    """ao_fp8_train_quantize_rowwise (ao_amd/csrc/fp8_train_kernels.hip:260-265) picks fp8_train_quant_rowwise_kernel<NV> from
    per_thread = ceil(C / 8 / 256): <= 1, 2, 4, 8 -> NV = 1, 2, 4, 8 (the row in registers), else NV = 0 (two sweeps).  A change of the
    launcher's thresholds must change K.row_depth, and then this list."""
    assert [K.row_depth(c) for c in K.ROW_C] == [1, 1, 2, 2, 4, 4, 8, 8, 0, 0]
    assert {K.row_depth(c) for c in K.ROW_C} == {0, 1, 2, 4, 8}
    for nv in (1, 2, 4, 8):
        vecs = [c // 8 for c in K.ROW_C if K.row_depth(c) == nv]
        assert nv * K.ROW_THREADS in vecs, "depth %d at its full extent" % nv                       # every thread holds nv vectors
        assert any(v % K.ROW_THREADS for v in vecs), "depth %d at a ragged extent" % nv             # the last pass has idle threads
    sweeps = [-(-(c // 8) // K.ROW_THREADS) for c in K.ROW_C if K.row_depth(c) == 0]
    assert min(sweeps) == 9 and max(sweeps) > 16  # just past the registers, and many passes of the loop
    assert all((c // 8) % K.ROW_THREADS for c in K.ROW_C if K.row_depth(c) == 0)
    assert all(c % 16 == 0 for c in K.ROW_C) and 1 in K.ROW_R and max(K.ROW_R) > 1


@pytest.mark.parametrize("plant", ["last", "first"])
def test_a_row_cases_maximum_sits_once_in_the_planted_vector(plant):
    for R_, C in ((3, 2064), (17, 16400)):
        x = np.abs(K.f32(K.row_case(R_, C, plant)))
        m = x.max(axis=1, keepdims=True)
        assert np.all((x == m).sum(axis=1)[m[:, 0] > 0] == 1) and int((m[:, 0] == 0).sum()) == 1
        where = x.argmax(axis=1)[m[:, 0] > 0] // 8
        assert np.all(where == (C // 8 - 1 if plant == "last" else 0))
        assert len(set(m[:, 0].tolist())) > 2  # rows of different magnitudes


# ---- 2. the NVFP4 amax ---------------------------------------------------------------------------------------------------------------------
def test_the_amax_shapes_fill_the_grid_pass_it_and_divide_by_no_power_of_two():
    """ao_nvfp4_train_amax (nvfp4_train_kernels.hip:259-261): min(ceil(units / 256), 1024) workgroups of 256 threads stride over
    (M / 16)(N / 2) units."""
    units = [K.amax_units(m, n) for m, n in K.AMAX_SHAPES]
    assert units[0] == K.AMAX_GRID_UNITS                                # the full grid, one trip
    assert units[1] - K.AMAX_GRID_UNITS == 2048                         # a second trip over the last 16-row block alone
    assert units[1] - 2048 == (K.AMAX_SHAPES[1][0] // 16 - 1) * (K.AMAX_SHAPES[1][1] // 2)
    half = K.AMAX_SHAPES[2][1] // 2
    assert half == 4040 and half & (half - 1) != 0 and units[2] > K.AMAX_GRID_UNITS
    for (m, n), u in zip(K.AMAX_SHAPES, units):
        plants = K.amax_plants(m, n)
        assert plants["unit0"][0] == 0 and plants["last"][0] == u - 1 and ("trip2" in plants) == (u > K.AMAX_GRID_UNITS)
        assert {s for _, s in plants.values()} == {1.0, -1.0}


# ---- 3. every amax -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [16, 32, 128])
def test_amax_rows_hold_every_amax_once_over_smaller_values_of_either_sign(width):
    xb = K.amax_rows(width)
    x = K.f32(xb)
    assert xb.shape == (K.N_AMAX, width) and np.all(np.isfinite(x))
    np.testing.assert_array_equal(np.abs(x).max(axis=1).view(np.uint32), K.amax_values().view(np.uint32))
    assert np.all((np.abs(x) == np.abs(x).max(axis=1, keepdims=True)).sum(axis=1)[1:] == 1)
    assert (x < 0).any(axis=1).mean() > 0.99 and (x > 0).any(axis=1).mean() > 0.99 and (x == 0).any(axis=1).all()
    assert len(set(np.abs(x).argmax(axis=1)[1:].tolist())) == width  # the amax visits every column


def test_amax_groups_and_weight_blocks_hold_their_amaxes():
    xb, offs = K.amax_groups()
    x = np.abs(K.f32(xb)).reshape(-1, 16, 16)
    np.testing.assert_array_equal(x.max(axis=1).reshape(-1), K.amax_values())
    assert offs.shape == (2040,) and offs[0] == 16 and offs[-1] == K.N_AMAX
    a = K.weight_block_amaxes()
    assert a.shape == (2040,) and len(set(a.tolist())) == 2040 and a.max() < 0x7F80
    w = np.abs(K.f32(K.weight_blocks())).reshape(2040, 128 * 128)
    np.testing.assert_array_equal(w.max(axis=1), K.f32(a))
    assert np.all((w == w.max(axis=1, keepdims=True)).sum(axis=1)[8:] == 1)


# ---- 4. every value ------------------------------------------------------------------------------------------------------------------------
def _all_e4m3(q, what):
    missing = sorted(set(K.E4M3_FINITE.tolist()) - set(np.unique(q).tolist()))
    assert not missing, "%s: e4m3 codes never expected: %s" % (what, ["%#x" % c for c in missing])
    assert not (set(np.unique(q).tolist()) - set(K.E4M3_FINITE.tolist())), what + ": a NaN code"


def _tie_and_clamp(t, what, tie=True, clamp=True):
    assert not tie or K.e4m3_ties(t).any(), what + ": no input is an exact tie"
    assert not clamp or (np.abs(t) > 448.0).any(), what + ": no input is clamped"


def test_every_arrangement_is_the_65536_patterns_with_the_non_finite_ones_zeroed():
    want = np.sort(K.all_values().reshape(-1))
    assert int((K.all_values() == 0).sum()) == 257  # 254 NaN, +-Inf and +0
    for xb in (K.row_blocks(128), K.col_blocks(128), K.row_blocks(32), K.col_blocks(32), K.row_blocks(16), K.weight_quadrants()):
        assert xb.shape == (256, 256)
        np.testing.assert_array_equal(np.sort(xb.reshape(-1)), want)


def test_the_casts_that_take_their_amax_meet_every_code_a_tie_and_the_clamp():
    xb = K.all_values()
    qs, ts = [], []
    for amax in K.FP8_GIVEN_AMAX:
        for pow2 in (False, True):
            q, _, t = K.fp8_given(xb, amax, pow2)
            qs.append(q)
            ts.append(t)
    _all_e4m3(np.stack(qs), "fp8_train_cast under the given amaxes")
    _tie_and_clamp(np.stack(ts), "fp8_train_cast under the given amaxes")
    q, _, t = K.fp8_given(xb, 448.0, False)  # the one launch with scale 1 meets them all by itself
    _all_e4m3(q, "fp8_train_cast under amax 448")
    _tie_and_clamp(t, "fp8_train_cast under amax 448")
    own = K.fp8_given(xb, K.FP8_GIVEN_AMAX[0], False)[0]
    quarter = K.fp8_given(xb, K.FP8_GIVEN_AMAX[1], False)
    assert (np.abs(quarter[2]) > 448.0).sum() > 400 and not np.array_equal(own, quarter[0])  # two binades saturate


def test_the_casts_that_find_their_amax_meet_every_code_a_tie_and_the_clamp():
    for pow2 in (False, True):
        q, _, _, t = K.fp8_rowwise(K.row_blocks(128), pow2)
        _all_e4m3(q, "fp8 rowwise pow2=%d" % pow2)
        _tie_and_clamp(t, "fp8 rowwise pow2=%d" % pow2, tie=pow2, clamp=not pow2)  # (a power-of-two scale never passes 448; the other ties
        #                                                                             where the amax is 1.75 2^e, which the blockwise casts meet)
    q, _, t = K.block_rows(K.row_blocks(128))
    _all_e4m3(q, "blockwise 1 x 128")
    _tie_and_clamp(t, "blockwise 1 x 128")
    q, _, t = K.block_cols(K.col_blocks(128))
    _all_e4m3(q, "blockwise 128 x 1")
    _tie_and_clamp(t, "blockwise 128 x 1")
    q, _, t = K.block_weight(K.weight_quadrants())
    _all_e4m3(q, "blockwise 128 x 128")
    _tie_and_clamp(t, "blockwise 128 x 128")
    for name, mode in (("floor", mx_ref.FLOOR), ("rceil", mx_ref.RCEIL)):
        q, _, t = K.mx_rows(K.row_blocks(32), mode)
        _all_e4m3(q, "mxfp8 rows " + name)
        _tie_and_clamp(t, "mxfp8 rows " + name, clamp=mode == mx_ref.FLOOR)  # (RCEIL rounds the scale up: nothing passes 448)
        q, _, t = K.mx_cols(K.col_blocks(32), mode)
        _all_e4m3(q, "mxfp8 columns " + name)
        _tie_and_clamp(t, "mxfp8 columns " + name, clamp=mode == mx_ref.FLOOR)


def test_the_nvfp4_cast_meets_all_16_codes_a_tie_and_the_clamp_under_either_rounding():
    xb = K.row_blocks(16)
    for sr in (None, K.NVFP4_VALUES_SR):
        codes, ties, clamped = set(), False, False
        for amax in K.NVFP4_GIVEN_AMAX:
            q, _, t = K.nvfp4_rows(xb, amax, sr)
            codes |= set(np.unique(K.unpack4(q.numpy())).tolist())
            v = t.numpy()
            ties |= bool(K.e2m1_ties(v).any())
            clamped |= bool((np.abs(v) > 6.0).any())
        assert codes == set(range(16)), (sr, sorted(codes))
        assert ties and clamped, (sr, ties, clamped)
