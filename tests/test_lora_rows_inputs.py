"""The exact family of tests/lora_rows_cases.py checked on the host in float64: its preconditions (what makes the expected output of
``imd_lora_expand_rows`` known exactly in both element types), and that it can tell a wrong kernel from a right one -- an entry index
off by one row at an entry boundary, a dropped `down` row, a scale applied to the wrong third of T."""
import numpy as np
import pytest

from tests import lora_rows_cases as LC


@pytest.mark.parametrize("shape", LC.SHAPES, ids=lambda s: "C%d_T%d_E%dx%d" % s)
def test_preconditions(shape):
    C, T, E, rpe = shape
    x, down, scale = LC.exact_operands(C, T, E, rpe)
    assert x.shape == (E * rpe, C) and down.shape == (T, C) and scale.shape == (E,)
    assert C % 16 == 0 and T % 16 == 0 and 64 <= C <= 1280 and 16 <= T <= 384
    assert set(np.unique(x)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and len(np.unique(x)) == 5
    assert set(np.unique(down)) <= {-1.0, 0.0, 1.0}
    nz = (down != 0).sum(axis=1)
    assert nz.max() <= LC.MAX_NONZERO and nz.min() >= 1
    assert set(scale) <= set(LC.SCALES) and all(scale[e] != scale[e + 1] for e in range(E - 1))
    sums = x @ down.T
    assert np.all(sums == np.round(sums)) and np.abs(sums).max() <= 64
    assert np.abs(sums).max() >= 8                  # ... and not trivially small
    full = LC.expected(x, down, scale, rpe)
    assert full.shape == (E * rpe, C + T)
    assert LC.fits_fp16(full) and LC.fits_bf16(full)
    assert np.array_equal(full[:, :C], x)
    # partial sums in any order are integers below 2^24: fp32 accumulation is exact whatever the MFMA's order
    assert np.abs(x).max() * LC.MAX_NONZERO < 2 ** 24


def test_representable_helper_rejects_what_does_not_fit():
    assert LC.fits_bf16([31.5, 126.0, 128.0, 0.0, -0.5]) and not LC.fits_bf16([257.0]) and not LC.fits_bf16([1.0 + 2.0 ** -8])
    assert LC.fits_fp16([2047.0, 0.5]) and not LC.fits_fp16([2049.0]) and not LC.fits_fp16([65536.0]) and not LC.fits_fp16([2.0 ** -15])


@pytest.mark.parametrize("shape", LC.SHAPES, ids=lambda s: "C%d_T%d_E%dx%d" % s)
def test_wrong_entry_index_shows_at_the_entry_boundaries_only(shape):
    C, T, E, rpe = shape
    x, down, scale = LC.exact_operands(C, T, E, rpe)
    good = LC.expected(x, down, scale, rpe)
    for shift in (1, -1):
        bad = LC.expected(x, down, scale, rpe, entry_shift=shift)
        rows = np.nonzero((bad != good).any(axis=1))[0]
        # only the last row of an entry (shift +1) / the first (shift -1) can move: the rows whose index crosses a boundary
        boundary = [e * rpe - 1 for e in range(1, E)] if shift == 1 else [e * rpe for e in range(1, E)]
        assert set(rows) <= set(boundary)
        moved = [m for m in boundary if (x[m] @ down.T != 0).any()]
        assert moved and set(rows) == set(moved)
        assert np.array_equal(bad[:, :C], good[:, :C])


@pytest.mark.parametrize("shape", LC.SHAPES, ids=lambda s: "C%d_T%d_E%dx%d" % s)
def test_dropped_down_row_shows_in_its_column(shape):
    C, T, E, rpe = shape
    x, down, scale = LC.exact_operands(C, T, E, rpe)
    good = LC.expected(x, down, scale, rpe)
    for j in (0, T // 2 + 3, T - 1):
        bad = LC.expected(x, down, scale, rpe, drop_row=j)
        cols = np.nonzero((bad != good).any(axis=0))[0]
        assert list(cols) == [C + j]
        want = (scale[LC.entry_of_row(E * rpe, rpe)] != 0) & ((x @ down[j]) != 0)
        assert want.any() and np.array_equal((bad != good)[:, C + j], want)


@pytest.mark.parametrize("shape", [s for s in LC.SHAPES if s[1] % 48 == 0], ids=lambda s: "C%d_T%d_E%dx%d" % s)
def test_scale_on_the_wrong_third_shows_in_that_third(shape):
    C, T, E, rpe = shape
    x, down, scale = LC.exact_operands(C, T, E, rpe)
    good = LC.expected(x, down, scale, rpe)
    third = T // 3
    for g in range(3):
        f = [1.0, 1.0, 1.0]
        f[g] = 2.0
        bad = LC.expected(x, down, scale, rpe, group_scales=f)
        cols = np.nonzero((bad != good).any(axis=0))[0]
        assert cols.size and cols.min() >= C + g * third and cols.max() < C + (g + 1) * third
        rows = np.nonzero((bad != good).any(axis=1))[0]
        assert set(rows) <= set(np.nonzero(scale[LC.entry_of_row(E * rpe, rpe)] != 0)[0])
