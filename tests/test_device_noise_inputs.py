"""The oracle of the device noise source (tests/device_noise_oracle.py) and the definition itself, without a GPU: Philox4x32-10 known
answers, the first normals, and the statistics of the float64 normals over 80 (seed, image, draw) tensors of 65536 values -- the
definition must be a usable noise source before the kernel is compared with it."""
import numpy as np
import pytest

from tests import device_noise_oracle as O

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_philox_known_answers(case):
    counter, key, want = KNOWN[case]
    got = O.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert " ".join("%08x" % int(v) for v in got) == want


def test_counter_layout_and_key_split():
    """counter = (pixel, image, draw, 0), key = (seed_lo, seed_hi)"""
    seed, image, draw = 0x0123456789ABCDEF, 7, 0xFFFFFFFF
    b = O.bits(seed, image, draw, 5)
    for pix in range(5):
        assert np.array_equal(b[pix], O.philox4x32_10((pix, image, draw, 0), (0x89ABCDEF, 0x01234567)))
    assert not np.array_equal(O.bits(seed, image, draw, 5), O.bits(seed ^ (1 << 63), image, draw, 5))          # the high word is used


def test_first_normals():
    got = O.normals(0, 0, 0, 1)[0]
    assert np.abs(got - np.array([0.99113748, -0.92466278, -0.61760905, -0.48206835])).max() < 1e-7


def test_uniforms_are_exact_in_fp32_and_never_0_or_1():
    w = np.array([0, 1, 511, 512, 0xFFFFFFFF, 0x80000000], dtype=np.uint32)
    u = O.uniforms(w)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    # the largest magnitude: u0 = 2^-24 -> sqrt(2 ln 2^24) = 5.768 (the tails beyond are cut: documented in the header)
    assert abs(O.CLIP - 5.7681) < 1e-4 and O.CLIP <= 5.77


def test_statistics_of_the_definition():
    worst, distinct = O.all_stats(lambda s, i, d: O.normals(s, i, d, O.STAT_HW))
    print("device noise, float64 oracle, worst figures (in standard errors):", {k: round(v, 2) for k, v in worst.items()})
    assert distinct
    assert set(worst) == {"mean", "std", "m4", "channel_pairs", "lag1", "images", "draws", "seeds"}
    for name, v in worst.items():
        assert v <= O.STAT_BAR, (name, v)
    x = O.normals(2 ** 64 - 1, 1, 51, O.STAT_HW)
    assert np.abs(x).max() <= O.CLIP
