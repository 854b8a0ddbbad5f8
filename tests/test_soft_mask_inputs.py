"""soft_mask on the CPU: ``image.mask_release_reference`` -- the host route of the inpainting pipeline and the oracle of the GPU tests --
against the brute-force definition, torch's ``adaptive_avg_pool2d``, and the properties the pipeline tests lean on."""
import numpy as np
import pytest
import torch

from tests.soft_mask_cases import (SHAPES, STEPS, aligned_binary_mask, bin_sums, blend_masks, noise_mask, ramp_mask, release_brute,
                                   three_level_mask)


def reference(mask, h, w, n):
    from imagdressing_amd.image import mask_release_reference
    return mask_release_reference(mask, h, w, n)


@pytest.fixture(scope="module", params=range(len(SHAPES)), ids=["%dx%d_to_%dx%d" % (s[0] + s[1]) for s in SHAPES])
def case(request):
    """(masks, (h, w), [(S, cnt)]): the bin sums are computed once per shape"""
    hw, (h, w) = SHAPES[request.param]
    masks = [ramp_mask(hw, 1), noise_mask(hw, 2), np.zeros(hw, np.uint8), np.full(hw, 255, np.uint8)]
    return masks, (h, w), [bin_sums(m, h, w) for m in masks]


def test_closed_form_equals_brute_force(case):
    masks, (h, w), sums = case
    for m, (S, cnt) in zip(masks, sums):
        for n in STEPS:
            got = reference(m, h, w, n)
            assert got.dtype == np.uint16 and got.shape == (h, w)
            assert np.array_equal(got.astype(np.int64), release_brute(S, cnt, n)), n


def test_bin_sums_are_adaptive_avg_pool(case):
    """S / cnt is torch's adaptive_avg_pool2d (= interpolate(mode="area")) in float64, so c = S / (255 cnt) is the pooled mask"""
    masks, (h, w), sums = case
    for m, (S, cnt) in zip(masks[:2], sums[:2]):
        t = torch.from_numpy(m.astype(np.float64))[None, None]
        pooled = torch.nn.functional.adaptive_avg_pool2d(t, (h, w))[0, 0].numpy()
        assert np.allclose(S / cnt, pooled, rtol=1e-13, atol=0)
        assert np.allclose(pooled, torch.nn.functional.interpolate(t, size=(h, w), mode="area")[0, 0].numpy(), rtol=1e-13, atol=0)


def test_release_is_n_minus_ceil_cn_in_64_bits():
    """S n passes 2^32 for a 4096 x 4096 mask on an 8 x 8 latent at 1000 steps; one bin at 255 everywhere but a single byte"""
    m = np.full((4096, 4096), 255, np.uint8)
    m[0, 0] = 254                                                   # bin (0, 0): S = D - 1
    m[:512, 512:1024] = 0                                           # bin (0, 1): S = 0
    got = reference(m, 8, 8, 1000).astype(np.int64)
    S, cnt = 255 * 512 * 512 - 1, 512 * 512
    assert S * 1000 > 2 ** 32
    assert got[0, 0] == 1000 - -(-S * 1000 // (255 * cnt)) == 0     # ceil(c n) = n as long as c > (n - 1) / n
    assert got[0, 1] == 1000 and (got.reshape(-1)[2:] == 0).all()


def test_masks_are_nested_and_the_ends_hold(case):
    masks, (h, w), sums = case
    for m, (S, cnt) in zip(masks, sums):
        for n in (1, 7, 50):
            rel = reference(m, h, w, n).astype(np.int64)
            M = blend_masks(rel, n)
            assert (M[:-1] <= M[1:]).all()                          # M_k is a subset of M_{k+1}
            full, empty = S == 255 * cnt, S == 0
            assert (rel[full] == 0).all() and M[:, full].all()      # c = 1: repainted at every step, a hard mask of 1
            assert (rel[empty] == n).all() and not M[:, empty].any()          # c = 0: never free, ends as the clean original
            between = ~full & ~empty
            assert ((rel[between] >= 0) & (rel[between] < n)).all()           # anything above 0 is free at the last step at least
            assert (M.sum(0) == n - rel).all()                      # the last n - release = ceil(c n) steps are free
    assert sums[2][0].max() == 0 and (sums[3][0] == 255 * sums[3][1]).all()   # (the all-0 and all-255 masks are among them)


@pytest.mark.parametrize("hw,latent", [((64, 64), (8, 8)), ((64, 96), (8, 12)), ((128, 128), (16, 16))])
def test_aligned_binary_mask_is_the_hard_mask_at_every_step(hw, latent):
    """the precondition of the GPU test: for a {0, 255} mask with its edges on bin borders M_k is, for every k, the mask the hard
    route makes -- binarise at 0.5, nearest-resize to the latent"""
    on = np.random.default_rng(3).random(latent) < 0.5
    m = aligned_binary_mask(hw, latent, on)
    hard = torch.nn.functional.interpolate((torch.from_numpy(m)[None, None].float() / 255 >= 0.5).float(), size=latent)[0, 0].numpy()
    assert np.array_equal(hard.astype(bool), on)
    for n in (1, 4, 6, 20):
        M = blend_masks(reference(m, *latent, n), n)
        assert (M == hard.astype(bool)[None]).all()


def test_three_level_mask_has_one_gray_release():
    m, level = three_level_mask((64, 96), (8, 12), 128)
    rel = reference(m, 8, 12, 6).astype(np.int64)
    assert (rel[level == 0] == 6).all() and (rel[level == 2] == 0).all()
    assert (rel[level == 1] == 6 - -(-128 * 6 // 255)).all() and 0 < rel[level == 1][0] < 6          # ceil(128 / 255 * 6) = 4 free steps


def test_an_off_by_one_release_changes_a_blend_mask():
    """sensitivity: the comparison of the GPU tests sees a release map that is wrong by one in a single pixel"""
    m = ramp_mask((64, 64), 4)
    seen = set()
    for n in (1, 7, 50):
        rel = reference(m, 8, 8, n).astype(np.int64)
        M = blend_masks(rel, n)
        for delta in (-1, 1):
            for pix in [i for i in np.ndindex(8, 8) if 0 <= rel[i] + delta <= n][:3]:          # (n = 1: the ramp has no pixel to lower)
                bad = rel.copy()
                bad[pix] += delta
                assert (blend_masks(bad, n) != M).any()
                seen.add((n, delta))
    assert seen >= {(1, 1), (7, -1), (7, 1), (50, -1), (50, 1)}


def test_float_levels_agree_with_the_integer_rule():
    """``mask_latents`` as a float tensor: release = n - ceil(c n) in float64 from the fp32 levels.  Where c = S / D is an fp32 number
    the two rules are the same function; elsewhere the fp32 rounding of c may move ceil(c n) across an integer, by one step at most."""
    from imagdressing_amd.image import release_of_levels
    exact_seen = fractional_seen = 0
    for hw, (h, w) in SHAPES[:4]:
        for m in (ramp_mask(hw, 5), noise_mask(hw, 6), np.kron(np.random.default_rng(7).integers(0, 5, (h, w)) * 51, np.ones((4, 4))).astype(np.uint8)):
            S, cnt = bin_sums(m, h, w)
            D = 255 * cnt
            c32 = (S / D).astype(np.float32)
            exact = c32.astype(np.float64) * D == S                 # c is an fp32 number (the product of two exact integers below 2^53)
            for n in STEPS:
                want = reference(m, h, w, n).astype(np.int64)
                got = release_of_levels(torch.from_numpy(c32), n).astype(np.int64)
                assert np.array_equal(got[exact], want[exact])
                assert (np.abs(got - want) <= 1).all()
            exact_seen += int(exact.sum())
            fractional_seen += int((exact & (S > 0) & (S < D)).sum())
    assert exact_seen >= 32 and fractional_seen > 0                  # (both kinds of pixel were seen)


def test_float_levels_are_checked():
    from imagdressing_amd.image import release_of_levels
    assert release_of_levels(torch.tensor([0.0, 0.5, 1.0, 0.26]), 4).tolist() == [4, 2, 0, 2]
    for bad in (float("nan"), float("inf"), -0.01, 1.01):
        with pytest.raises(ValueError, match=r"finite and in \[0, 1\]"):
            release_of_levels(torch.tensor([0.5, bad]), 4)


def test_reference_refusals():
    m = np.zeros((8, 8), np.uint8)
    for kw in (dict(h=0), dict(w=0), dict(n=0), dict(n=65536)):
        with pytest.raises(ValueError):
            reference(m, **dict(dict(h=2, w=2, n=4), **kw))
    with pytest.raises(ValueError):
        reference(m.astype(np.int32), 2, 2, 4)
    with pytest.raises(ValueError):
        reference(np.zeros((0, 8), np.uint8), 2, 2, 4)
    assert reference(m, 2, 2, 65535).max() == 65535                 # (the largest n fits the uint16)
