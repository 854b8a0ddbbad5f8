"""The two soft_mask kernels on the GPU, exactly: ``imd_image_mask_release`` against ``image.mask_release_reference`` (integer
arithmetic: every comparison is ``torch.equal``) and ``imd_soft_mask_rows`` against ``k >= release``, with rows that must keep their
bytes and a guard band behind the buffer."""
import numpy as np
import pytest
import torch

from tests.soft_mask_cases import noise_mask, ramp_mask

pytestmark = pytest.mark.gpu

WINDOWS = [(64, 64), (100, 77), (37, 29), (5, 5), (96, 128)]
LATENTS = [(8, 8), (8, 16), (12, 16)]
STEPS = [1, 7, 50, 1000]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def as_int(t):
    return t.cpu().to(torch.int32)


@pytest.mark.parametrize("window", WINDOWS, ids=lambda s: "%dx%d" % s)
def test_mask_release_equals_the_reference(dev, window):
    from imagdressing_amd import ops
    from imagdressing_amd.image import mask_release_reference
    H0, W0 = window
    big = noise_mask((H0 + 13, W0 + 21), 9)                       # the 100 x 77 case (and every other) is a strided view of a larger image
    masks = {"ramp": ramp_mask(window, 1), "noise": noise_mask(window, 2), "zeros": np.zeros(window, np.uint8),
             "ones": np.full(window, 255, np.uint8), "view": None}
    for name, m in masks.items():
        if m is None:
            up = torch.from_numpy(big).to(dev)[5:5 + H0, 8:8 + W0]
            m = big[5:5 + H0, 8:8 + W0]
            assert not up.is_contiguous() or W0 == big.shape[1]
        else:
            up = torch.from_numpy(m).to(dev)
        for h, w in LATENTS:
            for n in STEPS:
                got = ops.mask_release(up, h, w, n)
                assert got.dtype == torch.uint16 and tuple(got.shape) == (h, w)
                want = torch.from_numpy(mask_release_reference(np.ascontiguousarray(m), h, w, n).astype(np.int32))
                assert torch.equal(as_int(got), want), (name, h, w, n)
                if name == "zeros":
                    assert (want == n).all()
                if name == "ones":
                    assert (want == 0).all()


def test_mask_release_64_bit_products(dev):
    """S n passes 2^32: a 4096 x 4096 mask on an 8 x 8 latent at 1000 steps, one bin a single byte short of full"""
    from imagdressing_amd import ops
    from imagdressing_amd.image import mask_release_reference
    m = np.full((4096, 4096), 255, np.uint8)
    m[0, 0] = 254
    m[:512, 512:1024] = 0
    m[512:1024, :512] = 128
    got = as_int(ops.mask_release(torch.from_numpy(m).to(dev), 8, 8, 1000))
    assert torch.equal(got, torch.from_numpy(mask_release_reference(m, 8, 8, 1000).astype(np.int32)))
    assert got[0, 0] == 0 and got[0, 1] == 1000 and got[1, 0] == 1000 - 502


def test_device_processor_route(dev):
    """``DeviceImageProcessor.mask_release``: PIL / array / uploaded tensor, whole and through a crop box (a view)"""
    from PIL import Image
    from imagdressing_amd.image import DeviceImageProcessor, mask_release_reference
    proc = DeviceImageProcessor(dev)
    m = ramp_mask((111, 150), 3)
    box = (32, 12, 118, 98)
    want = mask_release_reference(m, 16, 16, 20).astype(np.int32)
    want_box = mask_release_reference(np.ascontiguousarray(m[12:98, 32:118]), 16, 16, 20).astype(np.int32)
    for src in (Image.fromarray(m), m, proc._upload(m, "L")):
        assert torch.equal(as_int(proc.mask_release(src, 16, 16, 20)), torch.from_numpy(want))
        assert torch.equal(as_int(proc.mask_release(src, 16, 16, 20, box)), torch.from_numpy(want_box))


@pytest.mark.parametrize("B", [1, 3, 4])
@pytest.mark.parametrize("HW", [1, 63, 64, 257, 5120])
def test_soft_mask_rows_equals_the_comparison(dev, HW, B):
    from imagdressing_amd import ops
    n = 50
    rng = np.random.default_rng(100 * B + HW)
    rel = rng.integers(0, n + 1, size=(B, HW)).astype(np.uint16)
    rel[0, 0] = 17
    release = torch.from_numpy(rel).to(dev)
    guard = 64
    sentinel = -123.5
    for k in (0, 17, 16, n - 1):                                   # 0, a release value, one below it, the last step
        for skip in (None, 0, B - 1):                              # every row soft; the first / the last row hard
            buf = torch.full((B * HW + guard,), sentinel, dtype=torch.float32, device=dev)
            mask = buf[:B * HW].view(B, HW)
            steps = [k] * B
            if skip is not None:
                steps[skip] = -1 - skip                            # (any negative entry)
            ops.soft_mask_rows(mask, release, torch.tensor(steps, dtype=torch.int32, device=dev))
            want = (k >= torch.from_numpy(rel.astype(np.int32))).float()
            if skip is not None:
                want[skip] = sentinel                              # the hard row keeps its bytes
            assert torch.equal(mask.cpu(), want), (k, skip)
            assert (buf[B * HW:] == sentinel).all()                # nothing past the buffer
            if skip is None:
                assert want[0, 0] == (1.0 if k >= 17 else 0.0)


def test_soft_mask_rows_full_range_of_the_uint16(dev):
    """release values up to 65535 compare as unsigned; a step past every release gives all ones"""
    from imagdressing_amd import ops
    rel = np.array([[0, 1, 32767, 32768, 65534, 65535, 7]], np.uint16)
    release = torch.from_numpy(rel).to(dev)
    for k in (0, 32767, 32768, 65534, 65535):
        mask = torch.zeros(1, 7, device=dev)
        ops.soft_mask_rows(mask, release, torch.tensor([k], dtype=torch.int32, device=dev))
        assert mask.cpu()[0].tolist() == [float(k >= int(r)) for r in rel[0]]
