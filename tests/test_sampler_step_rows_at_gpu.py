"""The fused sampler step through a row -> slot map on the GPU (``imd_sampler_step_rows_at``) and the session's input launch
(``imd_session_input_rows``): slot-indexed state against ``imd_sampler_step_rows`` run on the same data gathered into row order
beforehand -- bit for bit, the two kernels share one per-pixel body --, slots nobody names and skipped rows keep their bytes, map
entries out of range idle, and the input launch reproduces the step's ``x_next``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def g(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _row_coefs(b, K):
    """a different block for every row b, with mixed store slots: K = 4 -> 0, 1, 2, 3; K = 2 -> 0, 1, none, 0; K = 0 -> none"""
    from imagdressing_amd import ops
    zh = [0.7, -0.3, 0.45, -0.2][:K]
    return ops.sampler_coefs(m_x=1.2 + 0.1 * b, m_e=-0.8 - 0.05 * b, z_x=0.9 - 0.07 * b, z_m=0.35 + 0.03 * b, z_h=[c * (1 + 0.2 * b) for c in zh],
                             z_n=0.6 + 0.1 * b, b_img=0.95 - 0.02 * b, b_noise=0.3 + 0.04 * b, in_scale=0.37 + 0.11 * b,
                             store=(b + 1) % (K + 1) - 1)


def _layout(B, slots):
    """(map, inactive rows): non-monotone, one idle row and one row whose coefficient block is inactive (B >= 3); the highest slot used"""
    if B == 1:
        return [slots - 1], set()
    if B == 3:
        return [slots - 1, -1, slots - 3], {2}
    return [slots - 2, -1, slots - 1, 0], {2}


class _Data:
    def __init__(self, B, slots, HW, K, dtype, dev="cuda"):
        self.B, self.slots, self.HW, self.K, self.dtype, self.dev = B, slots, HW, K, dtype, dev
        self.z0, self.eps = g(1, slots, HW, 4).to(dev), g(2, 2 * B, HW, 4).to(dev)
        self.H0 = g(3, K, slots, HW, 4).to(dev) if K else None          # (random values: the sentinel of the history)
        self.noise, self.z_img, self.bn = g(4, slots, HW, 4).to(dev), g(5, slots, HW, 4).to(dev), g(6, slots, HW, 4).to(dev)
        mask = (torch.rand(slots, HW, generator=torch.Generator().manual_seed(7)) > 0.4).float()
        mask[0, 0] = 0.25
        self.mask = mask.to(dev)
        self.guidance = torch.tensor([5.0, 7.5, 9.0, 6.5][:B]).to(dev)
        self.coefs = [_row_coefs(b, K) for b in range(B)]

    def rows(self, rmap, inactive):
        from imagdressing_amd import ops
        return torch.tensor([ops.sampler_coef_row(c, active=(r not in inactive)) for r, c in enumerate(self.coefs)], dtype=torch.float32,
                            device=self.dev)

    def at(self, rmap, inactive, use_noise, use_blend):
        """the indexed launch on the slot-indexed state"""
        from imagdressing_amd import ops
        z, H = self.z0.clone(), (self.H0.clone() if self.K else None)
        xn = torch.full((2 * self.B, self.HW, 8), SENTINEL, dtype=self.dtype, device=self.dev)
        kw = dict(mask=self.mask, z_img=self.z_img, blend_noise=self.bn) if use_blend else {}
        ops.sampler_step_rows_at(z, self.eps, xn, guidance=self.guidance, coef_rows=self.rows(rmap, inactive),
                                 row_slot=torch.tensor(rmap, dtype=torch.int32, device=self.dev), hist=H,
                                 noise=self.noise if use_noise else None, **kw)
        return z, H, xn

    def gathered(self, rmap, inactive, use_noise, use_blend):
        """imd_sampler_step_rows on the same data gathered into row order first (a row without a slot: zeros, an inactive block)"""
        from imagdressing_amd import ops
        live = [0 <= s < self.slots for s in rmap]
        idx = torch.tensor([s if ok else 0 for s, ok in zip(rmap, live)], device=self.dev)

        def take(t, dim=0):
            return None if t is None else t.index_select(dim, idx).contiguous()
        z, H = take(self.z0), take(self.H0, 1)
        xn = torch.full((2 * self.B, self.HW, 8), SENTINEL, dtype=self.dtype, device=self.dev)
        kw = dict(mask=take(self.mask), z_img=take(self.z_img), blend_noise=take(self.bn)) if use_blend else {}
        rows = self.rows(rmap, inactive | {r for r, ok in enumerate(live) if not ok})
        ops.sampler_step_rows(z, self.eps, xn, guidance=self.guidance, coef_rows=rows, hist=H, noise=take(self.noise) if use_noise else None, **kw)
        return z, H, xn


def _compare(d, rmap, inactive, use_noise, use_blend):
    """-> (z, H, xn) of the indexed launch, after every comparison with the gathered one and with the sentinels"""
    what = (d.B, d.slots, d.HW, d.K, rmap, use_noise, use_blend)
    B, K = d.B, d.K
    z, H, xn = d.at(rmap, inactive, use_noise, use_blend)
    zg, Hg, xg = d.gathered(rmap, inactive, use_noise, use_blend)
    assert torch.isfinite(z).all(), what
    stepped = set()
    for r, s in enumerate(rmap):
        if 0 <= s < d.slots and r not in inactive:
            stepped.add(s)
            assert torch.equal(z[s], zg[r]) and not torch.equal(z[s], d.z0[s]), (what, r)
            assert K == 0 or torch.equal(H[:, s], Hg[:, r]), (what, r)           # every history plane
            assert torch.equal(xn[r], xg[r]) and torch.equal(xn[B + r], xg[B + r]), (what, r)
            assert (xn[r][:, 4:] == 0).all() and torch.equal(xn[r], xn[B + r]), (what, r)
        else:                                              # a skipped row: its pixels of x_next keep the sentinel
            assert (xn[r] == SENTINEL).all() and (xn[B + r] == SENTINEL).all(), (what, r)
    for s in range(d.slots):                               # slots no row names, and the slot of a skipped row, keep their bytes
        if s not in stepped:
            assert torch.equal(z[s], d.z0[s]) and (K == 0 or torch.equal(H[:, s], d.H0[:, s])), (what, s)
    return z, H, xn


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("K", [0, 2, 4])
@pytest.mark.parametrize("HW", [16, 64, 320])
@pytest.mark.parametrize("B,slots", [(1, 1), (1, 5), (3, 3), (3, 5), (4, 4)])
def test_indexed_equals_gathered(B, slots, HW, K, dtype):
    """HW = 16: a block spans several rows (and all of a small problem); 64: a wave per row; 320: a row that is no multiple of the
    256-thread block.  Noise and the inpainting-blend operands (slot-indexed) in every combination."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = _Data(B, slots, HW, K, dtype)
    rmap, inactive = _layout(B, slots)
    for use_noise in (False, True):
        for use_blend in (False, True):
            _compare(d, rmap, inactive, use_noise, use_blend)


def test_grid_stride_second_pass():
    """2 x 270000 pixels, more than the 2048 x 256 a grid covers in one pass: the threads that wrap around land in the other row, whose
    slot is another one"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = _Data(2, 3, 270000, 1, torch.float16)
    _compare(d, [2, 0], set(), True, False)


@pytest.mark.parametrize("bad", [-1, -7, 5, 6, 2 ** 30, -2 ** 31], ids=lambda v: f"entry{v}")
def test_map_entry_out_of_range_is_an_idle_row(bad):
    """an entry < 0 or >= slots: that row is skipped whole -- nothing of it moves, no error -- and the other rows step as they do
    without it.  (The kernel compares before it addresses anything through the entry.)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = _Data(3, 5, 80, 2, torch.float16)
    z, H, xn = _compare(d, [4, bad, 1], set(), True, True)
    zi, Hi, xi = _compare(d, [4, -1, 1], set(), True, True)
    assert torch.equal(z, zi) and torch.equal(H, Hi) and torch.equal(xn, xi)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,HW,K", [(1, 1, 0), (3, 77, 4), (4, 320, 2)])
def test_identity_map_is_the_unindexed_launch(B, HW, K, dtype):
    from imagdressing_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = _Data(B, B, HW, K, dtype)
    inactive = {1} if B > 1 else set()
    z, H, xn = d.at(list(range(B)), inactive, True, True)
    z2, H2 = d.z0.clone(), (d.H0.clone() if K else None)
    x2 = torch.full((2 * B, HW, 8), SENTINEL, dtype=dtype, device="cuda")
    ops.sampler_step_rows(z2, d.eps, x2, guidance=d.guidance, coef_rows=d.rows(None, inactive), hist=H2, noise=d.noise, mask=d.mask,
                          z_img=d.z_img, blend_noise=d.bn)
    assert torch.equal(z, z2) and torch.equal(xn, x2) and (K == 0 or torch.equal(H, H2))
    assert not torch.equal(z, d.z0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,slots,HW", [(1, 5, 16), (3, 5, 320), (4, 4, 64)])
def test_session_input_rows_reproduces_the_step(B, slots, HW, dtype):
    """after a step launch, the input launch with that step's in_scale (coefficient [11]) rewrites the launch's x_next exactly, both CFG
    halves, channels 4..7 zero; it follows a permuted map -- the same requests in other rows, as after a repack -- and skips idle rows"""
    from imagdressing_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = _Data(B, slots, HW, 2, dtype)
    rmap, inactive = _layout(B, slots)
    z, H, xn = d.at(rmap, inactive, True, False)
    scales = torch.tensor([c[11] for c in d.coefs], dtype=torch.float32, device="cuda")
    live = [r for r, s in enumerate(rmap) if s >= 0 and r not in inactive]
    stepped_map = [s if r in live else -1 for r, s in enumerate(rmap)]
    out = torch.full_like(xn, SENTINEL)
    before = z.clone()
    ops.session_input_rows(z, torch.tensor(stepped_map, dtype=torch.int32, device="cuda"), scales, out)
    assert torch.equal(out, xn) and torch.equal(z, before)                     # the skipped rows keep the sentinel in both
    for r in live:
        assert (out[r][:, 4:] == 0).all() and torch.equal(out[r], out[B + r]) and not (out[r][:, :4] == SENTINEL).all()
    # the same requests moved to other rows (reversed order), their scales with them
    perm = list(reversed(range(B)))
    moved = torch.full_like(xn, SENTINEL)
    ops.session_input_rows(z, torch.tensor([stepped_map[r] for r in perm], dtype=torch.int32, device="cuda"), scales[perm].contiguous(), moved)
    for new, old in enumerate(perm):
        assert torch.equal(moved[new], xn[old]) and torch.equal(moved[B + new], xn[B + old]), (new, old)


def test_refusals_keep_the_latent():
    """errors, and nothing launched: the latent keeps its bits"""
    from imagdressing_amd import ops
    from imagdressing_amd._lib import ImdError
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    B, slots, HW = 2, 3, 40
    z0, eps = g(1, slots, HW, 4).cuda(), g(2, 2 * B, HW, 4).cuda()
    xn = torch.zeros(2 * B, HW, 8, dtype=torch.float16, device="cuda")
    rows = torch.tensor([ops.sampler_coef_row(ops.sampler_coefs(z_x=0.5))] * B, dtype=torch.float32, device="cuda")
    rs = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
    z = z0.clone()
    for bad in (rs.long(), rs.cpu().tolist(), torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")[::2]):
        with pytest.raises(ImdError, match="row_slot"):
            ops.sampler_step_rows_at(z, eps, xn, guidance=7.5, coef_rows=rows, row_slot=bad)
    with pytest.raises(ImdError, match="coef_rows"):
        ops.sampler_step_rows_at(z, eps, xn, guidance=7.5, coef_rows=rows[:1], row_slot=rs)
    with pytest.raises(ImdError, match="eps"):
        ops.sampler_step_rows_at(z, eps[:2], xn, guidance=7.5, coef_rows=rows, row_slot=rs)
    with pytest.raises(ImdError, match="x_in"):
        ops.session_input_rows(z, rs, torch.ones(2, device="cuda"), xn[:3])
    torch.cuda.synchronize()
    assert torch.equal(z, z0)
    ops.sampler_step_rows_at(z, eps, xn, guidance=7.5, coef_rows=rows, row_slot=rs)
    assert not torch.equal(z[2], z0[2]) and not torch.equal(z[0], z0[0]) and torch.equal(z[1], z0[1])
