"""Exact cases of imd_guidance_rescale (the style of exact_cases.py): small-integer inputs whose every partial sum -- of values and of
squared deviations -- is an integer below 2^24, so every reduction is exact in fp32 WHATEVER its order, the ratio S_t / S_e is a power
of four, and the expected output is known to the bit.  Preconditions are asserted in float64 when a case is built.

  A   u = 0, t in {-2, 0, 2} with equal counts of +-2, g in {2, 4, 8}:  e = g t, mu = 0, r = 1 / g, f = phi / g + 1 - phi
  B   u = 64, t = 64 + s (s as in A), g = 8:  mu_t = mu_e = 64 exactly, S_e = 64 S_t, r = 1 / 8  (a non-zero mean: an uncentred
      variance E[x^2] - mu^2, or a skipped centring, gives another r)
  C   u = t (Gaussian): e = t, S_e = S_t, f = 1: the output equals the input for every phi and g

The first and the last element of every row of A and B are non-zero deviations, so a reduction that drops or repeats either differs."""
import torch

from tests.guidance_rescale_oracle import guidance_rescale as oracle

# the kernel's edge cases: below / at / above a wave (64 pixels) and a quarter of the workgroup (256), not a multiple of the per-thread
# stride (1024 pixels), and either side of the register-resident / re-read boundary (8192 pixels)
HW_SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1025, 8192, 8193)
PHIS = (1.0, 0.5, 0.25)
GS = (2.0, 4.0, 8.0)
LIMIT = float(2 ** 24)


def signs(HW, seed):
    """[HW, 4] float64 in {-2, 0, 2}: equal counts of +2 and -2 (a quarter of the elements each, at least one), the rest 0, shuffled;
    element 0 is +2 and the last one -2"""
    N = 4 * HW
    n2 = max(N // 4, 1)
    mid = torch.cat([torch.full((n2 - 1,), 2.0), torch.full((n2 - 1,), -2.0), torch.zeros(N - 2 * n2)]).double()
    mid = mid[torch.randperm(N - 2, generator=torch.Generator().manual_seed(seed))]
    return torch.cat([torch.tensor([2.0]).double(), mid, torch.tensor([-2.0]).double()]).view(HW, 4)


def build(family, HW, g, phi, B=1):
    """-> (eps [2B, HW, 4] fp32, expected [2B, HW, 4] fp32).  ``g`` / ``phi``: a float, or B values (per row)"""
    gs = [float(g)] * B if not isinstance(g, (list, tuple)) else [float(v) for v in g]
    ps = [float(phi)] * B if not isinstance(phi, (list, tuple)) else [float(v) for v in phi]
    if family == "C":
        t = (torch.randn(B, HW, 4, generator=torch.Generator().manual_seed(7 + HW)) + 0.5).float().double()
        u = t.clone()
    else:
        s = torch.stack([signs(HW, 100 * b + HW) for b in range(B)])
        base = 0.0 if family == "A" else 64.0
        t, u = base + s, torch.full_like(s, base)
    eps = torch.cat([t, u])
    want = oracle(eps, gs, ps)
    check_preconditions(family, eps, want, gs, ps)
    return eps.float(), want.float()


def check_preconditions(family, eps, want, gs, ps):
    B = eps.shape[0] // 2
    N = eps.shape[1] * 4
    assert torch.equal(want.float().double(), want), "the expected output is not representable in fp32"
    if family == "C":
        live = torch.tensor(ps) != 0
        assert torch.equal(want, eps) and live.any()
        return
    for b in range(B):
        t, u = eps[b].reshape(-1), eps[B + b].reshape(-1)
        e = u + gs[b] * (t - u)
        for x in (t, e):
            mu = x.sum() / N
            dev2 = (x - mu) ** 2
            assert torch.equal(x, x.round()) and torch.equal(dev2, dev2.round()) and mu == mu.round()
            assert x.abs().sum() < LIMIT and dev2.sum() < LIMIT          # every partial sum of either reduction is an exact integer
        s_t, s_e = ((t - t.mean()) ** 2).sum(), ((e - e.mean()) ** 2).sum()
        assert s_e == gs[b] ** 2 * s_t and s_t > 0                            # r = 1 / g, a power of two
        f = ps[b] / gs[b] + 1 - ps[b]
        assert float(torch.tensor(f).float()) == f                            # f is an fp32 number
        if ps[b] != 0:
            assert torch.equal(want[b], f * e.view(-1, 4)) and torch.equal(want[B + b], want[b])


def faulty(eps, g, phi, fault):
    """float64 statement of the kernel WITH one fault, for the assertion that the cases would see it:
    drop / double -- one element missing from / counted twice in every reduction;  uncentred -- S = sum x^2;
    neighbour -- the statistics of row (b + 1) % B;  cond_only -- the uncond half keeps its input"""
    x = eps.double()
    B, N = x.shape[0] // 2, x.shape[1] * 4
    gs = [float(g)] * B if not isinstance(g, (list, tuple)) else list(g)
    ps = [float(phi)] * B if not isinstance(phi, (list, tuple)) else list(phi)
    out = x.clone()

    def stats(b):
        t, u = x[b].reshape(-1), x[B + b].reshape(-1)
        e = u + gs[b] * (t - u)
        idx = torch.arange(N)
        if fault == "drop":
            idx = idx[:-1]
        if fault == "double":
            idx = torch.cat([idx, idx[:1]])
        res = []
        for v in (t, e):
            mu = 0.0 if fault == "uncentred" else v[idx].sum() / N
            res.append(((v[idx] - mu) ** 2).sum())
        return res
    for b in range(B):
        if ps[b] == 0:
            continue
        s_t, s_e = stats((b + 1) % B if fault == "neighbour" else b)
        e = x[B + b] + gs[b] * (x[b] - x[B + b])
        f = ps[b] * (1.0 if s_e == 0 else torch.sqrt(s_t / s_e)) + 1 - ps[b]
        out[b] = f * e
        if fault != "cond_only":
            out[B + b] = f * e
    return out
