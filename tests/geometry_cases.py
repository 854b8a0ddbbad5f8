"""Full-width (SD1.5: 320 / 640 / 1280 / 1280 channels) workloads OFF the benchmarked geometries (512x512, 512x640, 768x576), as a test plan.
Host only: nothing here touches a GPU.

``GEOMETRY_CASES`` is the one list the GPU tests draw from (tests/test_dispatch_sweep_gpu.py: per-launch replay; tests/test_fullsize_gpu.py: whole
forward against the fp32 oracle; tests/test_geometry_gpu.py: attention replay).  ``describe(case, table)`` says, level by level, what maps, token
counts and CFG row counts a case runs and which of the geometry-conditional branches of the fast paths it leaves the tuned road on
(``CONDITIONS``); tests/test_host_logic.py asserts that the list as a whole covers every one of them."""
from collections import namedtuple

from tests.dispatch_cases import parse_key

# latent (h, w) rows x columns (image = 8x), images per call (the CFG batch has twice as many rows), garment latent (h, w) or None = the generation size
GeoCase = namedtuple("GeoCase", "id h w images garment")
Level = namedtuple("Level", "level channels head_dim H W tokens cfg_rows garment_tokens")

CHANNELS = (320, 640, 1280, 1280)       # UNet levels 0..3 (level 3: the last down block and the mid block)
HEADS = 8

GEOMETRY_CASES = (
    GeoCase("16x16", 16, 16, 1, None),
    GeoCase("8x8", 8, 8, 1, None),
    GeoCase("16x32", 16, 32, 1, None),
    GeoCase("24x40 x3", 24, 40, 3, None),
    GeoCase("24x24 garment 16x24", 24, 24, 1, (16, 24)),
    GeoCase("32x8", 32, 8, 1, None),                    # an image 64 wide, 256 high
    GeoCase("32x32 x5", 32, 32, 5, None),               # CFG rows 10240 / 2560 / 640 / 160: the row counts of the tabulated 512x640 batch-1 workload, on other maps
)

CONDITIONS = {
    "a": "level-0 tokens per image % 128 != 0 (no fused norm1 -> q/k/v)",
    "b": "level-0 N < 512 (the small head-dim-40 attention kernel, no duplicated first phase)",
    "c-ragged": "level-0 N >= 512 with N % 256 != 0",
    "c-512": "level-0 N == 512 exactly",
    "d": "a level with W % 16 != 0 and W >= 16",
    "e": "a level with H < 8 or W < 16 at >= 64 channels (no halo-patch convolution)",
    "f-short": "an 8-wide map with H <= 12 (whole-map convolution kernel)",
    "f-tall": "an 8-wide map with H > 12 (too tall for the whole-map kernel)",
    "g-odd": "a map with an odd side",
    "g-1x1": "a 1x1 deepest level",
    "h": "a CFG batch that is 2 x an odd count",
    "i": "once-per-image first block eligible (level-0 N >= 512) with res_rows % 128 != 0 (no periodic residual)",
    "j": "garment token count != query count and not a multiple of 64",
    "k": "a CFG row count M equal to a plain (not |HxW) key of the tuning table, on a map the table holds no entry of that M for",
}


def levels(case):
    """The four UNet levels of a case: maps halve per level (latent sides are multiples of 8: the skips need that)."""
    if case.h % 8 or case.w % 8 or (case.garment and (case.garment[0] % 8 or case.garment[1] % 8)):
        raise ValueError(f"{case.id}: latent sides must be multiples of 8")
    out = []
    for lv, ch in enumerate(CHANNELS):
        H, W = case.h >> lv, case.w >> lv
        gh, gw = case.garment or (case.h, case.w)
        out.append(Level(lv, ch, ch // HEADS, H, W, H * W, 2 * case.images * H * W, (gh >> lv) * (gw >> lv)))
    return out


def foreign_plain_keys(table, M, channels, H, W):
    """Plain keys of the tuning table with ``M`` rows and the level's channel count on either side that a problem on an HxW map can land on: the
    table holds no ``|HxW`` entry of that row count for this map, i.e. every entry of that M was timed elsewhere."""
    home = set()
    plain = []
    for key in table:
        base, (kM, kN, kK, taps, _, _), hw = parse_key(key)
        if kM != M:
            continue
        if hw is not None:
            home.add(hw)
        elif channels in (kN, kK // taps):
            plain.append(key)
    return [] if (H, W) in home else plain


def describe(case, table):
    """-> dict(levels=[Level ...], conditions={name, ...}, collisions=[plain table keys a level's CFG rows land on from a foreign map])."""
    lv = levels(case)
    l0 = lv[0]
    hit = set()
    if l0.tokens % 128:
        hit.add("a")
    if l0.tokens < 512:
        hit.add("b")
    if l0.tokens >= 512 and l0.tokens % 256:
        hit.add("c-ragged")
    if l0.tokens == 512:
        hit.add("c-512")
    collisions = []
    for L in lv:
        if L.W % 16 and L.W >= 16:
            hit.add("d")
        if (L.H < 8 or L.W < 16) and L.channels >= 64:
            hit.add("e")
        if L.W == 8:
            hit.add("f-short" if L.H <= 12 else "f-tall")
        if L.H % 2 or L.W % 2:
            hit.add("g-odd")
        if L.garment_tokens != L.tokens and L.garment_tokens % 64:
            hit.add("j")
        collisions += foreign_plain_keys(table, L.cfg_rows, L.channels, L.H, L.W)
    if (lv[-1].H, lv[-1].W) == (1, 1):
        hit.add("g-1x1")
    if case.images % 2:
        hit.add("h")
    if l0.tokens >= 512 and (case.images * l0.tokens) % 128:        # the first block's residuals hold one copy per image: images x N rows
        hit.add("i")
    if collisions:
        hit.add("k")
    return dict(levels=lv, conditions=hit, collisions=collisions)


def workload_kwargs(case):
    """``tests/test_dispatch_sweep_gpu.py::WORKLOADS`` entry of a case (configs[1]: the bench.py pipeline at another size)."""
    return dict(config=1, batch=case.images, width=8 * case.w, height=8 * case.h, garment=case.garment)
