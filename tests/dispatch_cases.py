"""The tuning table as a test plan: ``cases(table)`` turns every entry of ``imagdressing_amd/gemm_tuning.json`` into the calls of
``ops.conv_gemm`` that reach it the way the product does (``cfg=-1, split_k=0``).  Host only: nothing here touches a GPU.

Key syntax: ``M,N,K,taps,stride,ups`` for a linear layer or a 3x3 conv on any map, ``M,N,K,9,stride,ups|HoxWo`` for a 3x3 conv on that output map.
An entry that no rule below can turn into a case raises ``ValueError`` naming the key: a regenerated table never loses coverage silently."""
from collections import namedtuple

Case = namedtuple("Case", "id key M N K Cin taps stride ups B Hin Win Hout Wout form table_cfg table_split rowvec gn_groups plain")

HEADS = 8            # attention heads of every q/k/v projection of the product
GN_GROUPS = 32       # GroupNorm groups of every ResNet of the product

# forms: "split"  bias + residual (+ per-image row vector and GroupNorm statistics on 3x3 stride-1 entries): the table's (cfg, split)
#        "geglu"  interleaved (value, gate) GEGLU epilogue: (cfg_nosplit, 1)
#        "heads"  q / k / v head-split epilogue into the attention layouts: (cfg_nosplit, 1)
FORMS = ("split", "geglu", "heads")


def parse_key(key):
    base, _, geom = key.partition("|")
    M, N, K, taps, stride, ups = map(int, base.split(","))
    hw = tuple(map(int, geom.split("x"))) if geom else None
    return base, (M, N, K, taps, stride, ups), hw


def input_map(Ho, Wo, stride, ups):
    return (Ho // 2, Wo // 2) if ups else (Ho * stride, Wo * stride)


def off_table_map(table, base):
    """A map the table does not hold for the plain 3x3 key ``base``, so that the lookup lands on the plain entry: the transpose of a sibling's
    map, else a sibling's map twice as high and half as wide."""
    M, _, _, _, _, ups = parse_key(base)[1]
    sibs = [parse_key(k)[2] for k in table if k.startswith(base + "|")]
    for Ho, Wo in sibs:
        if Ho != Wo and f"{base}|{Wo}x{Ho}" not in table:
            return Wo, Ho
    for Ho, Wo in sibs:
        if Wo % (4 if ups else 2) == 0 and f"{base}|{2 * Ho}x{Wo // 2}" not in table:
            return 2 * Ho, Wo // 2
    raise ValueError(f"tuning table key {base!r}: no off-table map found among the maps of its siblings {sibs} "
                     f"(a plain 3x3 key needs a geometry-keyed sibling to derive a test map from)")


def cases_of(table, key):
    ent = table[key]
    base, (M, N, K, taps, stride, ups), hw = parse_key(key)
    if taps not in (1, 9) or K % taps or stride not in (1, 2) or ups not in (0, 1) or (taps == 1 and (stride != 1 or ups or hw)):
        raise ValueError(f"tuning table key {key!r}: not a linear layer or a 3x3 convolution this sweep knows how to launch")
    Cin = K // taps
    out = []

    def add(form, cfg, split, B, Hin, Win, Hout, Wout, rowvec=False, gn_groups=0):
        out.append(Case(f"{key}/{form}", key, M, N, K, Cin, taps, stride, ups, B, Hin, Win, Hout, Wout, form, cfg, split, rowvec, gn_groups,
                        taps == 9 and hw is None))

    if taps == 1:
        add("split", ent["cfg"], ent["split"], M, 1, 1, 1, 1)
        if (ent["cfg_nosplit"], 1) != (ent["cfg"], ent["split"]):
            if N % 8:
                raise ValueError(f"tuning table key {key!r}: cfg_nosplit differs from cfg but N % 8 != 0 leaves no GEGLU form to reach it")
            add("geglu", ent["cfg_nosplit"], 1, M, 1, 1, 1, 1)
        if N == 3 * K:
            if K % HEADS:
                raise ValueError(f"tuning table key {key!r}: a q/k/v projection whose width does not split into {HEADS} heads")
            B = 1 if M % 2 else 2
            add("heads", ent["cfg_nosplit"], 1, B, M // B, 1, M // B, 1)
        return out
    Ho, Wo = hw if hw else off_table_map(table, base)
    if M % (Ho * Wo) or (ups and (Ho % 2 or Wo % 2)):
        raise ValueError(f"tuning table key {key!r}: {M} rows are not whole {Ho}x{Wo} maps" + (" of even size" if ups else ""))
    Hin, Win = input_map(Ho, Wo, stride, ups)
    add("split", ent["cfg"], ent["split"], M // (Ho * Wo), Hin, Win, Ho, Wo, rowvec=stride == 1, gn_groups=GN_GROUPS if stride == 1 and N % GN_GROUPS == 0 else 0)
    return out


def cases(table):
    out = []
    for key in table:
        got = cases_of(table, key)
        if not got:
            raise ValueError(f"tuning table key {key!r} produced no case")
        out += got
    return out


def lookup_key(table, M, N, K, taps, stride, ups, Hout, Wout):
    """The table key ``ops.conv_gemm`` finds for a problem (with the map first, then plain), or None."""
    base = f"{M},{N},{K},{taps},{stride},{int(ups)}"
    if taps == 9 and f"{base}|{Hout}x{Wout}" in table:
        return f"{base}|{Hout}x{Wout}"
    return base if base in table else None


def load_table():
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(os.path.dirname(here), "imagdressing_amd", "gemm_tuning.json")) as f:
        return json.load(f)["shapes"]
