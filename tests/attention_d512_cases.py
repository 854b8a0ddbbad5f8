"""The exact attention problems of tests/attention_exact_cases.py at head dim 512 (attention_d512.hip; the case list only -- the builders there are
generic in D).  Used by tests/test_attention_d512_gpu.py and, for the preconditions, by tests/test_attention_d512_inputs.py.

  count (c = -8 and 0) and weighted at every key count of LS and at 1345 keys (43 tiles of 32 keys, ragged by one), query counts 33 / 70 / 130 /
  128 (ragged 128-row workgroups, a wave with no rows at all, one exact multiple), (batch, heads) alternating between (3, 1) -- the VAE's single
  head -- and (2, 2), every third case with K / V shared by two batch entries;
  one staircase case (scores that climb or fall by whole 64-key units: the running maximum moves at every second tile, O is rescaled);
  three cases past the 16384 columns imd_softmax_rows takes: 16449 keys = 514 tiles and one key.

The staircase family is not used at long L: its K holds j // 64, and 257 is not a bf16 number."""
from tests import attention_exact_cases as ac

D = 512
LIMIT_L = 16449                                            # 257 x 64 + 1: past imd_softmax_rows' 16384 columns, ragged by one key
FORM = "d512"


def _cases():
    out = []
    for li, L1 in enumerate(ac.LS + (ac.L_LONG,)):
        for fi, (fam, c) in enumerate(ac.FAMILIES):
            n = li + fi
            B, H = (3, 1) if n % 2 == 0 else (2, 2)
            out.append(ac._case(FORM, fam, D, B, H, ac.GENERIC_N[n % 4], L1, bdiv1=2 if n % 3 == 0 else 1, c=c))
    out.append(ac._case("staircase", "staircase", D, 2, 2, 130, 640))
    for fam, c in ac.FAMILIES:
        out.append(ac._case(FORM, fam, D, 1, 1, 70, LIMIT_L, c=c))
    return out


CASES = _cases()
