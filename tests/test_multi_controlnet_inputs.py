"""Preconditions of the imd_residual_mix_rows comparison, without a GPU: the case data and scale patterns are what the GPU tests assume,
and the comparison against the CPU expression is SENSITIVE -- each mistake a kernel or a host plan could make changes at least one 16-bit
element of the case data, in both element types.  A kernel that made one of them could therefore not pass ``torch.equal``."""
import pytest
import torch

from tests import multi_controlnet_cases as M
from tests.control_rows_cases import ONE, SD15_8x8, SIXTEEN, segment_views

SHAPES = {"ONE": ONE, "SIXTEEN": SIXTEEN, "SD15_8x8": SD15_8x8}


def _sources(row_elems, rows, dtype, K):
    """per source ONE [rows, sum of the segments] tensor: the segments side by side (an element's row and source are what matter)"""
    return [torch.cat(segment_views(b, rows), dim=1) for b in M.source_buffers(row_elems, rows, dtype, K)]


def _differs(a, b):
    return int((M.bits(a) != M.bits(b)).sum())


@pytest.mark.parametrize("name,dtype", M.DTYPES)
def test_the_contract_is_the_issue_expression(name, dtype):
    """``mix`` == the chain of x.float() * torch.tensor(s, dtype=float32) and + written out by hand, a skipped source skipped"""
    g = torch.Generator().manual_seed(3)
    x = [(torch.randn(2, 64, generator=g) * 2).to(dtype) for _ in range(3)]
    s = [[0.7, 0.0], [1.3, -0.45], [0.0, 0.9]]
    f = lambda v: torch.tensor(v, dtype=torch.float32)          # noqa: E731
    row0 = (x[0][0].float() * f(0.7) + x[1][0].float() * f(1.3)).to(dtype)
    row1 = (x[1][1].float() * f(-0.45) + x[2][1].float() * f(0.9)).to(dtype)
    assert torch.equal(M.bits(M.mix(x, s)), M.bits(torch.stack([row0, row1])))
    assert torch.equal(M.bits(M.mix(x, [[0.0] * 2] * 3)), torch.zeros(2, 64, dtype=torch.int16))          # all skipped: +0
    assert torch.equal(M.bits(M.mix(x, [[0.0] * 2, [1.0] * 2, [0.0] * 2])), M.bits(x[1]))                  # exactly 1.0: the source's bits


@pytest.mark.parametrize("name,dtype", M.DTYPES)
def test_case_data_is_finite_and_the_sources_differ(name, dtype):
    for shape in SHAPES.values():
        src = _sources(shape, 3, dtype, M.MAX_SOURCES)
        assert all(bool(torch.isfinite(x.float()).all()) for x in src)
        for a in range(M.MAX_SOURCES):
            for b in range(a + 1, M.MAX_SOURCES):
                assert _differs(src[a], src[b]) > src[a].numel() // 2
        out = M.mix(src, [[M.OPEN[k]] * 3 for k in range(M.MAX_SOURCES)])
        assert bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("rows", [1, 3, 4])
def test_scale_patterns_are_what_the_kernel_tests_assume(K, rows):
    pats = dict(M.scale_patterns(K, rows))
    assert set(pats) == {"open", "all_zero", "negative", "per_row"} | {f"zero{k}" for k in range(K)} | {f"one{k}" for k in range(K)}
    for name, sc in pats.items():
        assert len(sc) == K and all(len(r) == rows for r in sc), name
    assert all(v != 0.0 for r in pats["open"] for v in r)
    assert all(v < 0.0 for r in pats["negative"] for v in r)
    assert all(v == 0.0 for r in pats["all_zero"] for v in r)
    for k in range(K):
        assert [pats[f"zero{k}"][j][0] == 0.0 for j in range(K)] == [j == k for j in range(K)]
        assert [pats[f"one{k}"][j][0] for j in range(K)] == [1.0 if j == k else 0.0 for j in range(K)]
    cols = [tuple(pats["per_row"][k][r] for k in range(K)) for r in range(rows)]
    assert len(set(cols)) == rows                                  # a different pattern in every row
    if K > 1:
        assert all(cols[r][r % K] == 0.0 and sum(v == 0.0 for v in cols[r]) == 1 for r in range(rows))


@pytest.mark.parametrize("name,dtype", M.DTYPES)
@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_crafted_block_is_found(name, dtype, K):
    fma = M.crafted_block(dtype, K, M.wrong_fma)
    assert fma.shape == (K, M.CRAFT_KEEP)
    srcs, sc = [fma[k:k + 1] for k in range(K)], [[M.OPEN[k]] for k in range(K)]
    assert _differs(M.wrong_fma(srcs, sc), M.mix(srcs, sc)) == M.CRAFT_KEEP          # every column shows a contracted evaluation
    if K >= 3:
        order = M.crafted_block(dtype, K, M.wrong_order)
        assert order.shape == (K, M.CRAFT_KEEP)
        srcs = [order[k:k + 1] for k in range(K)]
        assert _differs(M.wrong_order(srcs, sc), M.mix(srcs, sc)) == M.CRAFT_KEEP
    sp = M.specials(dtype, K)
    assert sp.shape == (K, M.CRAFT_KEEP * (2 if K >= 3 else 1)) and bool(torch.isfinite(sp.float()).all())


MISTAKES = [("dropped", M.wrong_dropped, 2), ("twice", M.wrong_twice, 1), ("transposed", M.wrong_transposed, 2),
            ("order", M.wrong_order, 3), ("fma", M.wrong_fma, 2)]


@pytest.mark.parametrize("name,dtype", M.DTYPES)
@pytest.mark.parametrize("shape", ["SIXTEEN", "SD15_8x8"])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_every_mistake_changes_the_result(name, dtype, shape, K):
    """on the data and patterns of the GPU tests (rows = 3; SIXTEEN and SD15_8x8 hold the whole crafted block): the arithmetic
    mistakes under the "open" pattern, the indexing mistakes under "per_row" """
    rows = 3
    src = _sources(SHAPES[shape], rows, dtype, K)
    pats = dict(M.scale_patterns(K, rows))
    for what, wrong, k_min in MISTAKES:
        if K < k_min:
            continue
        sc = pats["per_row"] if what == "transposed" else pats["open"]
        assert _differs(wrong(src, sc), M.mix(src, sc)) > 0, (what, K)
    if K >= 2:          # a gated source must be skipped, not multiplied by 0: with a NaN in it the two differ
        poisoned = [x.clone() for x in src]
        poisoned[0][:, 0] = float("nan")
        sc = pats["zero0"]
        assert bool(torch.isfinite(M.mix(poisoned, sc).float()).all())


@pytest.mark.parametrize("name,dtype", M.DTYPES)
@pytest.mark.parametrize("K", [1, 2, 4])
def test_the_uncond_half_mistake_changes_the_result(name, dtype, K):
    """rows = 2B as a pipeline lays them out (request_scales): uncond row B + j given the scale of cond row j + 1"""
    B = 2
    src = _sources(SD15_8x8, 2 * B, dtype, K)
    sc = M.request_scales(B, K)
    assert all(r[:B] == r[B:] and len(set(r[:B])) == B for r in sc)
    assert _differs(M.wrong_uncond_neighbour(src, sc), M.mix(src, sc)) > 0


def test_the_hand_written_table_is_consistent():
    assert len(M.TABLE_ROWS) == 2 and all(len(net) == 3 and all(len(r) == M.TABLE_STEPS for r in net) for net in M.TABLE_ROWS)
    assert M.TABLE_ROWS[0][0][2] == 0.0 and M.TABLE_ROWS[0][0][3] == 0.5          # net 0 opens late
    assert M.TABLE_ROWS[1][2][4] == 2.0 and M.TABLE_ROWS[1][2][5] == 0.0          # net 1 closes early for request 2
