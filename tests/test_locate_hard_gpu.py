"""The cut-out search on the GPU (ssw_locate_rgb8, ssw_locate_scaled_rgb8) on the hard cases of tests/locate_cases.py:
tie-heavy and saturated frames at the edges of the coarse kernel's template chunk, of its candidate tile and of the eight rounds
of the top-k.  Every answer must EQUAL the numpy restatement of the definition (tests/test_locate_cpu.py: locate_ref,
tests/test_locate_scale_cpu.py: locate_scaled_ref) -- integers, no tolerance, no case left out -- and, where the content decides
the answer (locate_cases.truth, confirmed by tests/test_locate_hard_cpu.py), that answer."""
import numpy as np
import pytest

import gpu_util as G
import locate_cases as LC
import spread_spectrum_watermarking_amd as wm
from spread_spectrum_watermarking_amd.api import Locate
from test_locate_gpu import check_against_ref
from test_locate_scale_cpu import height_of, locate_scaled_ref

pytestmark = pytest.mark.gpu

# the content of each table on which three suspects are also searched alone
ALONE = {"A": "periodic", "B": "rows", "C": "columns", "D": "periodic", "E": "flat", "F": "rows"}


def answer(g):
    return g.placement.x, g.placement.y, g.sad


def three(n):
    return sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("table,W,H,content", LC.ids(), ids=lambda v: str(v))
def test_tables_a_to_f_equal_the_restatement(table, W, H, content):
    base, sus = LC.case(table, W, H, content)
    got = check_against_ref(base, [s.pixels for s in sus], what="%s %dx%d %s" % (table, W, H, content))
    for s, g in zip(sus, got):
        want = LC.truth(content, s)
        if want is not None:
            assert answer(g) == want, (s.name, s.rect)
    if content == ALONE[table] or table == "F":                       # each alone gives what the batch gave (F: 2 suspects per content)
        for i in three(len(sus)):
            assert wm.locate(base, [sus[i].pixels], ctx=G.ctx())[0] == got[i], sus[i].name


@pytest.mark.parametrize("content", LC.G_CONTENTS)
def test_table_g_resized_suspects_of_known_size(content):
    """Both coarse factors in one call, every suspect through the restore resize first."""
    base, sus = LC.case_g(content)
    got = check_against_ref(base, [s.pixels for s in sus], [s.size for s in sus], "G " + content)
    assert got[-1] == got[len(LC.G_SCALES)]                           # alpha is ignored, through the resize too
    for i in three(len(sus)):
        assert wm.locate(base, [sus[i].pixels], [sus[i].size], ctx=G.ctx())[0] == got[i], sus[i].name


@pytest.mark.parametrize("name", list(LC.LADDER))
@pytest.mark.parametrize("content", LC.LADDER_CONTENTS)
def test_the_scale_ladder_equals_the_restatement(content, name):
    base, s, lo, hi, (x, y, pw, ph) = LC.ladder_case(content, name)
    want, rungs, keep = locate_scaled_ref(base, s, lo, hi, details=True)
    g = wm.locate(base, [s], [Locate(widths=(lo, hi))], ctx=G.ctx())[0]
    have = (g.placement.w, g.placement.h, g.placement.x, g.placement.y, g.sad)
    print(content, name, "cut", (pw, ph, x, y), "gpu", have, "numpy", want, "kept rungs", keep, "of", len(rungs))
    assert have == want and g.mean_abs_diff == g.sad / (want[0] * want[1])
    if content == "flat":
        # every rung has D = 0 at every position: the kept rungs are the first 8 by index (D_a n_b = D_b n_a: ties to the
        # smaller j), each answers (0, 0), and among the refined widths of equal SAD / (pw ph) = 0 the smallest, wmin, wins
        assert keep == list(range(min(8, len(rungs)))) and all(r[2:5] == (0, 0, 0) for r in rungs)
        assert want == (lo, height_of(lo, s.shape[1], s.shape[0]), 0, 0, 0)
    if content in ("noise", "binary"):                                # the truth, resized or not; an exact cut-out with SAD 0
        assert want[:4] == (pw, ph, x, y) and (want[4] == 0) == (LC.LADDER[name][1] is None)
    if name == "129x65 unscaled" and content in ("periodic", "rows", "columns"):
        # exact ties inside the windows of the refinement: the first (y, x) of the cut's shifts / of the tied line
        assert want == (pw, ph) + {"periodic": (x % 16, y % 8), "rows": (0, y), "columns": (x, 0)}[content] + (0,)


def test_a_large_search_leaves_nothing_behind_for_a_small_one():
    """Table F's call (1 085 349 candidates, D of 4.3 MB, every key slot filled), then table E's (1 to 9 candidates, key slots
    left empty) on the same context: the answers of a fresh context."""
    big_base, big = LC.case("F", 1100, 1000, "flat")
    small = [LC.case("E", W, H, "flat") for W, H in LC.bases("E")]
    ctx = G.ctx()
    wm.locate(big_base, [s.pixels for s in big], ctx=ctx)
    after = [wm.locate(base, [s.pixels for s in sus], ctx=ctx) for base, sus in small]
    with G.fresh_ctx() as fresh:
        alone = [wm.locate(base, [s.pixels for s in sus], ctx=fresh) for base, sus in small]
    assert after == alone
    for (base, sus), got in zip(small, after):
        for s, g in zip(sus, got):
            if s.variant == "exact":
                assert answer(g) == (0, 0, 0)
