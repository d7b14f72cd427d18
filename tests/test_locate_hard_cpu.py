"""The hard cases of the cut-out search (tests/locate_cases.py) without a GPU: that every table reaches the edge it is there
for -- worked out with the constants read from csrc/locate.hip, the way plan_items, coarse_desc and locate_coarse_kernel work
them out, so a changed LOC_TX, LOC_TY, LOC_JB, LOC_KW, LOC_TOP or top-k grid fails here instead of silently moving the edge
away from the table -- and the tie structure of every content, by the restatement (tests/test_locate_cpu.py: locate_ref)
alone.  tests/test_locate_hard_gpu.py holds the device to the same cases."""
import numpy as np
import pytest

import locate_cases as LC
from test_locate_cpu import locate_ref, luma

C = LC.constants()
TX, TY, JB, KW, TOP, BATCH = C["LOC_TX"], C["LOC_TY"], C["LOC_JB"], C["LOC_KW"], C["LOC_TOP"], C["LOC_BATCH"]
CW = LC.chunk_bytes()                 # template bytes per LDS chunk row


def plans(table):
    return [LC.plan(*e) for e in LC.TABLES[table]]


# ---- the boundary claims of the tables -------------------------------------------------------------------------------------------
def test_the_constants_are_read_from_the_source():
    assert TX == 64 and TY == 4 * C["LOC_YPL"]                                   # a lane per x; 4 waves of LOC_YPL y positions
    assert CW == 4 * KW and C["TOPK_PER_BLOCK"] % 256 == 0 and TOP == 8        # locate_ref rescoring 8


def test_table_a_reaches_the_template_chunk_edges_at_f1():
    ps = plans("A")
    assert all(p.f == 1 and (p.tw, p.th) == e[2:] for p, e in zip(ps, LC.TABLES["A"]))
    tws, ths = {p.tw for p in ps}, {p.th for p in ps}
    assert {tw % 4 for tw in tws} == {0, 1, 2, 3}                                # byte masks of 1, 2, 3 bytes and a whole last word
    assert {1, 2, 3, 4, 5} <= tws                                                # the mask in the chunk's first word, and the word after it
    assert {-1, 0, 1} <= {tw - CW for tw in tws} and {-1, 0, 1} <= {tw - 2 * CW for tw in tws}
    assert {CW - 3, CW + 3, 2 * CW + 3} <= tws                                   # 61, 67, 131: the other two masks at a chunk edge
    assert 1 in ths and {-1, 0, 1} <= {th - JB for th in ths} and {0, 1} <= {th - 2 * JB for th in ths}
    assert {-1, 0} <= {th - 8 * JB for th in ths} and {0, 1, JB - 1} <= {th % JB for th in ths}      # skipped rows: 7 and 1 of 8 left
    full = [p.tw >= CW and p.th >= JB for p in ps]                               # a search that takes locate_chunk<false> at all
    assert any(full) and not all(full)
    assert any(p.tw % CW == 0 and p.th % JB == 0 for p in ps)                    # ... and nothing else: (64, 8), (128, 16)
    assert any(f and p.tw % CW and p.th % JB for f, p in zip(full, ps))          # whole chunks, a masked column of chunks AND a masked row of them
    assert 2 * len(ps) > BATCH                                                  # exact + noisy: two launches of descriptors


def test_table_b_reaches_the_template_chunk_edges_at_f4():
    ps = plans("B")
    assert all(p.f == 4 and (p.tw, p.th) == (e[2] // 4, e[3] // 4) for p, e in zip(ps, LC.TABLES["B"]))
    assert all(e[0] % 4 == 3 for e in LC.TABLES["B"]) and len(LC.bases("B")) == 1
    tws, ths = {p.tw for p in ps}, {p.th for p in ps}
    assert tws == {KW, KW + 1, CW - 1, CW, CW + 1}                               # 16 words of 4 box means = one chunk row
    assert ths == {2 * JB, 2 * JB + 1}
    assert {tw % 4 for tw in tws} == {0, 1, 3}
    assert {e[2] % 4 for e in LC.TABLES["B"]} == {0, 3} and {e[3] % 4 for e in LC.TABLES["B"]} == {0, 3}     # pixels no box covers
    assert all(len({(nxp, nyp) for _, _, nxp, nyp in p.phases}) > 1 for p in ps if p.nx % 4 or p.ny % 4)


def test_table_c_reaches_the_candidate_tile_edges_at_f1():
    ps = plans("C")
    assert all(p.f == 1 and (p.tw, p.th) == (16, 16) for p in ps)
    assert [(p.nx - TX, p.ny - TY) for p in ps] == [(-1, -1), (0, 0), (1, 1), (TX + 1, TY + 1), (0, 1), (1, 0)]
    assert [(p.tiles_x, p.tiles_y) for p in ps] == [(1, 1), (1, 1), (2, 2), (3, 3), (1, 2), (2, 1)]
    assert all(p.phases == [(0, 0, p.nx, p.ny)] for p in ps)


def test_table_d_reaches_the_candidate_tile_edges_at_f4_with_uneven_phases():
    ps = plans("D")
    assert all(p.f == 4 and (p.tw, p.th) == (16, 16) and len(p.phases) == 16 for p in ps)
    cols = [sorted({nxp - TX for _, _, nxp, _ in p.phases}) for p in ps]
    rows = [sorted({nyp - TY for _, _, _, nyp in p.phases}) for p in ps]
    assert cols == [[-1, 0], [0], [0, 1], [1], [1, 2], [0, 1], [0]]               # 63 | 64, 64, 64 | 65, 65, 65 | 66 columns of candidates
    assert rows == [[-1, 0], [0], [0, 1], [1], [1, 2], [0], [0, 1]]               # 31 | 32, 32, 32 | 33, 33, 33 | 34 rows
    assert [(p.tiles_x, p.tiles_y) for p in ps] == [(1, 1), (1, 1), (2, 2), (2, 2), (2, 2), (2, 1), (1, 2)]
    # the grid is sized by phase 0: a phase with a tile fewer returns early from the blocks that have no candidate
    idle = [sum((p.tiles_x - 1) * TX >= nxp or (p.tiles_y - 1) * TY >= nyp for _, _, nxp, nyp in p.phases) for p in ps]
    assert idle == [0, 0, 15, 0, 0, 12, 12]
    for p in ps:                                                                 # the phases cover every candidate once
        assert sum(nxp * nyp for _, _, nxp, nyp in p.phases) == p.nx * p.ny


def test_table_e_counts_candidates_around_the_rounds_of_the_top_k():
    es, ps = LC.TABLES["E"], plans("E")
    assert [p.f for p in ps] == [1] * 7 + [4] * 7 and len(LC.bases("E")) == 2
    for half in (ps[:7], ps[7:]):
        assert [p.nx * p.ny - TOP for p in half] == [1 - 8, 2 - 8, 3 - 8, -1, 0, 1, 1]       # key slots left at LOC_NONE: 7, 6, 5, 1, 0
        assert [(p.nx, p.ny) for p in half[-2:]] == [(9, 1), (3, 3)]                         # 9 in a row, 9 in a square
        assert (half[0].nx, half[0].ny) == (1, 1)
    assert all(min(e[2:]) >= 64 for e in es[7:]) and all(min(e[2:]) < 64 for e in es[:7])


def test_table_f_has_more_candidates_than_one_sweep_of_the_top_k_grid():
    (p,) = plans("F")
    sweep = C["TOPK_BLOCKS"] * C["TOPK_PER_BLOCK"]
    assert sweep < p.nx * p.ny < 2 * sweep and p.nx * p.ny > C["TOPK_BLOCKS"] * 256 * 8      # a grid-stride loop of 9 steps
    assert LC.TABLE_CONTENTS["F"] == ("flat", "rows", "noise") and p.f == 1


def test_table_g_resizes_to_both_coarse_factors_through_the_clamp():
    from oracle import oracle as O
    W, H = LC.G_BASE
    assert sorted(LC.plan(W, H, *t).f for t in LC.G_TARGETS) == [1, 4]
    for content in LC.G_CONTENTS:
        base, sus = LC.case_g(content)
        assert len(sus) == 7 and sus[-1].pixels.shape[2] == 4 and np.array_equal(sus[-1].pixels[..., :3], sus[3].pixels)
        for s in sus:
            pw, ph = s.size
            assert (s.pixels.shape[1], s.pixels.shape[0]) in ((pw // 2, ph // 2), (2 * pw, 2 * ph), (3 * pw // 2, 3 * ph // 2))
    base, sus = LC.case_g("binary")
    for s in sus[:6]:                                                            # both ends of the clamp are reached on the way back
        back = O.resize_rgb8(s.pixels, *s.size)
        assert back.min() == 0 and back.max() == 255 and len(np.unique(back)) > 2


def test_every_id_once_and_batches_of_both_sizes():
    ids = LC.ids()
    assert len(ids) == len(set(ids)) == 9 * (1 + 1 + 6 + 7 + 2) + 3
    n = {t: sum(len(LC.case(*i)[1]) for i in ids if i[0] == t) for t in LC.TABLES}
    print("answers per table", n)
    assert n == {"A": 7 * 34 + 2 * 17, "B": 7 * 18 + 2 * 9, "C": 6 * 16, "D": 7 * 16, "E": 2 * (7 * 14 + 2 * 7), "F": 6}


# ---- the tie structure of the contents, by the restatement alone ------------------------------------------------------------------
def one(table, content, size):
    base, sus = LC.case(*[i for i in LC.ids() if i[0] == table and i[3] == content][0])
    return base, [s for s in sus if s.rect[2:] == size]


@pytest.mark.parametrize("table,size", [("A", (129, 17)), ("B", (71, 68))], ids=["A 129x17", "B 71x68"])
@pytest.mark.parametrize("content", LC.CONTENTS + LC.FOREIGN)
def test_each_content_decides_the_answer_as_stated(content, table, size):
    base, sus = one(table, content, size)
    assert sus and sus[0].variant in ("exact", "foreign")
    s = sus[0]
    x, y, pw, ph = s.rect
    want = LC.truth(content, s)
    gx, gy, sad, d2 = locate_ref(base, s.pixels, details=True)
    print(table, content, s.rect, "->", (gx, gy, sad), "two smallest D", d2)
    assert want is not None and (gx, gy, sad) == want
    H, W = base.shape[:2]
    if content == "flat":
        assert want == (0, 0, 0) and tuple(d2) == (0, 0)
    elif content == "periodic":
        assert want == (x % 16, y % 8, 0) and tuple(d2) == (0, 0)
        ties = ((W - pw - x % 16) // 16 + 1) * ((H - ph - y % 8) // 8 + 1)       # the shifts of the cut that fit the frame
        assert ties > TOP                                                        # the top 8 are chosen by index alone
    elif content == "rows":
        assert want == (0, y, 0) and tuple(d2) == (0, 0) and W - pw + 1 > TOP
    elif content == "columns":
        assert want == (x, 0, 0) and tuple(d2) == (0, 0) and H - ph + 1 > TOP
    elif content in LC.FOREIGN:
        assert want == (0, 0, 255 * pw * ph) == (0, 0, int(np.abs(luma(s.pixels) - luma(base[:ph, :pw])).sum()))
        assert d2[0] == d2[1] == 255 * LC.plan(W, H, pw, ph).tw * LC.plan(W, H, pw, ph).th    # every candidate at the largest D
    else:
        assert want == (x, y, 0) and d2[0] == 0 < d2[1]                          # a photograph's case: no tie
    if len(sus) > 1:                                                             # the noisy cut: the same ties at a non-zero difference
        n = locate_ref(base, sus[1].pixels, details=True)
        print(table, content, "noisy ->", n[:3], "two smallest D", n[3])
        assert n[2] > 0
        if content in ("flat", "rows", "columns", "periodic"):
            assert n[3][0] == n[3][1] > 0
        if content == "flat":
            assert n[:2] == (0, 0)


@pytest.mark.parametrize("table", ["C", "E"])
def test_the_rules_hold_on_every_case_of_the_small_tables(table):
    """Tables C and E are cheap enough to run whole: every suspect for which locate_cases.truth states an answer gets it."""
    stated = 0
    for i in LC.ids():
        if i[0] != table:
            continue
        base, sus = LC.case(*i)
        for s in sus:
            want = LC.truth(i[3], s)
            if want is not None:
                stated += 1
                assert locate_ref(base, s.pixels) == want, (i, s.name, s.rect)
    assert stated >= len(LC.bases(table)) * 9


@pytest.mark.parametrize("content", ["flat", "periodic", "noise", "binary"])
def test_the_expectations_recorded_with_the_cases(content):
    """A 129 x 63 cut at (37, 21) of a 320 x 192 base: flat answers (0, 0, 0), periodic (37 mod 16, 21 mod 8, 0) = (5, 5, 0),
    noise and binary the truth."""
    base = LC.frame(content, 192, 320, seed=1)
    got = locate_ref(base, LC.cut(base, 37, 21, 129, 63))
    assert got == {"flat": (0, 0, 0), "periodic": (5, 5, 0)}.get(content, (37, 21, 0))


def test_contents_and_variants_are_what_they_say():
    for kind in LC.CONTENTS:
        a = LC.frame(kind, 37, 53, seed=3)
        assert a.shape == (37, 53, 3) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]
        assert np.array_equal(a, LC.frame(kind, 37, 53, seed=3))
    from test_jpeg_cpu import content
    for kind in ("noise", "binary", "cat+noise"):
        assert np.array_equal(LC.frame(kind, 37, 53, 3), content(kind, 37, 53, 3))
    assert len(np.unique(LC.frame("flat", 9, 9).reshape(-1, 3), axis=0)) == 1
    p = LC.frame("periodic", 40, 50)
    assert np.array_equal(p[8:, 16:], p[:-8, :-16]) and not np.array_equal(p[4:], p[:-4]) and not np.array_equal(p[:, 8:], p[:, :-8])
    r, c = LC.frame("rows", 40, 50), LC.frame("columns", 40, 50)
    assert (r == r[:, :1]).all() and len(np.unique(luma(r)[:, 0])) > 20 and (c == c[:1]).all() and len(np.unique(luma(c)[0])) > 20
    cut = LC.cut(p, 3, 5, 20, 10)
    d = LC.noisy(cut, 1).astype(int) - cut
    assert d.min() >= -2 and d.max() <= 2 and d.any() and not np.array_equal(LC.noisy(cut, 1), LC.noisy(cut, 2))
    base, sus = LC.case("A", 200, 150, LC.FOREIGN[0])
    assert not base.any() and all((s.pixels == 255).all() for s in sus)
    base, sus = LC.case("A", 200, 150, LC.FOREIGN[1])
    assert (base == 255).all() and not any(s.pixels.any() for s in sus)
    for t in LC.TABLES:                                                          # every cut lies inside its base
        for W, H, pw, ph in LC.TABLES[t]:
            x, y = LC.position(t, W, H, pw, ph)
            assert 0 <= x <= W - pw and 0 <= y <= H - ph
