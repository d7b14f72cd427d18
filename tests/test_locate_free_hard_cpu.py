"""The hard cases of the free-aspect rescoring (tests/locate_free_cases.py), the parts that need no GPU: what the tables claim
to reach -- the tiles `free_pick_tile` gives every item (tests/cpp/locate_free_plan_test.cpp, built with hipcc and run on the
host), the edges of those tiles, the window classes of `free_window` -- is pinned here, and the answers that the content decides
are confirmed with the restatement alone (locate_free_ref(..., start=..., details=True)), so tests/test_locate_free_hard_gpu.py
compares the device with something that was checked without it."""
import ctypes as C
import os

import numpy as np
import pytest

import locate_cases as LC
import locate_free_cases as FC
from conftest import ROOT
from spread_spectrum_watermarking_amd import _lib as L
from test_locate_free_cpu import free_window

# every (oyb, oxb) the resized items of the tables get; the plain front's 32 x 64 comes on top
RESIZE_TILES = {(8, 32), (16, 32), (32, 32), (64, 32), (16, 64), (32, 64), (64, 64), (16, 128), (32, 128), (64, 128)}
PLAIN_TILE = (32, 64)
X_CLASSES = {"pw % oxb == 0", "pw % oxb == 1", "nox % 4 == 1", "nox % 4 == 2", "nox % 4 == 3"}
Y_CLASSES = {"ph % oyb == 0", "ph % oyb == 1"}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """{case name: [Tile per item]} of every case, from one build and one run of the host program."""
    return FC.tiles(FC.build_plan_program(tmp_path_factory.mktemp("plan")), FC.CASES)


def test_the_tables_are_what_they_say():
    assert {t: len(FC.names(t)) for t in "TWX"} == {"T": 19, "W": 53, "X": 24}
    for c in FC.CASES:
        base, s = FC.pixels(c.name)
        assert base.shape == (c.H, c.W, 3) and s.shape == (c.size[1], c.size[0], c.channels)
        assert c.W <= 300 and c.H <= 200
        assert max(c.size) <= 136 or c.name == "T 64x32 x4 rgba noise"                    # the one suspect of 256 x 128
    t = [c for c in FC.CASES if c.table == "T"]
    assert {c.start[:2] for c in t} == {(36, 36), (64, 64), (128, 64), (128, 128), (64, 32)} and all(c.slack == 4 for c in t)
    assert {c.channels for c in t} == {3, 4} and {c.variant for c in t} == {"exact", "noisy", "resized"}
    assert sum(c.rect != (c.start[2], c.start[3]) + c.start[:2] for c in t) >= 8            # starts off the truth
    for size in {c.start[:2] for c in t}:                                                   # the plain front is one item of the 81
        assert any(c.size == size for c in t if c.start[:2] == size) or size == (64, 32)
    w = [c for c in FC.CASES if c.table == "W"]
    assert {c.W % 4 for c in w if c.H > 32} == {0, 1, 2, 3}
    for r in range(4):
        on = [c for c in w if c.W % 4 == r and c.H > 32]
        assert {c.slack for c in on} == {1, 2, 3, 4}
        W, H = on[0].W, on[0].H
        pw0, ph0 = on[0].start[:2]
        assert {c.start[2] for c in on if c.start[:2] == (pw0, ph0)} >= {0, 3, 4, W - pw0 - 3, W - pw0}
        assert {c.start[3] for c in on if c.start[:2] == (pw0, ph0)} >= {0, 3, 4, H - ph0 - 3, H - ph0}
        assert {c.start[2:] for c in on} >= {(0, 0), (W - pw0, 0), (0, H - ph0), (W - pw0, H - ph0)}
        assert any(c.start[0] == W for c in on) and any(c.start[1] == H for c in on) and any(c.start[1] == 33 for c in on)
        one_width = [c for c in on if c.wmin == c.wmax == c.start[0]]
        assert one_width and all(len(FC.items(c)) == 9 for c in one_width)
    x = [c for c in FC.CASES if c.table == "X"]
    assert {c.content for c in x} == set(FC.CONTENTS) and len(FC.CONTENTS) == 8
    assert all({(c.size == c.start[:2], c.channels) for c in x if c.content == k} == {(True, 3), (False, 3), (False, 4)} for k in FC.CONTENTS)
    one = FC.BY_NAME["W 160x32 one size, one position"]
    assert [(pw, ph, w) for pw, ph, w in FC.items(one)] == [(160, 32, (0, 0, 0, 0))]
    assert {pw % 4 for c in t for pw, _, _ in FC.items(c)} == {0, 1, 2, 3}


def test_the_tiles_the_tables_reach(plan):
    """Every (oyb, oxb) that occurs is listed; per distinct oxb and per distinct oyb the tables hold the edges at which a
    tile's last word, last column and last row go wrong.  A single-tile item needs pw <= oxb and ph <= oyb with both sides
    >= 32: no tile of 8 or 16 rows can be one (ph >= 32 > oyb), so that class is pinned for every oxb and for oyb in {32, 64}; the
    one of 32 columns is the 126 x 36 suspect scored at 32 x 32.  RESIZE_TILES is what the tables reach, not all the picker has:
    a suspect four times as wide as its size gets 16 columns, which neither the tables nor the issue's list hold."""
    pairs, plain = set(), set()
    by_oxb, by_oyb = {}, {}
    for c in FC.CASES:
        for (pw, ph, _), t in zip(FC.items(c), plan[c.name]):
            assert t.tiles_x == -(-pw // t.oxb) and t.tiles_y == -(-ph // t.oyb) and t.lds <= 80 * 1024
            (plain if c.size == (pw, ph) else pairs).add((t.oyb, t.oxb))
            cx, cy = by_oxb.setdefault(t.oxb, set()), by_oyb.setdefault(t.oyb, set())
            nox = pw % t.oxb or t.oxb                                              # columns of the last tile of a row
            cx.update(k for k, hit in (("pw % oxb == 0", pw % t.oxb == 0), ("pw % oxb == 1", pw % t.oxb == 1), ("nox % 4 == 1", nox % 4 == 1),
                                       ("nox % 4 == 2", nox % 4 == 2), ("nox % 4 == 3", nox % 4 == 3)) if hit)
            cy.update(k for k, hit in (("ph % oyb == 0", ph % t.oyb == 0), ("ph % oyb == 1", ph % t.oyb == 1)) if hit)
            for k, hit in (("single tile", t.tiles_x == 1 and t.tiles_y == 1), ("2 x 2 tiles or more", t.tiles_x >= 2 and t.tiles_y >= 2)):
                if hit:
                    cx.add(k); cy.add(k)
    print("resized", sorted(pairs), "plain", sorted(plain))
    print({k: sorted(v) for k, v in by_oxb.items()}, {k: sorted(v) for k, v in by_oyb.items()})
    assert pairs == RESIZE_TILES and plain == {PLAIN_TILE} and len(RESIZE_TILES) >= 6
    assert set(by_oxb) == {32, 64, 128} and set(by_oyb) == {8, 16, 32, 64}
    for oxb, got in by_oxb.items():
        assert got >= X_CLASSES | {"2 x 2 tiles or more"} | {"single tile"}, (oxb, sorted(got))
    for oyb, got in by_oyb.items():
        assert got >= Y_CLASSES | {"2 x 2 tiles or more"} | ({"single tile"} if oyb >= 32 else set()), (oyb, sorted(got))


def test_the_windows_the_tables_reach():
    """nwx and nwy of 1, 5 and 9, and clipping at each of the four edges for each W mod 4.  An EMPTY window is not among them
    and cannot be: x0 <= W - pw0 and pw <= pw0 + 4 give W - pw >= x0 - 4, so a start that the ladder can answer (and the
    diagnostic accepts) never leaves a size without positions -- `free_window` is empty only from pw0 + 5 on, which no slack
    reaches.  The stage's `continue` for it stays unreached by design; the diagnostic refuses the starts that would reach it."""
    nwx, nwy, clipped = set(), set(), {r: set() for r in range(4)}
    for c in FC.CASES:
        pw0, ph0, x0, y0 = c.start
        for pw, ph, (xa, xb, ya, yb) in FC.items(c):
            nwx.add(xb - xa + 1); nwy.add(yb - ya + 1)
            clipped[c.W % 4].update(k for k, hit in (("left", xa > x0 - 4), ("right", xb < x0 + 4), ("top", ya > y0 - 4), ("bottom", yb < y0 + 4)) if hit)
        assert len(FC.items(c)) == len([1 for pw in range(max(pw0 - c.slack, c.wmin, 32), min(pw0 + c.slack, c.wmax, c.W) + 1)
                                        for ph in range(max(ph0 - c.slack, 32), min(ph0 + c.slack, c.H) + 1)]), c.name      # no size without a window
    assert nwx >= {1, 5, 9} and nwy >= {1, 5, 9}, (nwx, nwy)
    assert all(v == {"left", "right", "top", "bottom"} for v in clipped.values()), clipped
    xa, xb, _, _ = free_window((40, 36, 120, 60, 0), 160, 96, 45, 36)                  # pw0 + 5 at the right edge: what a = 4 cannot ask for
    assert xa > xb
    xa, xb, _, _ = free_window((40, 36, 120, 60, 0), 160, 96, 44, 36)
    assert xa == xb == 116


@pytest.mark.parametrize("name", FC.names())
def test_the_restatement_answers_what_the_content_decides(name):
    """locate_cases' contents under this stage's rule (locate_free_cases.truth), by the restatement alone; every scored slot holds
    a sum that fits the size, every other one is all ones."""
    c = FC.BY_NAME[name]
    sums, answer = FC.reference(name)
    want = FC.truth(c)
    print(name, "answer", answer, "truth", want, "cut", c.rect, "start", c.start)
    scored = sums != FC.EMPTY
    assert scored.sum() == sum((w[1] - w[0] + 1) * (w[3] - w[2] + 1) for _, _, w in FC.items(c)) > 0
    assert int(sums[scored].max()) <= 255 * (c.start[0] + c.slack) * (c.start[1] + c.slack)
    assert sums[FC.slot(c, *answer[:4])] == answer[4]
    if want is not None:
        assert answer[:4] == want[:4] and (want[4] is None or answer[4] == want[4])
    if c.content == "flat" or c.variant == "foreign":                              # every scored candidate ties, per pixel
        per_pixel = {int(sums[FC.slot(c, pw, ph, x, y)]) // (pw * ph) for pw, ph, (xa, xb, ya, yb) in FC.items(c) for y in (ya, yb) for x in (xa, xb)}
        assert per_pixel == ({255} if c.variant == "foreign" else {0}) and int(sums[scored].min()) == answer[4]
    if c.table == "X":
        assert want is not None or (c.content in ("rows", "columns") and c.variant == "resized")
    if c.rect != (c.start[2], c.start[3]) + c.start[:2] and c.variant != "foreign" and c.content in ("noise", "binary"):
        x, y, pw, ph = c.rect                                                      # a start off the truth: the winner is not the centre slot
        assert answer[:4] == (pw, ph, x, y) != c.start


def test_header_signature_and_stub_state_the_diagnostic():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    assert text.index("ssw_locate_free_rgb8(ssw_ctx") < text.index("Diagnostic: steps 2-5 of ssw_locate_free_rgb8") < text.index("ssw_locate_free_sums_rgb8(ssw_ctx")
    doc = " ".join(text[text.index("Diagnostic: steps 2-5 of ssw_locate_free_rgb8"):text.index("ssw_locate_free_sums_rgb8(ssw_ctx")].split())
    for phrase in ("ONE suspect", "The same stage as the public call runs", "(pw - pw0 + a) (2a + 1) + (ph - ph0 + a)", "9 (y - y0 + 4) + (x - x0 + 4)",
                   "relative to the unclipped start", "UINT64_MAX", "they are A0 and 0", "SSW_ERR_BAD_ARG", "x0 > w - pw0 or y0 > h - ph0",
                   "SSW_ERR_UNSUPPORTED as for the public call", "Waits for the stream once"):
        assert phrase in doc, phrase
    sig = L.SIGNATURES["ssw_locate_free_sums_rgb8"][1]
    assert len(sig) == 15 and sig[8] == C.POINTER(C.c_uint32) and sig[9:12] == [C.c_uint32] * 3 and sig[12] == sig[14] == C.POINTER(C.c_uint64)
    assert "ssw_locate_free_sums_rgb8(" in open(os.path.join(ROOT, "tests", "cpp", "locate_free_stub.cpp")).read()
    assert len(L.STAGES) == 15
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ssw_locate_free_sums_rgb8" in design and "free_stage" in design
    assert np.dtype(np.uint64).itemsize == C.sizeof(C.c_uint64)
    assert set(LC.FOREIGN) < set(FC.CONTENTS)
