"""The unknown-angle row of the strength report, without a GPU.  `rotate_search_ref` restates ssw_rotate_search_attack_rgb8 as
the composition include/ssw.h defines it by -- `affine_ref` (Pillow's rotate), `find_angle_ref`, `unrotate_ref`, `Rotate.kept`, all
imported from the files that check them -- and tests/test_rotate_search_gpu.py holds the device to it, with equality.  Checked
here: what the restatement answers on the cat for the angles of the GPU end-to-end test, the report's library calls for a mixed
`rotations=` list on the recording stand-in of tests/fake_ssw.py (and that a list without a `search` makes the calls of the
commit tests/golden/rotate_search_calls_parent.json names), and the Python and CLI surfaces."""
import argparse
import ctypes as C
import io
import json
import math
import os
import re
import sys

import numpy as np
import pytest

import fake_ssw
from conftest import GOLDEN, ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from test_angle_cpu import cat, find_angle_ref, marked_cat, smooth, turned
from test_rotate_cpu import BICUBIC, BILINEAR, affine_ref, is_copy, pil_rotate, rotation_matrix_ref, unrotate_mask_ref, unrotate_ref

sys.path.insert(0, GOLDEN)
import gen_rotate_search_calls as G  # noqa: E402

with open(G.RECORD) as f:
    PARENT = json.load(f)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
class SearchedRef:
    def __init__(self, turned_frame, found, out, kept):
        self.turned, self.found, self.out, self.kept = turned_frame, found, out, kept


def rotate_search_ref(base, frame, angle, filt, fill, amin, amax):
    """Job (frame, Rotate(angle, filt), fill) of ssw_rotate_search_attack_rgb8 over amin .. amax: the turned frame, what the
    search answers on it (a `FoundRef`: n, D, c, rungs), the frame turned back by n / 32 and the pixels that undoing keeps"""
    h, w = base.shape[:2]
    T = affine_ref(frame, (w, h), rotation_matrix_ref(angle, w, h), filt, fill)
    found = find_angle_ref(base, T, amin, amax)
    kept = w * h if is_copy(w, h, found.n / 32) else int(unrotate_mask_ref(w, h, found.n / 32).sum())
    assert api.Rotate(found.n / 32).kept(w, h) == kept / (w * h)        # the count `Rotate.kept` makes its share of
    return SearchedRef(T, found, unrotate_ref(base, T, found.n / 32), kept)


def test_the_restatement_is_a_composition_of_checked_parts():
    base = smooth(96, 64)
    marked = np.clip(base.astype(np.int64) + np.random.default_rng(2).integers(-2, 3, base.shape), 0, 255).astype(np.uint8)
    r = rotate_search_ref(base, marked, 1.5, BICUBIC, (9, 200, 30), -4, 4)
    assert np.array_equal(r.turned, pil_rotate(marked, 1.5, BICUBIC, (9, 200, 30)))                # Pillow's rotate
    assert (r.found.j0, r.found.j1, len(r.found.rungs)) == (-16, 16, 33) and abs(r.found.n - 48) <= 1
    angle = r.found.n / 32
    mask = unrotate_mask_ref(96, 64, angle)
    assert r.kept == int(mask.sum()) and 0 < r.kept < 96 * 64
    assert np.array_equal(r.out[~mask], base[~mask]) and not np.array_equal(r.out[mask], base[mask])
    same = rotate_search_ref(base, base, 0.0, BILINEAR, (0, 0, 0), -1, 1)                          # nothing turned: found 0, a copy
    assert same.found.n == 0 and same.found.D == 0 and same.kept == 96 * 64 and np.array_equal(same.out, base)


# ---- what the restatement answers on the cat: the angles of the GPU end-to-end test ----------------------------------------------
# (angle, filter, range, the answer): chosen so that the restatement alone is within one grid step (1/32 degree) of the truth --
# DESIGN 4.18 records 0.1 -> 0.125 as the near-miss of this search, so an angle like it is not among them
E2E = [(1.3, "bicubic", (-10.0, 10.0), 1.3125), (-2.5, "bilinear", (-5.0, 5.0), -2.5)]
E2E_KNOWN = 0.5


@pytest.mark.parametrize("angle,filt,search,answer", E2E, ids=lambda v: str(v))
def test_the_restatement_finds_the_end_to_end_angles_on_the_cat(angle, filt, search, answer):
    f = find_angle_ref(cat(), turned(marked_cat(), angle, filt.upper(), (0, 0, 0)), *search)
    print(angle, filt, search, "->", f.angle, "mean", f.D / f.c)
    assert f.angle == answer and abs(f.angle - angle) <= 1 / 32
    assert 2.0 < f.D / f.c < 4.5                                        # a marked copy's own distance, not a wrong angle's


# ---- the report's calls on the recording stand-in --------------------------------------------------------------------------------
MIXED = [api.Rotate(0.5), api.Rotate(1.3, search=True), api.Rotate(2.0, "bilinear"), api.Rotate(-1.0, search=(-5, 5)),
         api.Rotate(0.7, "bilinear", search=True)]
COPIES = 3
AFTER_AN_ATTACK = ["ssw_fingerprint_trace_rgb8", "ssw_quality_rgb8", "ssw_copy_to_host", "ssw_copy_to_host"]


def test_the_record_is_the_generators():
    assert re.fullmatch(r"[0-9a-f]{7,}", PARENT["commit"]) and PARENT["known"]["live"] == 0
    assert [c[0] for c in PARENT["known"]["calls"]].count("ssw_rotate_attack_rgb8") == 2         # one per alpha
    assert all("search" not in c[0] for c in PARENT["known"]["calls"])


@pytest.mark.parametrize("case,more", [("known", {}), ("known_ssim", {"ssim": True})])
def test_a_list_without_a_search_makes_the_parents_calls(case, more):
    assert all(r.search is None for r in G.known())
    got = G.record(G.known(), **more)
    assert len(got["calls"]) == len(PARENT[case]["calls"])
    for i, (g, p) in enumerate(zip(got["calls"], PARENT[case]["calls"])):
        assert g == p, (i, g, p)
    assert got["allocs"] == PARENT[case]["allocs"] and got["live"] == 0


def test_a_mixed_list_adds_one_search_call_per_range_behind_the_known_call():
    ctx = fake_ssw.fake_context()
    rows = G.report(ctx, MIXED)
    calls = json.loads(json.dumps(ctx._lib.calls))
    names = [c[0] for c in calls]
    assert ctx._lib.live == {}
    # per alpha: the known rotations' call and what follows an attack, then per range the search call and the same four
    per_alpha = ["ssw_rotate_attack_rgb8"] + AFTER_AN_ATTACK + 2 * (["ssw_rotate_search_attack_rgb8"] + AFTER_AN_ATTACK)
    first = names.index("ssw_rotate_attack_rgb8")
    assert names[first:first + len(per_alpha)] == per_alpha and names[-len(per_alpha):] == per_alpha
    assert names.count("ssw_rotate_search_attack_rgb8") == 4 and names.count("ssw_rotate_attack_rgb8") == 2
    # without the search calls and what follows them, the record is the known-only report's, argument for argument
    rest, i = [], 0
    while i < len(calls):
        if names[i] == "ssw_rotate_search_attack_rgb8":
            i += 1 + len(AFTER_AN_ATTACK)
            continue
        rest.append(calls[i])
        i += 1
    assert rest == PARENT["known"]["calls"]
    # the search calls themselves: the original, the copies, rotation-major jobs of the range's entries, the range
    w, h, fb = G.W, G.H, G.W * G.H * 3
    searches = [c[1] for c in calls if c[0] == "ssw_rotate_search_attack_rgb8"]
    for args, (rng, which) in zip(searches, 2 * [((-10.0, 10.0), [1, 4]), ((-5.0, 5.0), [3])]):
        n = len(which) * COPIES
        jobs = (L.RotateJob * n)(*[MIXED[i].job(c, w, h) for i in which for c in range(COPIES)])
        assert args[:6] == ["ctx", ["dev", fb, 0], ["dev", COPIES * fb, 0], COPIES, w, h]
        assert args[6] == bytes(jobs).hex() and args[7:10] == [n, rng[0], rng[1]]
        assert args[10] == ["dev", n * fb, 0] and args[11] is None and args[13] is None and args[14] == "host"
        assert args[12] == bytes(C.sizeof(L.AngleFound) * n).hex()       # the answers' array, still empty: the stand-in finds nothing
    # the rows: in the order given; the stand-in answers n = 0 and kept = 0 everywhere
    for row in rows:
        assert [r.rotation for r in row.rotations] == [m.label for m in MIXED]
        for r, m in zip(row.rotations, MIXED):
            assert r.search == m.search
            if m.search is None:
                assert math.isnan(r.found_min) and math.isnan(r.found_max) and math.isnan(r.worst_angle_error)
            else:
                assert (r.found_min, r.found_max, r.worst_angle_error, r.kept) == (0.0, 0.0, abs(m.angle), 0.0)


def test_only_searched_rotations_make_no_known_call():
    ctx = fake_ssw.fake_context()
    rows = G.report(ctx, [api.Rotate(1.0, search=(0, 2))], ssim=True)
    names = [c[0] for c in ctx._lib.calls]
    assert "ssw_rotate_attack_rgb8" not in names and "ssw_unrotate_kept" not in names and names.count("ssw_rotate_search_attack_rgb8") == 2
    assert names[-7:] == ["ssw_rotate_search_attack_rgb8"] + AFTER_AN_ATTACK + ["ssw_ssim_rgb8", "ssw_copy_to_host"]
    assert [len(r.rotations) for r in rows] == [1, 1] and ctx._lib.live == {}


def test_an_error_from_the_search_call_leaves_nothing_live():
    ctx = fake_ssw.fake_context({"ssw_rotate_search_attack_rgb8": L.SSW_ERR_BAD_ARG})
    with pytest.raises(api.SswError) as e:
        G.report(ctx, MIXED)
    assert e.value.status == L.SSW_ERR_BAD_ARG and ctx._lib.calls[-1][0] == "ssw_rotate_search_attack_rgb8" and ctx._lib.live == {}


def test_rotate_search_attack_groups_by_range_on_the_stand_in():
    ctx = fake_ssw.fake_context()
    images = list(np.random.default_rng(4).integers(0, 256, (2, G.H, G.W, 3), dtype=np.uint8))
    frames, found = api.rotate_search_attack(G.frame(), images, [api.Rotate(1.0, search=(0, 2)), api.Rotate(2.0), api.Rotate(3.0, search=(0, 2))], ctx)
    calls = [c for c in ctx._lib.calls if c[0] == "ssw_rotate_search_attack_rgb8"]
    assert [c[1][7:10] for c in calls] == [[4, 0.0, 2.0], [2, -10.0, 10.0]]      # a rotation without a range: the default one
    w, h = G.W, G.H
    jobs = (L.RotateJob * 4)(*[api.Rotate(a).job(i, w, h) for i in range(2) for a in (1.0, 3.0)])      # frame-major, as rotate_attack's
    assert calls[0][1][6] == bytes(jobs).hex()
    assert [len(f) for f in frames] == [3, 3] and frames[1][2].shape == (h, w, 3) and found[0][1] == api.FoundAngle(0.0, 0, 0, 0, 0.0)
    assert ctx._lib.live == {}


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_python_surface_without_a_gpu():
    assert api.Rotate(1.3).search is None and api.Rotate(1.3, search=True).search == (-10.0, 10.0)
    assert api.Rotate(1.3, "bilinear", (-2, 3)).search == (-2.0, 3.0) and api.Rotate(1.3, search=[0, 45]).search == (0.0, 45.0)
    assert api.Rotate(1.3, search=True).label == "rotate 1.3 bicubic, angle searched in -10..10"
    assert api.Rotate(2, "Bilinear", search=(-0.5, 7.25)).label == "rotate 2 bilinear, angle searched in -0.5..7.25"
    assert api.Rotate(1.3).label == "rotate 1.3 bicubic"
    assert bytes(api.Rotate(1.3, search=True).job(2, 640, 444, (1, 2, 3))) == bytes(api.Rotate(1.3).job(2, 640, 444, (1, 2, 3)))      # `job` is unchanged
    assert api.Rotate(1.3, search=True).kept(64, 48) == api.Rotate(1.3).kept(64, 48)
    for bad in (lambda: api.Rotate(1, search=(2, 1)), lambda: api.Rotate(1, search=(-46, 0)), lambda: api.Rotate(1, search=(0, 45.5)),
                lambda: api.Rotate(1, search=(float("nan"), 1)), lambda: api.Rotate(1, search=(1,)), lambda: api.Rotate(1, search=("0", 1)),
                lambda: api.Rotate(1, search=False), lambda: api.Rotate(1, search=5),
                lambda: api.rotate_search_attack(np.zeros((40, 40, 3), np.uint8), [np.zeros((40, 41, 3), np.uint8)], [api.Rotate(1)]),
                lambda: api.rotate_search_attack(np.zeros((31, 40, 3), np.uint8), [np.zeros((31, 40, 3), np.uint8)], [api.Rotate(1)]),
                lambda: api.rotate_search_attack(np.zeros((40, 40, 3), np.uint8), [np.zeros((40, 40, 3), np.uint8)], [1.0]),
                lambda: api.strength_report(np.zeros((31, 40, 3), np.uint8), [0.1], rotations=[api.Rotate(1, search=True)])):
        with pytest.raises(ValueError):
            bad()
    z = np.zeros((40, 40, 3), np.uint8)
    assert api.rotate_search_attack(z, [], [api.Rotate(1)]) == ([], []) and api.rotate_search_attack(z, [z, z], []) == ([[], []], [[], []])
    r = api.RotateResult("rotate 1 bicubic", 0.5, 3, 1.0, 0.5, 0, 30.0, 31.0)                     # the constructor of before
    assert r.search is None and math.isnan(r.found_min) and math.isnan(r.found_max) and math.isnan(r.worst_angle_error) and math.isnan(r.ssim_min)
    from spread_spectrum_watermarking_amd import rotate_search_attack
    assert rotate_search_attack is api.rotate_search_attack


def test_header_declares_what_the_loader_binds():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssw.h")).read(), flags=re.S)
    assert re.search(r"int ssw_rotate_search_attack_rgb8\(ssw_ctx\* ctx, const uint8_t\* dev_base, const uint8_t\* dev_frames, size_t n_frames, size_t w, size_t h,\s*"
                     r"const ssw_rotate_job\* jobs, size_t n_jobs, double amin, double amax, uint8_t\* dev_out,\s*"
                     r"uint8_t\* dev_turned, ssw_angle_found\* host_found, uint64_t\* host_rungs, uint64_t\* host_kept\);", text)
    kinds = L.SIGNATURES["ssw_rotate_search_attack_rgb8"][1]
    assert len(kinds) == 15 and kinds[8:10] == [C.c_double, C.c_double] and kinds[6] == C.POINTER(L.RotateJob) and kinds[12] == C.POINTER(L.AngleFound)
    assert re.search(r"SSW_STAGE_COUNT = 15\b", text) and len(L.STAGES) == 15                      # no new stage
    assert hasattr(L.load(), "ssw_rotate_search_attack_rgb8")
    hpp = open(os.path.join(ROOT, "include", "ssw_rotate_search.hpp")).read()
    assert "ssw_rotate_search_attack_rgb8(" in hpp and '#include "ssw_angle.hpp"' in hpp


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_cli_parses_the_three_spellings():
    assert cli._rotate_arg("1.3:?") == api.Rotate(1.3, "bicubic", (-10.0, 10.0))
    assert cli._rotate_arg("2:bilinear:?") == api.Rotate(2.0, "bilinear", (-10.0, 10.0))
    assert cli._rotate_arg("1.3:?-5..5") == api.Rotate(1.3, "bicubic", (-5.0, 5.0))
    assert cli._rotate_arg("-1:bilinear:?-3.5..-0.25") == api.Rotate(-1.0, "bilinear", (-3.5, -0.25))
    assert cli._rotate_arg("0.5") == api.Rotate(0.5) and cli._rotate_arg("2:bilinear") == api.Rotate(2.0, "bilinear")       # as before
    for bad in ("1:", "1::?", "1:?5", "1:?9..1", "x:?", "1:lanczos:?", "1:?:bicubic", "1:?-50..0", "1:?..", "1:bicubic:?:?"):
        with pytest.raises(argparse.ArgumentTypeError):
            cli._rotate_arg(bad)
    args = cli.build_parser().parse_args(["strength", "cat.png", "--alpha", "0.1", "--rotate", "0.5", "1.3:?", "2:bilinear:?", "1.3:?-5..5"])
    assert args.rotations == [api.Rotate(0.5), api.Rotate(1.3, search=True), api.Rotate(2.0, "bilinear", True), api.Rotate(1.3, search=(-5, 5))]


def strength_output(rows, rotations, as_json):
    """What cli.cmd_strength prints for `rows` (strength_report and the image file are stood in for)"""
    args = argparse.Namespace(file="cat.png", alpha=[0.1], length=50, copies=8, collude=[], method=[], similarity_exceed=6.0, jpeg=[], ssim=False,
                              filters=[], scales=[], rotations=rotations, json=as_json)
    before = cli.strength_report, cli._open_image
    seen = {}
    cli.strength_report, cli._open_image = (lambda *a, **k: seen.update(k) or rows), (lambda path: None)
    try:
        out = io.StringIO()
        assert cli.cmd_strength(args, out) == 0
        assert seen["rotations"] == rotations
        return out.getvalue()
    finally:
        cli.strength_report, cli._open_image = before


def test_cli_prints_the_searched_row():
    q = [api.Quality((120, 90, 300), 170, 400, 3, 640 * 444)] * 8
    rotations = [api.Rotate(0.5), api.Rotate(1.3, search=True)]
    known = api.RotateResult("rotate 0.5 bicubic", 0.9849, 8, 27.31, 2.04, 0, 33.04, 35.96)
    searched = api.RotateResult(rotations[1].label, 0.979, 8, 25.46, 2.31, 0, 31.5, 32.25, search=(-10.0, 10.0), found_min=1.28125, found_max=1.3125,
                                worst_angle_error=0.01875)
    rows = [api.StrengthRow(0.1, q, [], rotations=[known, searched])]
    lines = strength_output(rows, rotations, False).splitlines()
    assert lines[-2] == "  rotate 0.5 bicubic: own mark found 8/8, weakest 27.3, strongest innocent 2.0, 33.0 .. 36.0 dB, 98.5 % kept"      # as before
    assert lines[-1] == ("  rotate 1.3 bicubic, angle searched in -10..10: found 1.28125 .. 1.3125, own mark found 8/8, weakest 25.5, "
                         "strongest innocent 2.3, 31.5 .. 32.2 dB, 97.9 % kept")
    doc = json.loads(strength_output(rows, rotations, True))
    assert sorted(doc[0]["rotations"][0]) == ["accused", "kept", "psnr_max", "psnr_min", "rotation", "strongest_innocent", "survived", "weakest_own"]
    assert {k: doc[0]["rotations"][1][k] for k in ("search", "found_min", "found_max", "worst_angle_error", "kept", "rotation")} == {
        "search": [-10.0, 10.0], "found_min": 1.28125, "found_max": 1.3125, "worst_angle_error": 0.01875, "kept": 0.979,
        "rotation": "rotate 1.3 bicubic, angle searched in -10..10"}
