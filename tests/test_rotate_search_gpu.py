"""ssw_rotate_search_attack_rgb8 on the GPU against `rotate_search_ref` of tests/test_rotate_search_cpu.py -- the composition of
the committed restatements the call is defined by: EQUALITY of host_found, every rung's (D, c), the turned frames, the restored
frames and the kept counts, at the smallest shapes at which angle_cost_shared_kernel can go wrong (the minimum, tail bytes of a
word, a pixel past a tile at either factor, the largest box, the 64-bit origin of a 20 000 pixel strip), each with share-groups of
1, 16 and 17 members; members of one group whose candidate lists differ, two groups whose kept rungs differ, ties at every stage,
the largest D, device pointers one and three bytes off, a call of two workspace groups, every error code; that
ssw_find_angle_rgb8 answers the same on the same turned frames; and the report's rows on the cat, in float32 bits."""
import ctypes as C
import functools
import json
import re

import numpy as np
import pytest
from PIL import Image

from gpu_util import ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import check
from test_angle_cpu import cat, rungs_ref, smooth, turned
from test_angle_gpu import Dev, dev_find
from test_rotate_cpu import BICUBIC, BILINEAR, NAMES
from test_rotate_search_cpu import E2E, E2E_KNOWN, rotate_search_ref

pytestmark = pytest.mark.gpu

FILL = (200, 30, 120)


def dev_search(base, frames, jobs, amin, amax, off=0, want_turned=True, want_rungs=True):
    """One call.  jobs: (frame, angle, filter, fill).  -> ([(n, D, c)], rungs [jobs][n_rungs][2], turned, out, kept)"""
    frames = np.stack(frames)
    n, (_, h, w, _) = len(jobs), frames.shape
    arr = (L.RotateJob * n)(*[api.Rotate(a, NAMES[filt]).job(f, w, h, fill) for f, a, filt, fill in jobs])
    for j in arr:                                                       # `back` is not read
        j.back[:] = [float("nan")] * 6
    b, d = Dev(base, off), Dev(frames, off)
    out, tur = Dev(np.full((n, h, w, 3), 0xA5, np.uint8), off), Dev(np.full((n, h, w, 3), 0x5A, np.uint8), off)
    found, kept = (L.AngleFound * n)(), np.full(n, 0xA5A5A5A5, np.uint64)
    j0, j1 = rungs_ref(amin, amax)
    rungs = np.full((n, j1 - j0 + 1, 2), 0xA5A5A5A5, np.uint64)
    try:
        check(lib().ssw_rotate_search_attack_rgb8(ctx().handle, b.ptr, d.ptr, len(frames), w, h, arr, n, amin, amax, out.ptr,
                                                  tur.ptr if want_turned else None, found, rungs.ctypes.data if want_rungs else None,
                                                  kept.ctypes.data), "ssw_rotate_search_attack_rgb8")
        got = []
        for x in (tur, out):
            host = np.empty((n, h, w, 3), np.uint8)
            check(lib().ssw_copy_to_host(ctx().handle, host.ctypes.data, x.ptr, host.nbytes), "ssw_copy_to_host")
            got.append(host)
    finally:
        for x in (b, d, out, tur):
            x.free()
    assert all(f.n_rungs == j1 - j0 + 1 for f in found)
    return [(f.n, f.sad, f.count) for f in found], rungs, got[0], got[1], [int(k) for k in kept]


def same_as_ref(base, frames, jobs, amin, amax, what, off=0, ref=None):
    """Every output of the call equals the restatement's; -> the restatement's answers, one per job"""
    ref = ref or (lambda f, a, filt, fill: rotate_search_ref(base, frames[f], a, filt, fill, amin, amax))
    cache = {}
    refs = [cache.get(j) or cache.setdefault(j, ref(*j)) for j in jobs]
    found, rungs, tur, out, kept = dev_search(base, frames, jobs, amin, amax, off)
    for i, r in enumerate(refs):
        want = np.asarray(r.found.rungs, np.uint64)
        bad = np.nonzero((rungs[i] != want).any(axis=1))[0]
        assert bad.size == 0, (what, i, "rung", int(bad[0]), rungs[i][bad[0]].tolist(), r.found.rungs[bad[0]])
        assert found[i] == (r.found.n, r.found.D, r.found.c), (what, i, found[i], (r.found.n, r.found.D, r.found.c))
        assert np.array_equal(tur[i], r.turned), (what, i, "turned")
        assert np.array_equal(out[i], r.out), (what, i, "restored")
        assert kept[i] == r.kept, (what, i, kept[i], r.kept)
    return refs


def variants(base, n):
    """n frames that differ from `base` by a little noise of their own: neighbours in a share-group must not mix"""
    return [np.clip(base.astype(np.int64) + np.random.default_rng(90 + i).integers(-2, 3, base.shape), 0, 255).astype(np.uint8) for i in range(n)]


# ---- shapes x share-group sizes ----------------------------------------------------------------------------------------------------
# (w, h, range, the angle of the turn, why)
SHAPES = [(32, 32, 4, 1.5, "the minimum"), (33, 47, 4, -2.75, "tail bytes of a word"), (65, 41, 2, 0.8, "a pixel past a tile at f = 1"),
          (132, 36, 2, -1.3, "a partial tile at f = 4"), (35, 130, 45, 18.0, "the largest box"),
          (20000, 32, 0.5, 0.25, "the 64-bit origin, across"), (32, 20000, 0.5, -0.09375, "the 64-bit origin, down")]


@functools.lru_cache(maxsize=None)
def shape_case(w, h):
    """(base, three frames, the restatement of (frame, angle, filter) memoised): made once for the three group sizes"""
    base = smooth(w, h)
    frames = variants(base, 3 if w * h < 100000 else 2)
    r, angle = next((r, a) for sw, sh, r, a, _ in SHAPES if (sw, sh) == (w, h))
    ref = functools.lru_cache(maxsize=None)(lambda f, a, filt, fill: rotate_search_ref(base, frames[f], a, filt, fill, -r, r))
    return base, frames, ref, r, angle


@pytest.mark.parametrize("members", [1, 16, 17])
@pytest.mark.parametrize("w,h", [s[:2] for s in SHAPES], ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_shapes_and_share_group_sizes_equal_the_restatement(w, h, members):
    base, frames, ref, r, angle = shape_case(w, h)
    jobs = [(i % len(frames), angle, BICUBIC, FILL) for i in range(members)]     # one matrix: one share-group, two at 17
    refs = same_as_ref(base, frames, jobs, -r, r, (w, h, members), ref=ref)
    assert len(refs[0].found.rungs) == int(8 * r) + 1


# ---- lists that differ --------------------------------------------------------------------------------------------------------
def test_members_of_one_group_whose_lists_differ():
    """One matrix, so one share-group -- but the frames arrive already turned by different angles, so the members' kept rungs and
    slot lists differ and most candidates of the union are wanted by one member only"""
    base = smooth(96, 64)
    frames = [turned(base, a, "BICUBIC", (0, 0, 0)) for a in (0.0, -3.0, 2.5, -0.5)] + variants(base, 1)
    jobs = [(i % 5, 1.0, BICUBIC if i % 2 else BILINEAR, FILL) for i in range(11)]
    refs = same_as_ref(base, frames, jobs, -6, 6, "lists differ")
    assert len({tuple(sorted(r.found.kept)) for r in refs}) >= 4
    assert len({r.found.n for r in refs}) >= 4


def test_two_groups_in_one_call_whose_kept_rungs_differ():
    base = smooth(65, 41, 5)
    frames = variants(base, 2)
    jobs = [(i % 2, 3.0 if i % 3 else -2.0, BICUBIC, FILL) for i in range(9)]      # two matrices, interleaved
    refs = same_as_ref(base, frames, jobs, -4, 4, "two groups")
    assert len({tuple(r.found.kept) for r in refs}) >= 2
    # a filter or a fill of its own does not split a share-group, and frames may repeat
    same_as_ref(base, frames, [(0, 1.0, BICUBIC, FILL), (0, 1.0, BILINEAR, FILL), (1, 1.0, BICUBIC, (0, 0, 0)), (0, 1.0, BICUBIC, FILL)], -2, 2, "one matrix")


def test_identical_flat_frames_tie_at_every_stage():
    flat = np.full((40, 52, 3), 93, np.uint8)
    refs = same_as_ref(flat, [flat], [(0, 0.0, BICUBIC, (93, 93, 93))] * 5, -3, 3, "flat")
    assert all((r.found.n, r.found.D, r.found.kept) == (-96, 0, [0, 1, 2, 3]) for r in refs)      # as DESIGN 4.18 records


def test_the_largest_difference():
    black, white = np.zeros((48, 40, 3), np.uint8), np.full((48, 40, 3), 255, np.uint8)
    refs = same_as_ref(black, [white], [(0, 0.0, BILINEAR, (255, 255, 255))] * 3, -2, 2, "all-255 on all-0")
    assert all(r.found.D == 255 * r.found.c for r in refs)


def test_device_pointers_one_and_three_bytes_off():
    base = smooth(65, 41, 3)
    frames = variants(base, 2)
    same_as_ref(base, frames, [(0, 1.0, BICUBIC, FILL), (1, 1.0, BICUBIC, FILL), (0, -1.75, BILINEAR, FILL)], -2, 2, "one byte off", off=1)
    same_as_ref(base, frames, [(1, 1.0, BICUBIC, FILL)], -2, 2, "three bytes off", off=3)


def test_the_angle_found_is_zero_or_on_the_edge_of_the_range():
    base = smooth(64, 48)
    refs = same_as_ref(base, [base], [(0, 0.0, BICUBIC, FILL), (0, 360.0, BILINEAR, FILL)], -1, 1, "nothing turned")
    assert all(r.found.n == 0 and r.kept == 64 * 48 and np.array_equal(r.out, base) for r in refs)      # the undoing is a copy
    same_as_ref(base, [base], [(0, 2.0, BICUBIC, FILL)], 2.0, 2.0, "a range of one angle")


def test_without_the_optional_outputs_the_answers_are_the_same():
    base = smooth(65, 41)
    frames, jobs = variants(base, 2), [(0, 0.5, BICUBIC, FILL), (1, 0.5, BICUBIC, FILL)]
    full = dev_search(base, frames, jobs, -2, 2)
    bare = dev_search(base, frames, jobs, -2, 2, want_turned=False, want_rungs=False)
    assert bare[0] == full[0] and np.array_equal(bare[3], full[3]) and bare[4] == full[4]
    assert np.all(bare[2] == 0x5A) and np.all(bare[1] == 0xA5A5A5A5)    # neither written


# ---- the two checks that guard ssw_find_angle_rgb8 itself ---------------------------------------------------------------------------
def test_find_angle_answers_the_same_on_the_same_turned_frames():
    base = smooth(132, 36)
    frames = [turned(base, a, "BICUBIC", (0, 0, 0)) for a in (0.0, 1.25)] + variants(base, 1)
    jobs = [(i % 3, -1.0 if i < 4 else 0.75, BICUBIC, FILL) for i in range(7)]
    found, rungs, tur, _, _ = dev_search(base, frames, jobs, -3, 3)
    alone, alone_rungs = dev_find(base, list(tur), -3, 3)
    assert alone == found and np.array_equal(alone_rungs, rungs)


def test_every_rung_sum_is_find_angles_on_the_turned_frames():
    """angle_cost_shared_kernel against angle_cost_kernel at every rung, not only the winner: one 65 x 41 frame, 3 copies, +-2
    degrees -- the rung sums [n][n_rungs][2] of the call are, word for word, those ssw_find_angle_rgb8 returns for dev_turned"""
    base = smooth(65, 41)
    jobs = [(i, 1.25, BICUBIC, FILL) for i in range(3)]
    found, rungs, tur, _, _ = dev_search(base, variants(base, 3), jobs, -2, 2)
    alone, alone_rungs = dev_find(base, list(tur), -2, 2)
    assert rungs.shape == alone_rungs.shape == (3, 17, 2) and rungs.dtype == alone_rungs.dtype == np.uint64
    assert np.array_equal(alone_rungs, rungs) and alone == found


def test_a_report_without_a_searched_entry_leaves_locate_untimed():
    base = smooth(64, 48)
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        api.strength_report(base, [0.1], k=50, copies=2, sizes=(2,), methods=("average",), seed=1, ctx=c, rotations=[api.Rotate(1.0)])
        c.synchronize()
        t = c.timing()
        assert t["locate"]["launches"] == 0 and t["locate"]["ms"] == 0.0 and t["locate_coarse"]["launches"] == 0
        c.reset_timing()
        api.strength_report(base, [0.1], k=50, copies=2, sizes=(2,), methods=("average",), seed=1, ctx=c, rotations=[api.Rotate(1.0, search=(-2, 2))])
        c.synchronize()
        t = c.timing()
    finally:
        c.enable_timing(False)
    assert t["locate"]["launches"] >= 1 and t["locate"]["work"] > 0
    assert t["locate_coarse"]["launches"] == 1 and t["locate_coarse"]["work"] == 2 * 17 * (64 // 4) * (48 // 4)      # the ladder, nested
    assert t["resize"]["launches"] >= 2                                 # the turn and its undoing


# ---- two workspace groups -----------------------------------------------------------------------------------------------------
def test_a_call_of_two_workspace_groups_is_the_calls_it_is_made_of():
    """At 3840 x 2160 a job's turned frame and planes take 34 MB: 9 jobs are two groups (7 + 2), and the share-group of a rotation
    is cut where the workspace group ends.  The restatement would take minutes here; the device calls the entry is DEFINED by
    (ssw_affine_rgb8, ssw_find_angle_rgb8, ssw_unrotate_rgb8, ssw_unrotate_kept) are the reference, and frames are compared on
    the device (ssw_quality_rgb8, one original per copy: no byte differs)."""
    w, h, n = 3840, 2160, 9
    base = smooth(w, h)
    frame = np.clip(base.astype(np.int16) + np.random.default_rng(5).integers(-2, 3, base.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    angles = [1.3] * 5 + [-0.7] * 4
    jobs = (L.RotateJob * n)(*[api.Rotate(a).job(0, w, h) for a in angles])
    c, fb = ctx(), w * h * 3
    b, d = Dev(base), Dev(frame[None])
    out, tur, ref_t, ref_o, stats = [c.alloc(n * fb) for _ in range(4)] + [c.alloc(n * 8 * L.QUALITY_STATS)]
    found, kept, rungs = (L.AngleFound * n)(), np.zeros(n, np.uint64), np.zeros((n, 81, 2), np.uint64)
    at = lambda buf, i: C.c_void_p(buf.ptr.value + i * fb)
    try:
        check(lib().ssw_rotate_search_attack_rgb8(c.handle, b.ptr, d.ptr, 1, w, h, jobs, n, -10.0, 10.0, out.ptr, tur.ptr, found, rungs.ctypes.data,
                                                  kept.ctypes.data), "ssw_rotate_search_attack_rgb8")
        fill, host = (C.c_uint8 * 4)(0, 0, 0, 0), np.empty(fb, np.uint8)
        for i0, i1 in ((0, 5), (5, 9)):                                 # the turned frame of a rotation, made once and laid out per job
            check(lib().ssw_affine_rgb8(c.handle, d.ptr, 1, w, h, w, h, jobs[i0].forward, L.AFFINE_BICUBIC, fill, at(ref_t, i0)), "ssw_affine_rgb8")
            check(lib().ssw_copy_to_host(c.handle, host.ctypes.data, at(ref_t, i0), fb), "ssw_copy_to_host")
            for i in range(i0 + 1, i1):
                check(lib().ssw_copy_to_dev(c.handle, at(ref_t, i), host.ctypes.data, fb), "ssw_copy_to_dev")
        alone, alone_rungs = (L.AngleFound * n)(), np.zeros((n, 81, 2), np.uint64)
        check(lib().ssw_find_angle_rgb8(c.handle, b.ptr, ref_t.ptr, n, w, h, -10.0, 10.0, alone, alone_rungs.ctypes.data), "ssw_find_angle_rgb8")
        assert [(f.n, f.sad, f.count) for f in found] == [(f.n, f.sad, f.count) for f in alone] and np.array_equal(rungs, alone_rungs)
        assert [f.n for f in found] == [42] * 5 + [-22] * 4             # 1.3125 and -0.6875: the nearest grid angles
        undo = (L.RotateJob * n)(*[api.Rotate(f.n / 32).job(i, w, h) for i, f in enumerate(alone)])
        check(lib().ssw_unrotate_rgb8(c.handle, b.ptr, ref_t.ptr, n, w, h, undo, ref_o.ptr), "ssw_unrotate_rgb8")
        want_kept = np.zeros(n, np.uint64)
        check(lib().ssw_unrotate_kept(c.handle, w, h, undo, n, want_kept.ctypes.data), "ssw_unrotate_kept")
        assert kept.tolist() == want_kept.tolist() and 0 < kept[0] < w * h
        for got, want, what in ((tur, ref_t, "turned"), (out, ref_o, "restored")):
            check(lib().ssw_quality_rgb8(c.handle, want.ptr, n, got.ptr, n, w, h, stats.ptr), "ssw_quality_rgb8")
            assert not stats.to_host(np.uint64, (n, L.QUALITY_STATS)).any(), what
        check(lib().ssw_quality_rgb8(c.handle, tur.ptr, n, out.ptr, n, w, h, stats.ptr), "ssw_quality_rgb8")
        assert stats.to_host(np.uint64, (n, L.QUALITY_STATS))[:, 4].all()      # (the comparison can tell frames apart)
    finally:
        for x in (b, d, out, tur, ref_t, ref_o, stats):
            x.free()


# ---- end to end on the cat ----------------------------------------------------------------------------------------------------
PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def test_the_report_rows_say_what_trace_finds_in_copies_pillow_turned():
    """k = 1000, 4 copies, alpha 0.1, two searched rotations and a known one beside them: a searched row is what trace_many makes
    of the copies turned by PIL.Image.rotate itself and handed over as `Rotated(search=...)` -- in float32 bits -- and the known
    row is the row of a report that has no searched entry"""
    image, n, k, alpha = cat(), 4, 1000, 0.1
    c = ctx()
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    copies = api.Writer(image, api.WriteConfig(insertion=api.Insertion.Option2(alpha)), c).mark_copies_rgb8(list(marks))
    cfg = api.ReadConfig(extraction=api.Extraction.Option2(alpha))
    rotations = [api.Rotate(E2E[0][0], E2E[0][1], E2E[0][2]), api.Rotate(E2E_KNOWN), api.Rotate(E2E[1][0], E2E[1][1], E2E[1][2])]
    rows = api.strength_report(image, [alpha], copies=n, k=k, sizes=(2,), rotations=rotations, seed=3, ctx=c)[0].rotations
    assert [r.rotation for r in rows] == [r.label for r in rotations]
    h, w = image.shape[:2]
    for row, (angle, filt, search, answer) in zip((rows[0], rows[2]), E2E):
        by_pillow = [np.asarray(Image.fromarray(copies[i]).rotate(angle, resample=PIL_FILTER[filt])) for i in range(n)]
        traced = api.trace_many(image, by_pillow, list(marks), threshold=6.0, config=cfg, ctx=c, placements=[api.Rotated(search=search)] * n)
        sims = np.asarray(traced.sims, np.float32)
        own, others = np.diagonal(sims), sims[~np.eye(n, dtype=bool)]
        print(f"{row.rotation}: found {[traced.turned[i].angle for i in range(n)]} own {own.tolist()} row {row}")
        assert np.float32(row.weakest_own).tobytes() == own.min().tobytes() and np.float32(row.strongest_innocent).tobytes() == others.max().tobytes()
        assert row.weakest_own == float(own.min()) and row.strongest_innocent == float(others.max())
        assert row.survived == int((own > np.float32(6.0)).sum()) == n and row.accused == int((others > np.float32(6.0)).sum()) == 0
        angles = [traced.turned[i].angle for i in range(n)]
        assert (row.found_min, row.found_max, row.search) == (min(angles), max(angles), search)
        assert row.worst_angle_error == max(abs(a - angle) for a in angles) <= 1 / 32 and answer in angles
        assert row.kept == min(api.Rotate(a).kept(w, h) for a in angles)
        # and the Python call: the frames the report traced
        frames, found = api.rotate_search_attack(image, list(copies), [api.Rotate(angle, filt, search)], c)
        assert [f[0].angle for f in found] == angles
        again = np.asarray(api.trace_many(image, [f[0] for f in frames], list(marks), threshold=6.0, config=cfg, ctx=c).sims, np.float32)
        assert again.tobytes() == sims.tobytes()
    known = api.strength_report(image, [alpha], copies=n, k=k, sizes=(2,), rotations=[api.Rotate(E2E_KNOWN)], seed=3, ctx=c)[0].rotations[0]
    assert repr(rows[1]) == repr(known) and known.search is None


def test_cli_strength_prints_the_searched_rows(tmp_path, capsys):
    path = str(tmp_path / "cat.png")
    Image.fromarray(cat()).save(path)
    args = ["strength", path, "--alpha", "0.1", "--copies", "3", "--collude", "2", "--method", "average", "-n", "200", "--rotate", "0.5", "1.3:?", "2.5:bilinear:?-5..5"]
    assert cli.main(args) == 0
    lines = capsys.readouterr().out.splitlines()
    tail = r"own mark found \d/3, weakest -?\d+\.\d, strongest innocent -?\d+\.\d(, \d innocent accused)?, \d\d\.\d \.\. \d\d\.\d dB, \d\d\.\d % kept"
    assert re.fullmatch(r"  rotate 0\.5 bicubic: " + tail, lines[-3]), lines[-3]
    assert re.fullmatch(r"  rotate 1\.3 bicubic, angle searched in -10\.\.10: found 1\.(28125|3125) \.\. 1\.3125, " + tail, lines[-2]), lines[-2]
    assert re.fullmatch(r"  rotate 2\.5 bilinear, angle searched in -5\.\.5: found 2\.(46875|5) \.\. 2\.(5|53125), " + tail, lines[-1]), lines[-1]
    assert cli.main(args + ["--json"]) == 0
    doc = json.loads(capsys.readouterr().out)[0]["rotations"]
    assert "search" not in doc[0] and doc[1]["search"] == [-10.0, 10.0] and doc[2]["search"] == [-5.0, 5.0]
    assert doc[2]["found_min"] <= 2.5 <= doc[2]["found_max"] and doc[2]["worst_angle_error"] <= 1 / 32 and doc[1]["worst_angle_error"] <= 1 / 32


# ---- billing, errors -------------------------------------------------------------------------------------------------------------
def test_the_call_is_billed_to_locate_and_resize():
    base = smooth(96, 64)
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_search(base, variants(base, 2), [(i % 2, 1.0, BICUBIC, FILL) for i in range(5)], -3, 3)
        t = c.timing()
    finally:
        c.enable_timing(False)
    assert t["locate"]["launches"] >= 1 and t["locate"]["work"] > 0 and t["resize"]["launches"] == 2 and t["resize"]["work"] == 2 * 5 * 2 * 96 * 64 * 3
    assert t["locate_coarse"]["launches"] == 1 and t["locate_coarse"]["work"] == 5 * 25 * (96 // 4) * (64 // 4)      # the ladder, nested
    assert all(v["launches"] == 0 for k, v in t.items() if k not in ("locate", "locate_coarse", "resize")), t


def test_errors():
    z = np.zeros((40, 40, 3), np.uint8)
    b, d, o, u = Dev(z), Dev(z[None]), Dev(z[None]), Dev(z[None])
    found, kept, h = (L.AngleFound * 1)(), np.zeros(1, np.uint64), ctx().handle
    k = kept.ctypes.data
    job = lambda **kw: (L.RotateJob * 1)(api.Rotate(1.0).job(kw.get("frame", 0), 40, 40))
    f = lib().ssw_rotate_search_attack_rgb8
    try:
        ok = job()
        assert f(h, b.ptr, d.ptr, 1, 31, 40, ok, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_DIMS
        assert f(h, b.ptr, d.ptr, 1, 40, 31, ok, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_DIMS
        assert f(h, b.ptr, d.ptr, 1, 65536, 40, ok, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_DIMS
        assert f(h, b.ptr, d.ptr, 1, 1 << 14, (1 << 13) + 1, ok, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_UNSUPPORTED
        for lo, hi in ((1.0, -1.0), (-45.5, 1.0), (0.0, 45.25), (float("nan"), 1.0), (0.0, float("inf"))):
            assert f(h, b.ptr, d.ptr, 1, 40, 40, ok, 1, lo, hi, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG
        assert f(h, None, d.ptr, 1, 40, 40, ok, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, None, 1, 40, 40, ok, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, None, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, ok, 1, -1.0, 1.0, None, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, ok, 1, -1.0, 1.0, o.ptr, u.ptr, None, None, k) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, ok, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, None) == L.SSW_ERR_BAD_ARG
        assert f(None, b.ptr, d.ptr, 1, 40, 40, ok, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, job(frame=1), 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG      # no such frame
        bad = job()
        bad[0].filter = 2
        assert f(h, b.ptr, d.ptr, 1, 40, 40, bad, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG
        bad = job()
        bad[0].forward[4] = float("inf")
        assert f(h, b.ptr, d.ptr, 1, 40, 40, bad, 1, -1.0, 1.0, o.ptr, u.ptr, found, None, k) == L.SSW_ERR_BAD_ARG
        for out, tur in ((d.ptr, u.ptr), (b.ptr, u.ptr), (o.ptr, d.ptr), (o.ptr, b.ptr), (o.ptr, o.ptr)):                  # an output over an input, or over the other
            assert f(h, b.ptr, d.ptr, 1, 40, 40, ok, 1, -1.0, 1.0, out, tur, found, None, k) == L.SSW_ERR_BAD_ARG
        assert f(h, None, None, 0, 0, 0, None, 0, 5.0, -5.0, None, None, None, None, None) == L.SSW_OK      # n_jobs == 0 is checked first
        ok[0].back[:] = [float("nan")] * 6                                                           # `back` is not read
        assert f(h, b.ptr, d.ptr, 1, 40, 40, ok, 1, -1.0, 1.0, o.ptr, None, found, None, k) == L.SSW_OK
        assert found[0].n_rungs == 9 and found[0].sad == 0 and kept[0] > 0
    finally:
        for x in (b, d, o, u):
            x.free()
