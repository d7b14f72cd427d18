"""The host code around the strength report's kernels (api.quality, ssim, collude, jpeg, filter, strength_report and the CLI's
`strength`) against what it did at the commit tests/golden/strength_calls_parent.json names: the same library calls in the same
order with the same arguments, the same allocations, the same printed text -- on a recording stand-in for the library
(tests/fake_ssw.py), no GPU."""
import collections
import json
import os

import numpy as np
import pytest

import fake_ssw
from conftest import GOLDEN
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api

with open(os.path.join(GOLDEN, "strength_calls_parent.json")) as f:
    PARENT = json.load(f)


def test_the_record_holds_every_case():
    assert PARENT["commit"] == "1a5cdf4" and set(PARENT["cases"]) == set(fake_ssw.CASES)
    assert all(case["live"] == 0 for case in PARENT["cases"].values())
    report = PARENT["cases"]["report_jpeg_filters_ssim"]
    assert len(report["calls"]) + 2 * len(report["allocs"]) == 78


@pytest.mark.parametrize("name", list(fake_ssw.CASES))
def test_same_library_calls_same_allocations_nothing_live(name):
    lib, _ = fake_ssw.run_case(name)
    parent = PARENT["cases"][name]
    got = json.loads(json.dumps(lib.calls))
    assert len(got) == len(parent["calls"])
    for i, (g, p) in enumerate(zip(got, parent["calls"])):
        assert g == p, (i, g, p)
    assert sorted(lib.allocs) == parent["allocs"]
    assert lib.live == {}


def test_the_fake_library_returns_what_the_shapes_promise():
    _, rows = fake_ssw.run_case("report_jpeg_filters_ssim")
    assert [r.alpha for r in rows] == [0.02, 0.1]
    assert all(len(r.quality) == len(r.ssim) == 3 and len(r.collusions) == 2 for r in rows)
    assert [[j.quality for j in r.jpeg] for r in rows] == [[75, 30]] * 2 and [[f.filter for f in r.filters] for r in rows] == [["blur 1", "median 3"]] * 2
    _, nested = fake_ssw.run_case("filter_cap_1")
    assert [len(per) for per in nested] == [3] * 4 and nested[3][2].shape == (fake_ssw.H, fake_ssw.W, 3)
    _, s = fake_ssw.run_case("ssim_maps_one_per_copy")
    assert len(s) == 5 and all(x.map.shape == api._ssim_windows(fake_ssw.W, fake_ssw.H)[::-1] for x in s)
    assert len(fake_ssw.run_case("collude_cap_1")[1]) == len(fake_ssw.COALITIONS)


def cases_that_call(call):
    return [case for case in fake_ssw.CASES if any(c[0] == call for c in PARENT["cases"][case]["calls"])]


@pytest.mark.parametrize("case,call", [(case, call) for call in ("ssw_jpeg_rgb8", "ssw_quality_rgb8", "ssw_fingerprint_trace_rgb8")
                                       for case in cases_that_call(call)])
def test_an_error_from_the_library_leaves_nothing_live(case, call):
    """The wrappers free what they allocated on every way out: with SswError still in hand (and its traceback, which holds every
    frame's locals), no allocation is live.  At 1a5cdf4 up to 18 buffers were, until the traceback went."""
    ctx = fake_ssw.fake_context({call: L.SSW_ERR_BAD_ARG})
    with pytest.raises(api.SswError) as e:
        fake_ssw.run_case(case, ctx)
    assert e.value.status == L.SSW_ERR_BAD_ARG and e.traceback is not None
    assert ctx._lib.calls[-1][0] == call and ctx._lib.allocs and ctx._lib.live == {}


@pytest.mark.parametrize("call", ["ssw_copy_to_dev", "ssw_copy_to_host", "ssw_ssim_rgb8", "ssw_filter_rgb8", "ssw_collude_rgb8"])
def test_a_failed_copy_or_other_call_leaves_nothing_live(call):
    assert cases_that_call(call)
    for case in cases_that_call(call):
        ctx = fake_ssw.fake_context({call: L.SSW_ERR_HIP})
        with pytest.raises(api.SswError) as e:
            fake_ssw.run_case(case, ctx)
        assert e.value.status == L.SSW_ERR_HIP and ctx._lib.live == {}, (call, case)


# ---- the grouping function against the three loops it replaced ---------------------------------------------------------------
def parent_collude_groups(co, fb, cap):
    """api.collude's loop at 1a5cdf4; co: (count, members) per coalition.  Returns (used, g0, g1, local members per job)."""
    groups, g0 = [], 0
    while g0 < len(co):
        used, g1 = [], g0
        while g1 < len(co):
            more = [i for i in dict.fromkeys(co[g1][1][:co[g1][0]]) if i not in used]
            if g1 > g0 and (len(used) + len(more) + g1 - g0 + 1) * fb > cap:
                break
            used += more
            g1 += 1
        where = {i: j for j, i in enumerate(used)}
        groups.append((used, g0, g1, [[where[i] for i in members[:count]] for count, members in co[g0:g1]]))
        g0 = g1
    return groups


def parent_frame_order_groups(jobs, fb, cap):
    """the loop of api.jpeg and api.filter at 1a5cdf4; jobs: (frame, parameter) in frame order"""
    groups, g0 = [], 0
    while g0 < len(jobs):
        used, g1 = [], g0                                     # the jobs are in frame order: a group's frames are a run
        while g1 < len(jobs):
            new = not used or used[-1] != jobs[g1][0]
            if g1 > g0 and (len(used) + new + g1 - g0 + 1) * fb > cap:
                break
            if new:
                used.append(jobs[g1][0])
            g1 += 1
        groups.append((used, g0, g1, [[i - used[0]] for i, _ in jobs[g0:g1]]))
        g0 = g1
    return groups


def new_groups(job_frames, fb, cap, monkeypatch):
    monkeypatch.setattr(api, "UPLOAD_GROUP_BYTES", cap)
    out = []
    for used, g0, g1 in api._job_groups(job_frames, fb):
        where = {i: j for j, i in enumerate(used)}
        out.append((used, g0, g1, [[where[i] for i in job] for job in job_frames[g0:g1]]))
    return out


FB = 1000
CAPS = [1, FB, 3 * FB - 1, 5 * FB, 256 << 20]


@pytest.mark.parametrize("cap", CAPS)
def test_groups_of_single_frame_jobs_are_the_jpeg_and_filter_loop_s(cap, monkeypatch):
    for n_frames, per_frame in ((1, 1), (1, 5), (4, 3), (7, 1), (16, 3), (3, 9)):
        jobs = [(i, p) for i in range(n_frames) for p in range(per_frame)]
        job_frames = [(i,) for i, _ in jobs]
        want = parent_frame_order_groups(jobs, FB, cap)
        assert new_groups(job_frames, FB, cap, monkeypatch) == want
        # and the general loop, fed one frame per job in frame order, is the special one
        assert parent_collude_groups([(1, [i]) for i, _ in jobs], FB, cap) == want
        assert sum(g1 - g0 for _, g0, g1, _ in want) == len(jobs) and all(g1 > g0 for _, g0, g1, _ in want)


@pytest.mark.parametrize("cap", CAPS)
def test_groups_of_coalitions_are_the_collude_loop_s(cap, monkeypatch):
    rng = np.random.default_rng(cap % 9973)
    sets = [[(c, list(range(c))) for c in range(1, 17)],                                   # 1 .. 16 members, sharing a prefix
            [(4, [2, 2, 0, 2]), (1, [5]), (3, [5, 5, 5]), (16, [1] * 16), (2, [0, 7])]]     # repeats
    for _ in range(40):
        n_copies = int(rng.integers(1, 24))
        sets.append([(int(c), [int(i) for i in rng.integers(0, n_copies, c)]) for c in rng.integers(1, 17, int(rng.integers(1, 12)))])
    for co in sets:
        padded = [(count, members + [0] * (16 - count)) for count, members in co]         # as ssw_coalition holds them
        want = parent_collude_groups(padded, FB, cap)
        assert new_groups([members for _, members in co], FB, cap, monkeypatch) == want
        assert want[0][1] == 0 and want[-1][2] == len(co) and all(a[2] == b[1] for a, b in zip(want, want[1:]))
        if cap <= FB:
            assert len(want) == len(co)                          # a group always takes its first job, and here no second


def test_the_cap_is_read_at_the_call(monkeypatch):
    jobs = [(i,) for i in range(6)]
    assert len(api._job_groups(jobs, FB)) == 1
    monkeypatch.setattr(api, "UPLOAD_GROUP_BYTES", 1)
    assert len(api._job_groups(jobs, FB)) == 6


# ---- the strength command ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_json", [False, True])
def test_the_strength_command_prints_what_it_printed(as_json):
    """Hand-made rows (a NaN strongest innocent, innocents accused, JPEG and filter rows with and without SSIM, an infinite PSNR)
    through cli.cmd_strength, byte for byte."""
    rows = fake_ssw.cli_rows()
    assert any(c.strongest_innocent != c.strongest_innocent for c in rows[0].collusions) and any(c.accused for c in rows[0].collusions)
    assert rows[0].ssim and not rows[1].ssim and rows[1].jpeg and rows[1].filters and any(j.accused for j in rows[0].jpeg)
    assert any(f.psnr_max == float("inf") for f in rows[0].filters) and collections.Counter(type(r) for r in rows) == {api.StrengthRow: 3}
    assert fake_ssw.cli_output(as_json) == PARENT["cli_json" if as_json else "cli_text"]
    if as_json:
        json.loads(PARENT["cli_json"])
