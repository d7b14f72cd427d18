"""tests/tail_layout.py against the code, on the host: tests/cpp/tail_layout_test.cpp prints what pair_class_args answers for the
eight level-2 row classes of a width and the column tiles each tile column writes, in the gate's own arithmetic; the Python
restatement must say the same for the three layouts of tests/test_base_energy_gpu.py and the four of
tests/test_base_tail_layouts_gpu.py, and base_tail_plan -- what the row pass's builder goes by -- the same tile width, pairs
and chunks; two more widths must come out not eligible (264 terms; one tile column).  Then the table of those layouts as plain numbers -- what the GPU tests rely on."""
import os
import subprocess

import numpy as np
import pytest

import tail_layout as T
from conftest import ROOT

LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
LAYOUTS = [(1152, 0), (1152, 1), (2048, 1), (2176, 1), (2176, 0), (3840, 1), (4096, 1)]
INELIGIBLE = [(4224, 1), (1024, 1)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("tail_layout")), "tail_layout_test")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "cpp", "tail_layout_test.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe] + [f"{w}:{t}" for w, t in LAYOUTS + INELIGIBLE], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    per, cur = {}, None
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] == "L":
            cur = per[(int(f[1]), int(f[2]))] = {"split_bytes": int(f[3]), "classes": []}
        elif f[0] == "P":
            cur["plan"] = tuple(int(v) for v in f[1:])
        else:
            assert f[0] == "C" and int(f[1]) == len(cur["classes"]), line
            cur["classes"].append((tuple(int(v) for v in f[2:8]), [tuple(int(v) for v in r.split(":")) for r in f[8:]]))
    return per


@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: f"{l[0]}-tile48={l[1]}")
def test_restatement_equals_pair_class_args_and_the_gate(printed, lay):
    got, t = printed[lay], T.tail_layout(*lay)
    assert got["split_bytes"] == t.split_bytes                 # k-steps x (2 bases x hi / lo) x MFMA tiles x 1 KB + the maximum
    assert got["plan"] == (1, t.tw, t.pairs, t.chunks)         # eligible, first tail pair = the tile width, pairs, chunks
    assert len(got["classes"]) == 8
    for c, ((np_, kp, tiles_n, bn32, gsh, e2off), ranges) in enumerate(got["classes"]):
        assert (np_, kp, tiles_n, bn32, gsh, e2off) == (t.pairs, t.kp, len(t.tile_cols), t.bn32, T.GSH, T.E_SHAPED[c]), (c, T.CLASSES[c])
        assert ranges[1:] == [T.feeds(t, c, tn) for tn in range(1, tiles_n)], (c, T.CLASSES[c])
        assert ranges[0] == (0, (t.tw - 1) >> T.GSH)


@pytest.mark.parametrize("lay", INELIGIBLE, ids=lambda l: f"{l[0]}-tile48={l[1]}")
def test_the_plan_refuses_long_sums_and_single_tile_columns(printed, lay):
    got, t = printed[lay], T.tail_layout(*lay)
    assert (t.kp, t.pairs, len(t.tile_cols)) == {4224: (264, 264, 5), 1024: (64, 64, 1)}[lay[0]]      # why: > 256 terms | no tail
    assert got["plan"] == (0, 0, 0, 0) and got["split_bytes"] == 0
    for c, ((np_, kp, tiles_n, bn32, gsh, e2off), ranges) in enumerate(got["classes"]):
        assert (np_, kp, tiles_n, bn32, gsh, e2off) == (t.pairs, t.kp, len(t.tile_cols), t.bn32, T.GSH, T.E_SHAPED[c]), (c, T.CLASSES[c])
        assert ranges == []


def row(lay):
    t = T.tail_layout(*lay)
    return t.pairs, t.tile_cols, t.tail_pairs, t.mfma_tiles, t.chunks, t.kp, t.ksteps, t.column_tiles, T.seam_tiles(t)


def test_the_table_of_the_layouts():
    assert row((1152, 0)) == (72, (64, 8), 8, 1, 1, 72, 3, 9, [7])
    assert row((1152, 1)) == (72, (48, 24), 24, 2, 1, 72, 3, 9, [5])
    assert row((2048, 1)) == (128, (64, 64), 64, 4, 1, 128, 4, 16, [7])
    assert row((2176, 1)) == (136, (48, 48, 40), 88, 6, 1, 136, 5, 17, [5, 11])         # (the sixth MFMA tile half full)
    assert row((2176, 0)) == (136, (64, 64, 8), 72, 5, 1, 136, 5, 17, [7, 15])
    assert row((3840, 1)) == (240, (64, 64, 64, 48), 176, 11, 1, 240, 8, 30, [7, 15, 23])  # (the eighth k-step half empty)
    assert row((4096, 1)) == (256, (64, 64, 64, 64), 192, 12, 2, 256, 8, 32, [7, 15, 23])
    assert T.tail_layout(4224, 1).kp == 264                   # beyond the bound's 256 terms


def test_jobs_of_needed_tiles():
    """Away from a seam a needed tile runs the eight classes of its one tile column; a seam tile runs the tile column below it
    when that is a tail one, and the one entry of the five classes of E's shape in the tile column above."""
    e = sum(T.E_SHAPED)
    assert e == 5
    for lay in LAYOUTS:
        t = T.tail_layout(*lay)
        cols = len(t.tile_cols)
        assert T.jobs(t, []) == [] and T.jobs(t, range((t.tw - 1) >> 3)) == []
        assert len(T.jobs(t, range(t.column_tiles))) == 8 * (cols - 1)
        for tn in range(1, cols):
            own = T.own_tiles(t, tn)
            assert own and own[0] == tn * t.tw // 8, (lay, tn)
            for tile in (own[0], own[-1]):
                assert T.jobs(t, [tile]) == [(c, tn) for c in range(8)], (lay, tn, tile)
            seam = T.seam_tiles(t)[tn - 1]
            want = [(c, tn - 1) for c in range(8) if tn >= 2] + [(c, tn) for c in range(8) if T.E_SHAPED[c]]
            assert T.jobs(t, [seam]) == want and len(want) == 8 * (tn >= 2) + e, (lay, tn)
        assert T.head_width(t) == 128 * ((t.tw >> 3) - 1)
    t = T.tail_layout(3840, 1)
    assert T.own_tiles(t, 1) == list(range(8, 15)) and T.own_tiles(t, 3) == list(range(24, 30))
    assert T.own_tiles(T.tail_layout(2176, 0), 2) == [16]
    assert len(T.jobs(t, [8, 29])) == 16 and len(T.jobs(t, [15])) == 8 + e


def test_smooth_like_is_smooth():
    from test_base_prune_gpu import smooth
    a, b = smooth(2, 48, 256, 5), T.smooth_like(2, 48, 256, 5)
    assert np.abs(a.astype(np.float64) - b).max() <= 2e-7
