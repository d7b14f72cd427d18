"""The base reader of a batch extract (csrc/ssw_pipeline.hip: build_base_reader) against recorded accounts.

tests/golden/base_reader_accounts.json holds, for every case below, what ONE ssw_batch_extract left behind on a library built
from the commit BEFORE the base reader's transform got a builder of its own (loaded through SSW_LIB_PATH): per stage the timed
regions, the work and the algorithmic bytes (ssw_ctx_get_timing / _get_work / _get_traffic), every prune counter, and a SHA-256
of the extracted marks and the similarities.  The loaded library must leave the same: a stage that moved, a timer around other
work, a rate billed per tile or per job at another figure, or a launch that takes another part of the pass shows here.  The file
is a recorded fact -- never regenerate it from the code under test.

Shapes: H = 256, k = 64, the settings of tests/test_base_prune_gpu.py (FUSED), timers on; smooth frames with one white-noise
frame in the middle, so that a call has frames that skip tiles and a frame that needs every tile.  Widths, by the row pass's
route: 384 (one tile column per class: the eight exact energy launches), 1152 (a tail of 48-pair tiles), 2048 (of 64-pair
tiles), 2176 (three tile columns).  Calls: the default; base_energy_lowp = 0; base_prune = 0; merge_max_lines at its default
(8192: the eight classes of a pass launch one by one, as in the 4K benchmark); three chunks on two lanes.  The batch is the
smallest the planner gives the fused forward transform (under the default merge_max_lines: the smallest of more than 8192
lines, in whole groups of eight frames).

Integers and digests compare exactly, work and bytes to a relative 1e-9: the device adds the per-tile and per-job rates up with
atomic adds in the order the blocks arrive, which moves last bits only; a billing mistake is a whole tile's or launch's worth."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "base_reader_accounts.json")
H, K = 256, 64
WIDTHS = (384, 1152, 2048, 2176)
CALLS = ("default", "base_energy_lowp=0", "base_prune=0", "unmerged", "three-chunks")
MERGE_DEFAULT = 8192
REL = 1e-9


def _frames(n, w):
    """n smooth frames, the middle one white noise."""
    from test_base_prune_gpu import noise
    from test_base_select_gpu import smooth
    frames = smooth(n, H, w, 31 + w)
    frames[n // 2] = noise(1, H, w, 7 + w)[0]
    return frames


def _accounts(ctx):
    t = ctx.timing()
    return {s: [v["launches"], v["work"], v["bytes"]] for s, v in t.items() if v["launches"] or v["work"] or v["bytes"]}


def _one_call(G, w, n, chunk=0):
    """One batch extract of n frames on the current context of gpu_util: its accounts, counters and digest."""
    from test_base_prune_gpu import marks_for
    ctx = G.ctx()
    ctx.enable_timing(True)
    base, marks = _frames(n, w), marks_for(n, K)
    with np.errstate(all="ignore"):
        derived = G.batch_embed(base, marks)["rgb"]
    ctx.set_chunk_frames(chunk)
    try:
        ctx.reset_timing()
        ext, sims = G.batch_extract(base, derived, K, marks)
        got = {"stages": _accounts(ctx), "prune_stats": ctx.prune_stats(),
               "sha256": hashlib.sha256(ext.tobytes() + sims.tobytes()).hexdigest()}
    finally:
        ctx.set_chunk_frames(0)
    return got


def generate():
    """{case: accounts} of the loaded library, every width under every call."""
    import gpu_util as G
    from spread_spectrum_watermarking_amd.api import tuning
    from test_base_prune_gpu import FUSED
    out = {}
    with tuning(**FUSED):
        for w in WIDTHS:
            with G.fresh_ctx() as ctx:
                n = next(i for i in range(1, 65) if ctx.transform_plan(i, w, H)["fused_cols"])
                out[f"{w}x{H}x{n} default"] = _one_call(G, w, n)
                with tuning(base_energy_lowp=0):
                    out[f"{w}x{H}x{n} base_energy_lowp=0"] = _one_call(G, w, n)
                with tuning(base_prune=0):
                    out[f"{w}x{H}x{n} base_prune=0"] = _one_call(G, w, n)
                out[f"{w}x{H}x{3 * n} three-chunks"] = _one_call(G, w, 3 * n, chunk=n)
            with tuning(merge_max_lines=MERGE_DEFAULT), G.fresh_ctx() as ctx:
                n = next(i for i in range(8, 513, 8) if i * H > MERGE_DEFAULT and ctx.transform_plan(i, w, H)["fused_cols"])
                out[f"{w}x{H}x{n} unmerged"] = _one_call(G, w, n)
    return out


def record():
    """Writes the golden file from the loaded library: run once, with SSW_LIB_PATH naming a build of the parent commit."""
    lib = os.environ.get("SSW_LIB_PATH")
    assert lib, "record() is for a build of the parent commit: set SSW_LIB_PATH"
    cases = generate()
    with open(GOLDEN, "w") as f:
        json.dump({"_how": "tests/test_base_reader_accounts_gpu.py record() on a library built from the parent of the base-reader "
                           "builder refactor (SSW_LIB_PATH) -- per stage [timed regions, work, bytes], the prune counters, sha256 of "
                           "extracted marks + similarities of one ssw_batch_extract; recorded, never regenerated",
                   "cases": cases}, f, indent=1, sort_keys=True)
    print(f"{len(cases)} cases -> {GOLDEN}")


_WANT = {}
if os.path.exists(GOLDEN):           # (absent only while record() writes it: the first test below then fails)
    with open(GOLDEN) as _f:
        _WANT = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def replay():
    return generate()


@pytest.mark.gpu
def test_every_recorded_case_is_still_a_case(replay):
    assert set(replay) == set(_WANT)


def test_the_recorded_cases_take_the_routes_they_are_named_for():
    """The golden file itself: tail jobs only where the row pass has a tail and the bound is on, no base tile counted with
    base_prune = 0, the noise frame extended everywhere else."""
    assert len(_WANT) == len(WIDTHS) * len(CALLS) and all(sum(k.endswith(" " + c) for k in _WANT) == len(WIDTHS) for c in CALLS)
    for key, rec in _WANT.items():
        w, call, st = int(key.split("x")[0]), key.split(" ", 1)[1], rec["prune_stats"]
        tail = w != 384 and call not in ("base_energy_lowp=0", "base_prune=0")
        assert (st["base_tail_jobs"] > 0) == tail, key
        assert (st["base_tiles"] > 0) == (call != "base_prune=0"), key
        if call != "base_prune=0":
            assert 0 < st["base_frames_extended"] and st["base_tiles_computed"] < st["base_tiles"], key


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_WANT))
def test_base_reader_leaves_the_recorded_accounts(replay, case):
    got, want = replay.get(case), _WANT[case]
    assert got is not None, case
    print(case, json.dumps(got, sort_keys=True))
    assert got["sha256"] == want["sha256"], "extracted marks or similarities differ"
    assert got["prune_stats"] == want["prune_stats"]
    assert set(got["stages"]) == set(want["stages"])
    for stage, (launches, work, nbytes) in want["stages"].items():
        g = got["stages"][stage]
        assert g[0] == launches, (stage, "timed regions", g[0], launches)
        assert abs(g[1] - work) <= REL * abs(work), (stage, "work", g[1], work)
        assert abs(g[2] - nbytes) <= REL * abs(nbytes), (stage, "bytes", g[2], nbytes)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    record()
