"""Writes rotate_search_calls_parent.json: the library calls and allocations of a strength report whose rotations are all KNOWN
(no `search`), on the recording stand-in of tests/fake_ssw.py, as the commit named in the file made them -- the record
tests/test_rotate_search_cpu.py holds the report to once `Rotate` has a `search` field.  Run at a checkout of that commit, from
the repository root, with the commit's short hash:
    python tests/golden/gen_rotate_search_calls.py HASH
SPREAD_SPECTRUM_PACKAGE_ROOT (optional): the directory of the package to record, when it is not this tree's."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.environ.get("SPREAD_SPECTRUM_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import fake_ssw  # noqa: E402
from spread_spectrum_watermarking_amd import api  # noqa: E402

W, H = 40, 36                        # both sides at least 32: the frame a searched rotation accepts as well
RECORD = os.path.join(HERE, "rotate_search_calls_parent.json")


def frame():
    return np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)


def known():
    return [api.Rotate(0.5), api.Rotate(2.0, "bilinear")]


def report(ctx, rotations, **more):
    kw = dict(k=50, copies=3, sizes=(2,), methods=("average",), seed=1)
    kw.update(more)
    return api.strength_report(frame(), [0.02, 0.1], ctx=ctx, rotations=rotations, **kw)


def record(rotations, **more):
    ctx = fake_ssw.fake_context()
    report(ctx, rotations, **more)
    return {"calls": json.loads(json.dumps(ctx._lib.calls)), "allocs": sorted(ctx._lib.allocs), "live": len(ctx._lib.live)}


if __name__ == "__main__":
    with open(RECORD, "w") as f:
        json.dump({"commit": sys.argv[1], "known": record(known()), "known_ssim": record(known(), ssim=True)}, f, separators=(",", ":"))
        f.write("\n")
