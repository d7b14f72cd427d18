"""Writes locate_free_answers.json: what the numpy restatements answer on every named case of tests/test_locate_free_cpu.py --
per case and slack a the ladder's answer (locate_scaled_ref, run in full: the crop thumbnails over 240 .. 640 take 4 - 12 s
each) and the free answer (locate_free_ref), each as (pw, ph, x, y, sad).  tests/test_locate_free_cpu.py checks the file against
the restatements; the GPU tests compare the device with the file, so they stay quick.  Run from the repository root (a few
minutes; with names, only those cases are redone):
    python tests/golden/gen_locate_free.py [NAME ...]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_locate_free_cpu as T  # noqa: E402

if __name__ == "__main__":
    out = {}
    if sys.argv[1:]:                                                    # only the named cases; the others stay as recorded
        with open(T.ANSWERS) as f:
            out = json.load(f)
    for name in sys.argv[1:] or T.ALL:
        base, s, lo, hi, truth = T.case(name)
        a0, out[name] = None, {}
        for a in T.slacks(name):
            best, a0, _ = T.locate_free_ref(base, s, lo, hi, a, start=a0, details=True)
            out[name][str(a)] = {"ladder": [int(v) for v in a0], "free": [int(v) for v in best]}
            print(name, "a", a, "ladder", a0, "free", best, "truth", truth, flush=True)
    with open(T.ANSWERS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
