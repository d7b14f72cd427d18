"""Writes locate_turned_answers.json: what the numpy restatement of the search for turned cut-outs
(tests/test_locate_turned_cpu.py: locate_turned_ref) answers on the eight cases of the marked cat -- the answer
(n, x, y, tw, th, sad) and every rung's (D, n_j, x, y).  tests/test_locate_turned_cpu.py checks the file against the
restatement; the GPU tests compare the device with the file, so they stay quick.  Run from the repository root:
    python tests/golden/gen_locate_turned.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_locate_turned_cpu as T  # noqa: E402

if __name__ == "__main__":
    out = {}
    for c in T.CASES:
        f = T.found(c)
        out[T.name_of(c)] = {"answer": [int(v) for v in f.answer()], "rungs": [[int(v) for v in r] for r in f.rung_rows()]}
        print(T.name_of(c), out[T.name_of(c)]["answer"], f.angle, f.centre, flush=True)
    with open(T.ANSWERS, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
