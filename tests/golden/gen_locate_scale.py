"""Writes locate_scale_answers.json: what the numpy restatement of the scale ladder (tests/test_locate_scale_cpu.py:
locate_scaled_ref) answers on every named case -- (pw, ph, x, y, sad).  tests/test_locate_scale_cpu.py checks the file against
the restatement; the GPU tests compare the device with the file, so they stay quick.  Run from the repository root:
    python tests/golden/gen_locate_scale.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_locate_scale_cpu as T  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in list(T.SIX) + T.EXTRA:
        base, s, lo, hi, _ = T.case(name)
        out[name] = [int(v) for v in T.locate_scaled_ref(base, s, lo, hi)]
        print(name, out[name], flush=True)
    with open(T.ANSWERS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
