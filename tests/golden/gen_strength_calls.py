"""Writes strength_calls_parent.json: the library calls the host wrappers of the strength report make for the cases of
tests/fake_ssw.py, and what `cli strength` prints for its hand-made rows.  The file in the repository was written at commit
1a5cdf4, the parent of the refactor that tests/test_strength_calls_cpu.py holds to it; run this only to add a case, at a commit
whose wrappers are known good:  python tests/golden/gen_strength_calls.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import fake_ssw  # noqa: E402

doc = {"commit": "1a5cdf4", "cases": {name: fake_ssw.record(name) for name in fake_ssw.CASES},
       "cli_text": fake_ssw.cli_output(False), "cli_json": fake_ssw.cli_output(True)}
with open(os.path.join(HERE, "strength_calls_parent.json"), "w") as f:
    json.dump(doc, f, separators=(",", ":"))
    f.write("\n")
