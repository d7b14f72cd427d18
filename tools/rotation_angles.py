"""The 64 angles of tests/golden/rotation_angles.json: what tests/test_rotate_cpu.py feeds to rotation_matrix of
csrc/affine_tables.hpp and to Python's own.  Deterministic: `python tools/rotation_angles.py` rewrites the file as it is.
Multiples of 0.1 degree (whose cosines need the decimal rounding most), the neighbours of every multiple of 90 degrees a
double can tell apart from it, negative angles and angles beyond a full turn."""
import json
import math
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def angles() -> list:
    out = [k * 0.1 for k in (1, 2, 3, 4, 5, 7, 10, 13, 25, 75, 300, 450, 599, 600, 899, 901, 1799, 1801, 2705, 3599)]
    for q in (0.0, 90.0, 180.0, 270.0, 360.0):
        out += [q, math.nextafter(q, -1000.0), math.nextafter(q, 1000.0), q - 1e-9, q + 1e-9]
    out += [-0.1, -0.25, -1.0, -7.5, -30.0, -45.0, -90.0, -179.9, -180.0, -270.0, -359.9, -360.0, -1e-20, -720.5]
    out += [361.0, 725.3, 1e6 + 0.5, 33.333333333333336, 57.29577951308232]
    assert len(out) == 64 and len(set(out)) == 64
    return out


if __name__ == "__main__":
    with open(os.path.join(ROOT, "tests", "golden", "rotation_angles.json"), "w") as f:
        json.dump({"angles": [a.hex() for a in angles()], "as_decimals": [repr(a) for a in angles()]}, f, indent=1)
        f.write("\n")
