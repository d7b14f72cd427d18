"""wm::crop_attack and wm::crop_search_attack (include/ssw_crop.hpp) as a stand-alone program over a contract stub of the two C
functions (it has its own main; nothing is loaded into Python), plain and under ASan/UBSan: argument order, the packed
thumbnails, the answers of a search, a thrown status with nothing left alive."""
import subprocess

import pytest

from test_angle_cpu import build_exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_cpp_wrappers_against_a_stub(tmp_path, sanitize):
    exe = build_exe(tmp_path, "crop_wrappers_test", ["crop_wrappers_test.cpp", "crop_stub.cpp", "ssw_stub.cpp"], sanitize)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout.splitlines()[-1] == "crop wrappers: ok"
