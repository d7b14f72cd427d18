"""wm::locate_free (include/ssw_locate_free.hpp) as a stand-alone program over a contract stub of the C function (it has its
own main; nothing is loaded into Python), plain and under ASan/UBSan: argument order, ranges and slacks that go with their
suspects, the answers, a thrown status with nothing left alive."""
import subprocess

import pytest

from test_angle_cpu import build_exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_cpp_wrapper_against_a_stub(tmp_path, sanitize):
    exe = build_exe(tmp_path, "locate_free_wrappers_test", ["locate_free_wrappers_test.cpp", "locate_free_stub.cpp", "ssw_stub.cpp"], sanitize)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout.splitlines()[-1] == "locate_free wrappers: ok"


def test_every_size_with_a_resize_tile_gets_an_item(tmp_path):
    """csrc/locate_free_tile.hpp on the host (tests/cpp/locate_free_tile_test.cpp): the tile is chosen with the window of the
    original counted, so no band of scale factors -- the one-third thumbnail, x 0.95, RGBA x 1.2 -- is refused for its LDS."""
    import os
    from conftest import ROOT
    libdir = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
    exe = os.path.join(str(tmp_path), "locate_free_tile_test")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "cpp", "locate_free_tile_test.cpp"),
                    "-I", os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, "-L", libdir, "-lssw_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "locate_free tiles: ok", out.stdout + out.stderr
