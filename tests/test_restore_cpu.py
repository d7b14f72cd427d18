"""Tracing attacked copies (restore on the device, then trace): the parts that need no GPU -- the C ABI symbols, their
citations and contract, the struct layout, the Python and CLI surfaces, the numpy restatement of Rgba<u8>::blend that the GPU
tests use as their yardstick, and the C++ wrapper compiling against the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli

NAMES = ("ssw_restore_rgb8", "ssw_fingerprint_trace_restored_host_rgb8", "ssw_reader_trace_restored_host_rgb8")
LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
INCLUDE = os.path.join(ROOT, "include")


def header():
    return open(os.path.join(INCLUDE, "ssw.h")).read()


def test_symbols_declared_exported_bound_and_cited():
    text = header()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        decl = text.index(n + "(")
        assert hasattr(lib, n), n
        assert n in L.SIGNATURES, n
        comment = text[text.rfind("/*", 0, decl):decl]
        assert re.search(r"attack_resize\.rs:31-36", comment) and re.search(r"attack_crop\.rs:56-70", comment), n
    for n in NAMES[1:]:
        decl = text.index(n + "(")
        assert re.search(r"algorithm\.rs:\d+", text[text.rfind("/*", 0, decl):decl]), n
    assert len(L.SIGNATURES["ssw_restore_rgb8"][1]) == 8
    # the five outputs, marks and threshold exactly as the existing host forms
    assert L.SIGNATURES["ssw_fingerprint_trace_restored_host_rgb8"][1][9:] == L.SIGNATURES["ssw_fingerprint_trace_host_rgb8"][1][8:]
    assert L.SIGNATURES["ssw_reader_trace_restored_host_rgb8"][1][6:] == L.SIGNATURES["ssw_reader_trace_host_rgb8"][1][4:]


def test_header_states_the_contract():
    text = header()
    doc = text[text.index("tracing attacked copies"):text.index("ssw_reader_trace_restored_host_rgb8(")]
    for phrase in ("parity unpinned", "bit for bit", "in the order of host_suspects", "not touched by any restore launch",
                   "today's trace", "largest suspect of the call", "bounded for any n_suspects", "SSW_ERR_BAD_ARG", "SSW_ERR_K_TOO_LARGE",
                   "SSW_ERR_NOT_BASE", "SSW_ERR_UNSUPPORTED", "SSW_STAGE_RESIZE", "truncated toward zero", "af = ba + fa - ba * fa"):
        assert phrase in doc, phrase


def test_struct_layout_equal_in_c_and_ctypes(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ssw.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(ssw_placement), offsetof(ssw_placement, w), offsetof(ssw_placement, h), offsetof(ssw_placement, channels), "
                   "offsetof(ssw_placement, x), offsetof(ssw_placement, y), offsetof(ssw_placement, pw), offsetof(ssw_placement, ph)); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", INCLUDE, str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    P = L.Placement
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in ("w", "h", "channels", "x", "y", "pw", "ph")]
    assert [f for f, _ in P._fields_] == ["w", "h", "channels", "x", "y", "pw", "ph"]


def test_python_surface():
    import spread_spectrum_watermarking_amd as wm
    assert wm.Placement is api.Placement and callable(wm.restore)
    p = api.Placement()
    assert (p.x, p.y, p.w, p.h) == (0, 0, None, None)
    W, H = 640, 444
    f = lambda pl, sw, sh, c=3: tuple(getattr(api._resolve_placement(pl, sw, sh, c, W, H), n) for n in ("w", "h", "channels", "x", "y", "pw", "ph"))
    # None, or no size at (0, 0): whole frame when the suspect's size differs from the base's ...
    assert f(None, 320, 222) == (320, 222, 3, 0, 0, W, H)
    assert f(api.Placement(), 80, 55, 4) == (80, 55, 4, 0, 0, W, H)
    assert f(None, 1280, 888) == (1280, 888, 3, 0, 0, W, H)
    # ... and own size at (x, y) otherwise
    assert f(None, W, H, 4) == (W, H, 4, 0, 0, W, H)
    assert f(api.Placement(160, 60), 400, 320) == (400, 320, 3, 160, 60, 400, 320)
    assert f(api.Placement(0, 5), 400, 320) == (400, 320, 3, 0, 5, 400, 320)
    assert f(api.Placement(160, 60, 400, 320), 200, 160) == (200, 160, 3, 160, 60, 400, 320)
    for bad in (api.Placement(0, 0, 5, None), api.Placement(-1, 0), api.Placement(0, 0, 0, 0)):
        with pytest.raises(ValueError):
            f(bad, 10, 10)
    arrs, ptrs, pl = api._placed_suspects([np.zeros((4, 6, 4), np.uint8), np.zeros((H, W, 3), np.uint8)], [api.Placement(1, 2), None], W, H)
    assert len(ptrs) == 2 and (pl[0].w, pl[0].h, pl[0].channels, pl[0].x, pl[0].y, pl[0].pw, pl[0].ph) == (6, 4, 4, 1, 2, 6, 4)
    assert (pl[1].channels, pl[1].pw, pl[1].ph) == (3, W, H)
    for bad_suspects, bad_pl in (([np.zeros((4, 6, 2), np.uint8)], [None]), ([np.zeros((4, 6, 3), np.float32)], [None]),
                                 ([np.zeros((4, 6, 3), np.uint8)], [None, None]), ([], [])):
        with pytest.raises(ValueError):
            api._placed_suspects(bad_suspects, bad_pl, W, H)
    # placements=None: exactly as before -- one size for all, an alpha channel cut off, a mismatched shape raises
    with pytest.raises(ValueError):
        api._frame_ptrs([np.zeros((4, 6, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)])
    with pytest.raises(ValueError):
        api._frame_ptrs([np.zeros((4, 5, 3), np.uint8)], 6, 4)
    import inspect
    assert inspect.signature(api.Reader.trace).parameters["placements"].default is None
    assert inspect.signature(api.trace_many).parameters["placements"].default is None
    src = inspect.getsource(api.Reader.trace)
    assert src.index("SSW_ERR_LENGTH_MISMATCH") > src.index("if placements is not None")      # the old path still raises it
    assert "whole frame" in api.restore.__doc__ and "own size at (x, y)" in api.restore.__doc__


def test_place_parser():
    p = cli.build_parser()
    common = ["trace", "cat.jpg", "--suspects", "a.png", "b.png", "--marks", "x.json"]
    a = p.parse_args(common + ["--place", "a.png=10,20"])
    assert a.placements == {"a.png": api.Placement(10, 20, None, None)}
    a = p.parse_args(common + ["--place", "a.png=10,20,300x200", "--place", "b.png=0,0"])
    assert a.placements == {"a.png": api.Placement(10, 20, 300, 200), "b.png": api.Placement(0, 0, None, None)}
    assert p.parse_args(common).placements == {}
    assert cli.parse_place("dir/a=b.png=1,2,3x4") == ("dir/a=b.png", api.Placement(1, 2, 3, 4))
    for bad in ("a.png", "a.png=10", "a.png=10,20,30", "a.png=10,20,300x", "a.png=10,20,0x5", "a.png=-1,2", "a.png=x,y", "=1,2", "a.png=1,2,3x4,5"):
        with pytest.raises(ValueError):
            cli.parse_place(bad)
        with pytest.raises(SystemExit):
            p.parse_args(common + ["--place", bad])
    with pytest.raises(SystemExit):
        p.parse_args(common + ["--place", "c.png=1,2"])                    # not among --suspects
    with pytest.raises(SystemExit):
        p.parse_args(common + ["--place", "a.png=1,2", "--place", "a.png=3,4"])
    # the other subcommands parse as before
    t = p.parse_args(["test", "b.png", "w.png", "m.json"])
    assert (t.command, t.base, t.watermarked, t.watermark_files, t.similarity_exceed) == ("test", "b.png", "w.png", ["m.json"], 6.0)
    w = p.parse_args(["watermark", "f.png", "--length", "10", "-p"])
    assert (w.command, w.file, w.length, w.ordering, w.alpha, w.method, w.print_similarity) == ("watermark", "f.png", 10, "energy", 0.1, "option2", True)
    f = p.parse_args(["fingerprint", "f.png", "--copies", "3"])
    assert (f.command, f.file, f.copies, f.length) == ("fingerprint", "f.png", 3, 1000)
    for bad in (["trace", "cat.jpg", "--marks", "x.json"], ["fingerprint", "f.png"], ["test", "b.png"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_numpy_blend_against_hand_worked_bytes():
    """The yardstick of tests/test_restore_gpu.py, checked against values worked by hand in f32:
        bg = O / 255, fg = R / 255, fa = a / 255;  af = (1 + fa) - 1 * fa;  out = (fg * fa + bg * (1 - fa)) / af;  byte = trunc(255 * out)."""
    from test_restore_gpu import blend_ref
    f = np.float32
    px = lambda o, r: tuple(int(v) for v in blend_ref(np.array([o], np.uint8), np.array([r], np.uint8))[0])
    assert px((10, 20, 30), (200, 100, 50, 0)) == (10, 20, 30)               # alpha 0: the original
    assert px((10, 20, 30), (200, 100, 50, 255)) == (200, 100, 50)           # alpha 255: the suspect
    hand = lambda o, r, a: int(f(255) * ((((f(r) / f(255)) * (f(a) / f(255))) + ((f(o) / f(255)) * f(1)) * (f(1) - f(a) / f(255))) / ((f(1) + f(a) / f(255)) - f(1) * (f(a) / f(255)))))
    # a = 128, the case where 1 + fa - fa != 1 in f32: fa = 0.5019608 has a 2^-24 bit that 1 + fa (ulp 2^-23) drops, so
    # af = 1 - 2^-24 = 0.99999994.  Red 255 over 0: 255 * (fa / af) = 128.00002 -> 128.  Blue 0 over 255: (1 - fa) / af =
    # 0.49803925, times 255 = 127.00001 -> 127 (truncated; with af == 1 it would be 126.99999.. -> 126).
    fa = f(128) / f(255)
    af = (f(1) + fa) - f(1) * fa
    assert af == np.nextafter(f(1), f(0)) and af != f(1)
    assert int(f(255) * ((f(1) - fa) / f(1))) == 126                          # what a fused or reordered af would give
    assert px((0, 0, 255), (255, 0, 0, 128)) == (128, 0, 127) == (hand(0, 255, 128), hand(0, 0, 128), hand(255, 0, 128))
    # a = 1: fa = 0.003921569, af == 1 exactly; 255 under 0 keeps 255 * (1 - fa) = 254.0 -> 254, 0 under 255 gets 255 * fa * 1 = 1
    fa = f(1) / f(255)
    assert (f(1) + fa) - f(1) * fa == f(1)
    assert px((255, 128, 0), (0, 128, 255, 1)) == (254, 128, 1) == (hand(255, 0, 1), hand(128, 128, 1), hand(0, 255, 1))
    # every (o, r, a) on a coarse grid equals the scalar restatement
    grid = [0, 1, 2, 63, 127, 128, 129, 200, 254, 255]
    for a in (1, 2, 3, 127, 128, 129, 253, 254):
        for o in grid:
            for r in grid:
                assert px((o, o, o), (r, r, r, a))[0] == hand(o, r, a), (o, r, a)


CPP = r"""
#include "ssw.hpp"
int main() {
    wm::Context ctx(0);
    wm::ImageRgb8 img(8, 8), s0(4, 4), cut(3, 2);
    wm::ImageRgba8 s1(8, 8);
    wm::Reader base = wm::Reader::base(ctx, img);
    wm::MarkBuf a = wm::MarkBuf::generate_normal(4), b = wm::MarkBuf::generate_normal(4);
    wm::Placement at{2, 3, 0, 0}, scaled{1, 1, 6, 4};
    wm::TraceResult r = base.trace(img, {s0, s1, cut, cut}, {wm::Placement::whole_frame(img), wm::Placement(), at, scaled}, {&a, &b}, 6.0f);
    if (r.best[0] == wm::TraceResult::none) return 2;
    return (int)(r.extracted.size() + r.sims.size() + r.best.size()) - 12 + (int)sizeof(ssw_placement) - 28;
}
"""


def test_cpp_placement_and_rgba_compile_and_link(tmp_path):
    src = tmp_path / "restore.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "restore")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INCLUDE, str(src), "-o", exe,
                    "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert os.path.exists(exe)
