"""Builds and runs the C++ host-side mirror (include/ssw.hpp) against libssw_hip.so.

CPU part: the wrapper header and the test program compile and link (no GPU needed).
GPU part: the doc-test flow of the reference (lib.rs:24-66) through the C++ types, checked
against the CPU oracle on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "crate_surface_test.cpp")
LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")


def build(tmpdir):
    exe = os.path.join(str(tmpdir), "crate_surface_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_class_major_layout_maps_on_the_host(tmp_path):
    """csrc/dct_pair_common.hpp's column orders of the intermediate planes (deep transforms): bijections, inverses of each
    other, and consistent with the output maps of the GEMM launch classes -- compiled for the host, no device code runs."""
    exe = os.path.join(str(tmp_path), "class_layout_test")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "cpp", "class_layout_test.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "ok"


def test_transform_planner_on_the_host(tmp_path):
    """csrc/dct_plan.hpp: the strategy of every pass for the shapes DESIGN 4.0 names, the folding levels, the odd split off and
    lowered thresholds (ssw_tuning_set), and the SSW_PLAN_* flags as a function of the plan -- no GPU, no context."""
    exe = os.path.join(str(tmp_path), "dct_plan_test")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "cpp", "dct_plan_test.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "ok", out


def test_workspace_enumeration_on_the_host(tmp_path):
    """csrc/ssw_internal.hpp: the one enumeration of a context's workspace buffers that teardown and the automatic pass size
    run off -- every Buf once, under its own name, none left out, and exactly the lanes' planes, operand slots, compact planes,
    index lists, gathered bases and prune tables counted towards the held total -- no GPU, no HIP call."""
    exe = os.path.join(str(tmp_path), "workspace_test")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "cpp", "workspace_test.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout


def test_pair_class_table_on_the_host(tmp_path):
    """csrc/dct_pair_class.hpp: the launch-class table answers what the per-class launch code answered before the table existed
    (tests/golden/pair_class_parent.txt: all 33600 tuples of class, pass, direction, layout, length, the rejected ones included,
    and the class rows of the pruned plans), and agrees with ForwardClassLayout, with a partition of the frequencies per pass
    and with the flop the level-2 builders assume; the class sources of the pruned row pass answer what the loop they replaced
    resolved (tests/golden/prune_class_src_parent.txt) -- no GPU, no context."""
    exe = os.path.join(str(tmp_path), "pair_class_test")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "cpp", "pair_class_test.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "pair_class_parent.txt"),
                          os.path.join(ROOT, "tests", "golden", "prune_class_src_parent.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout


def test_cpp_wrappers_compile_and_link(tmp_path):
    exe = build(tmp_path)
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_doc_test_flow_matches_oracle(tmp_path):
    from oracle import oracle as O
    exe = build(tmp_path)
    w, h, k = 320, 180, 200
    rgb = O.synth_frame(5, 0, w, h)
    mark = np.random.default_rng(5).standard_normal(k).astype(np.float32)
    p = lambda n: os.path.join(str(tmp_path), n)
    rgb.tofile(p("rgb.f32")); mark.tofile(p("mark.f32"))
    out = subprocess.run([exe, p("rgb.f32"), str(w), str(h), p("mark.f32"), str(k), p("marked.f32"), p("ext.f32"), p("marked8.u8")],
                         check=True, capture_output=True, text=True).stdout.split()
    vals = dict(zip(out[::2], out[1::2]))
    marked = np.fromfile(p("marked.f32"), np.float32).reshape(h, w, 3)
    ext = np.fromfile(p("ext.f32"), np.float32)
    ref_marked = O.embed_frame(rgb, mark)
    ref_ext, ref_sim = O.extract_frame(rgb, ref_marked, mark)
    assert np.abs(marked - ref_marked).max() <= 2e-7       # default = canonical precision
    assert np.abs(ext - ref_ext).max() <= 1e-5 * np.maximum(1.0, np.abs(ref_ext)).max()
    assert abs(float(vals["similarity"]) - ref_sim) < 1e-4
    assert vals["exceeds6"] == "1" and vals["consumed_ok"] == "1" and vals["too_large_ok"] == "1"
    assert abs(float(vals["random"])) < 5.0
    coef = O.dct2d(O.rgb_to_yiq(rgb)[0])
    assert int(vals["first_index"]) == int(O.indices(coef, k=1)[0])
    # the 8-bit leg (ImageRgb8 in, mark_rgb8 out): same bytes through the oracle
    img8 = O.f32_to_u8(rgb)
    marked8 = np.fromfile(p("marked8.u8"), np.uint8).reshape(h, w, 3)
    o_marked8 = O.f32_to_u8(O.embed_frame(O.u8_to_f32(img8), mark))
    assert np.mean(marked8 == o_marked8) >= 0.9999
    _, o_sim8 = O.extract_frame(O.u8_to_f32(img8), O.u8_to_f32(marked8), mark)
    assert abs(float(vals["similarity8"]) - o_sim8) < 1e-4 * max(1.0, abs(o_sim8))


def build_strength_wrappers(tmpdir, *flags):
    exe = os.path.join(str(tmpdir), "strength_wrappers_test")
    return exe, subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "include"),
                                os.path.join(ROOT, "tests", "cpp", "strength_wrappers_test.cpp"), "-o", exe,
                                "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)


def test_cpp_strength_wrappers_compile_without_warnings(tmp_path):
    exe, done = build_strength_wrappers(tmp_path, "-Wall", "-Wextra")
    assert os.path.exists(exe) and done.stderr == "", done.stderr


@pytest.mark.gpu
def test_cpp_strength_wrappers_answer_what_the_python_ones_do(tmp_path):
    """wm::quality, ssim, collude, jpeg and filter of include/ssw.hpp, run: two 24 x 40 copies of an original, every byte and
    every statistic against api.quality, ssim, collude, jpeg and filter on the same frames -- both routes end in the same
    library calls, so nothing may differ."""
    import spread_spectrum_watermarking_amd as wm
    exe, _ = build_strength_wrappers(tmp_path)
    h, w = 24, 40
    rng = np.random.default_rng(11)
    original = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    copies = [np.clip(original.astype(np.int16) + rng.integers(-6, 7, original.shape), 0, 255).astype(np.uint8) for _ in range(2)]
    p = lambda n: os.path.join(str(tmp_path), n)
    for name, frame in (("original.u8", original), ("copy0.u8", copies[0]), ("copy1.u8", copies[1])):
        frame.tofile(p(name))
    run = subprocess.run([exe, p("original.u8"), p("copy0.u8"), p("copy1.u8"), str(w), str(h), p("frames.u8")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = [[int(v) for v in line.split()[1:]] for line in run.stdout.splitlines()]
    assert [line.split()[0] for line in run.stdout.splitlines()] == ["quality"] * 2 + ["ssim"] * 2
    ctx = wm.Context(0)
    assert lines[:2] == [[*q.sse, q.sse_luma, q.changed, q.max_abs, q.pixels] for q in wm.quality(original, copies, ctx)]
    assert lines[2:] == [[s.sum, s.worst, *s.worst_position, s.windows_x * s.windows_y] for s in wm.ssim(original, copies, ctx)]
    filters = [wm.Filter.blur(1.5), wm.Filter.median(), wm.Filter.unsharp()]
    expected = (wm.collude(copies, [("median", [0, 1]), ("mosaic", [1])], ctx) + [f for per in wm.jpeg(copies, (75, 10), ctx) for f in per]
                + [f for per in wm.filter(copies, filters, ctx) for f in per])
    got = np.fromfile(p("frames.u8"), np.uint8).reshape(-1, h, w, 3)
    assert len(expected) == len(got) == 12
    for i, e in enumerate(expected):
        assert np.array_equal(got[i], e), i
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[2], got[3]) and not np.array_equal(got[6], got[7])
    ctx.close()
