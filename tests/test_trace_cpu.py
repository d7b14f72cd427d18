"""Tracing (one original, many suspects, many stored marks per call): the parts that need no GPU -- the C ABI symbols and
their citations, the ctypes bindings, the Python and CLI surfaces, and the C++ wrapper compiling against the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd.storage import Configuration, DescribedWatermark, Version1Storage

NAMES = ("ssw_fingerprint_trace", "ssw_fingerprint_trace_rgb8", "ssw_fingerprint_trace_host_rgb8", "ssw_reader_trace_host_rgb8")
LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")


def test_symbols_declared_exported_bound_and_cited():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        decl = text.index(n + "(")
        assert hasattr(lib, n), n
        assert n in L.SIGNATURES, n
        comment = text.rfind("/*", 0, decl)
        assert re.search(r"algorithm\.rs:\d+", text[comment:decl]), n
    dev = L.SIGNATURES["ssw_fingerprint_trace"][1]
    assert len(dev) == 16 and dev[10] is C.c_float and dev[4:8] == [C.c_size_t] * 4          # n_suspects, w, h, k ... threshold
    assert L.SIGNATURES["ssw_fingerprint_trace_rgb8"][1][4:11] == dev[4:11]
    assert len(L.SIGNATURES["ssw_fingerprint_trace_host_rgb8"][1]) == 16 and len(L.SIGNATURES["ssw_reader_trace_host_rgb8"][1]) == 12
    assert L.TRACE_NONE == 0xFFFFFFFF


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    doc = text[text.index("tracing: ONE original"):text.index("ssw_fingerprint_trace(")]
    for phrase in ("bit-identical to ssw_batch_extract", "ssw_similarity_matrix", "lowest index on ties", "0xFFFFFFFF", "ssw_similarity_batch",
                   "NaN never exceeds", "SSW_ERR_K_TOO_LARGE", "SSW_ERR_UNSUPPORTED", "stream capture"):
        assert phrase in doc, phrase


def test_python_surface():
    import spread_spectrum_watermarking_amd as wm
    assert callable(api.Reader.trace) and callable(wm.trace_many) and wm.TraceResult.NONE == 0xFFFFFFFF
    m, k = api._trace_marks([np.zeros(5), api.MarkBuf(np.ones(5))], None)
    assert m.shape == (2, 5) and m.dtype == np.float32 and k == 5
    m, k = api._trace_marks(None, 7)
    assert m.shape == (0, 7) and k == 7
    with pytest.raises(ValueError):
        api._trace_marks([np.zeros(5), np.zeros(4)], None)
    with pytest.raises(ValueError):
        api._trace_marks(None, None)
    r = api.TraceResult.empty(3, 2, 5)
    assert r.extracted.shape == (3, 5) and r.sims.shape == (3, 2) and list(r.best) == [0xFFFFFFFF] * 3 and np.all(np.isnan(r.best_sim))
    r.sims[:] = [[7.0, np.nan], [1.0, 6.5], [np.nan, np.nan]]
    r.threshold = 6.0
    assert [r.matches(s) for s in range(3)] == [[0], [1], []]                  # NaN never exceeds (algorithm.rs:677)
    assert r._args(np.zeros((0, 5), np.float32), 6.0)[:2] == (None, 0)         # extraction only: no similarity output either
    assert all(a is None for a in r._args(np.zeros((0, 5), np.float32), 6.0)[4:])


def test_trace_parser_surface():
    p = cli.build_parser()
    a = p.parse_args(["trace", "cat.jpg", "--suspects", "a.png", "b.png", "--marks", "x_fp.json", "y.json"])
    assert (a.command, a.base, a.suspects, a.marks, a.similarity_exceed) == ("trace", "cat.jpg", ["a.png", "b.png"], ["x_fp.json", "y.json"], 6.0)
    a = p.parse_args(["trace", "--similarity-exceed", "4.5", "cat.jpg", "--suspects", "a.png", "--marks", "x.json"])
    assert a.similarity_exceed == 4.5
    for bad in (["trace", "cat.jpg", "--marks", "x.json"], ["trace", "cat.jpg", "--suspects", "a.png"], ["trace", "--suspects", "a.png", "--marks", "x.json"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    # the existing subcommands parse as before
    t = p.parse_args(["test", "b.png", "w.png", "m.json"])
    assert (t.command, t.base, t.watermarked, t.watermark_files, t.similarity_exceed) == ("test", "b.png", "w.png", ["m.json"], 6.0)


def test_stored_marks_group_like_the_test_command(tmp_path):
    """`test` keys its extractions by (config, length) (main.rs:369-371) and accepts a file whose marks differ in length: so does
    `trace` -- one call per group, every mark in exactly one group, file order kept inside a group."""
    c1, c2 = Configuration(), Configuration(alpha=0.2, method="Option1", ordering="Legacy")
    mk = lambda n, d: DescribedWatermark(np.arange(n, dtype=np.float32), d)
    a, b = tmp_path / "a.json", tmp_path / "b.json"
    a.write_text(Version1Storage(c1, [mk(8, "a0"), mk(5, "a1"), mk(8, "a2")]).to_json())          # mixed lengths in one file
    b.write_text(Version1Storage(c2, [mk(8, "b0")]).to_json())
    c = tmp_path / "c.json"
    c.write_text(Version1Storage(c1, [mk(8, "c0")]).to_json())
    stored = [(str(p), Version1Storage.load(str(p))) for p in (a, b, c)]
    groups = cli.group_stored_marks(stored)
    assert list(groups) == [(c1, 8), (c1, 5), (c2, 8)]
    assert [(os.path.basename(p), w.description) for p, w in groups[(c1, 8)]] == [("a.json", "a0"), ("a.json", "a2"), ("c.json", "c0")]
    assert [w.description for _, w in groups[(c1, 5)]] == ["a1"] and [w.description for _, w in groups[(c2, 8)]] == ["b0"]


CPP = r"""
#include "ssw.hpp"
int main() {
    wm::Context ctx(0);
    wm::ImageRgb8 img(8, 8), s0(8, 8), s1(8, 8);
    wm::Reader base = wm::Reader::base(ctx, img);
    wm::MarkBuf a = wm::MarkBuf::generate_normal(4), b = wm::MarkBuf::generate_normal(4);
    wm::TraceResult r = base.trace({&s0, &s1}, {&a, &b}, 6.0f);
    if (r.best[0] == wm::TraceResult::none) return 2;
    return (int)(r.extracted.size() + r.sims.size() + r.best.size() + r.best_sim.size() + r.n_exceed.size()) - 10;
}
"""


def test_cpp_reader_trace_compiles_and_links(tmp_path):
    src = tmp_path / "trace.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "trace")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert os.path.exists(exe)
