"""Fingerprinting (many individually marked copies of one image per call): the parts that need no GPU -- the C ABI
symbols and their citations, the ctypes bindings, the CLI surface, and the C++ wrapper compiling against the library."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli

NAMES = ("ssw_fingerprint_embed", "ssw_fingerprint_embed_rgb8", "ssw_writer_mark_copies", "ssw_writer_mark_copies_rgb8")
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
    assert L.SIGNATURES["ssw_fingerprint_embed"][1][6:8] == [C.c_size_t, C.c_size_t]       # n_copies, k
    assert len(L.SIGNATURES["ssw_writer_mark_copies"][1]) == 5


def test_writer_surface():
    assert callable(api.Writer.mark_copies) and callable(api.Writer.mark_copies_rgb8)


def test_fingerprint_parser_surface():
    p = cli.build_parser()
    a = p.parse_args(["fingerprint", "cat.jpg", "--copies", "5", "-d", "buyer"])
    assert (a.command, a.file, a.copies, a.description) == ("fingerprint", "cat.jpg", 5, "buyer")
    assert (a.length, a.ordering, a.alpha, a.method) == (1000, "energy", 0.1, "option2")
    a = p.parse_args(["fingerprint", "x.png", "--copies", "2", "--length", "64", "--ordering", "legacy", "--alpha", "0.3",
                      "--method", "option3"])
    assert (a.length, a.ordering, a.alpha, a.method) == (64, "legacy", 0.3, "option3")
    with pytest.raises(SystemExit):
        p.parse_args(["fingerprint", "x.png"])                  # --copies is required


def test_fingerprint_output_names():
    imgs, js = cli.fingerprint_paths("/tmp/cat.jpg", 5)
    assert imgs == [f"/tmp/cat_fp{i}.png" for i in range(5)] and js == "/tmp/cat_fp.json"
    imgs, _ = cli.fingerprint_paths("/tmp/cat.jpg", 12)
    assert imgs[0] == "/tmp/cat_fp00.png" and imgs[-1] == "/tmp/cat_fp11.png"


def test_fingerprint_refuses_to_overwrite(tmp_path):
    src = tmp_path / "pic.png"
    src.write_bytes(b"")
    (tmp_path / "pic_fp1.png").write_bytes(b"")
    args = cli.build_parser().parse_args(["fingerprint", str(src), "--copies", "3"])
    with pytest.raises(SystemExit, match="already exists"):
        cli.cmd_fingerprint(args)


CPP = r"""
#include "ssw.hpp"
int main() {
    wm::Context ctx(0);
    wm::ImageRgb8 img(8, 8);
    wm::Writer w(ctx, img);
    wm::MarkBuf a = wm::MarkBuf::generate_normal(4), b = wm::MarkBuf::generate_normal(4);
    std::vector<wm::ImageRgb32F> f = w.mark_copies({&a, &b});
    std::vector<wm::ImageRgb8> u = w.mark_copies_rgb8({&a, &b});
    return (int)(f.size() + u.size()) - 4;
}
"""


def test_cpp_mark_copies_compiles_and_links(tmp_path):
    src = tmp_path / "fp.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "fp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert os.path.exists(exe)
