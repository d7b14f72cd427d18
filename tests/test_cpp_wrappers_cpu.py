"""The whole of include/ssw.hpp, run on the CPU: tests/cpp/wrappers_stub_test.cpp calls every public function, constructor and
method of namespace wm against tests/cpp/ssw_stub.cpp, a contract stand-in for libssw_hip.so that is linked INSTEAD of the
library (no HIP, no GPU; the C++ counterpart of tests/fake_ssw.py).  The stub reads every byte a call's contract reads and
writes patterns that encode the position, so a transposed slice, a swapped argument or an undersized std::vector shows; then
every flow runs again with its n-th library call failing, for every n, and must throw that status and leave nothing alive.
A stand-alone program under ASan + UBSan: nothing is preloaded and nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_sanitizers import _runtime

CPP = os.path.join(ROOT, "tests", "cpp")
HEADER = os.path.join(ROOT, "include", "ssw.hpp")
DRIVER = os.path.join(CPP, "wrappers_stub_test.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """Stub and driver, compiled once per module without and (where the image has libasan) with the sanitizers, side by side."""
    d = tmp_path_factory.mktemp("wrappers_stub")
    builds = {"plain": [], "sanitized": SANITIZE} if _runtime("libasan.so") else {"plain": []}
    running = {name: subprocess.Popen(["g++", *FLAGS, *extra, "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "ssw_stub.cpp"), DRIVER,
                                       "-o", str(d / name)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
               for name, extra in builds.items()}
    exes = {"sanitized": None}
    for name, proc in running.items():
        _, err = proc.communicate()
        assert proc.returncode == 0 and err == "", err
        exes[name] = str(d / name)
    return exes


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    report = r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error:" not in report and "AddressSanitizer" not in report, report
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", report
    return r.stdout.splitlines()


def check_sweep(lines):
    """One line per flow with the number of library calls the failure sweep visited, and their sum."""
    sweeps = [line.split() for line in lines if line.startswith("sweep ")]
    assert len(sweeps) == 14 and all(int(s[2]) > 0 for s in sweeps), lines
    assert lines[-2] == f"calls swept {sum(int(s[2]) for s in sweeps)}"


def test_every_wrapper_against_the_stub_under_asan_ubsan(programs):
    if programs["sanitized"] is None:
        pytest.skip("no libasan in this image")
    check_sweep(run(programs["sanitized"]))


def test_every_wrapper_against_the_stub(programs):
    check_sweep(run(programs["plain"]))


# ---- what must and must not compile ------------------------------------------------------------------------------------------
def syntax_only(tmp_path, name, body):
    src = tmp_path / f"{name}.cpp"
    src.write_text('#include "ssw.hpp"\nvoid f(wm::Context& ctx) { ' + body + " }\n")
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)


def test_what_compiles_and_what_does_not(tmp_path):
    good = {"reader_base_16": "wm::Reader r = wm::Reader::base(ctx, wm::ImageRgb16(4, 4)); (void)r;",
            "reader_derived_16": "wm::ReaderDerived d(ctx, wm::ImageRgb16(4, 4)); (void)d;",
            "suspect_rgba": "wm::ImageRgba8 a(4, 4); wm::Suspect s(a); (void)wm::locate(ctx, wm::ImageRgb8(8, 8), {s});"}
    bad = {"writer_copy": "wm::Writer w(ctx, wm::ImageRgb8(4, 4)); wm::Writer c(w);",
           "catalogue_copy": "wm::Catalogue a(ctx); wm::Catalogue c(a);"}
    for name, body in good.items():
        done = syntax_only(tmp_path, name, body)
        assert done.returncode == 0, done.stderr
    for name, body in bad.items():
        done = syntax_only(tmp_path, name, body)
        assert done.returncode != 0 and "deleted" in done.stderr, (name, done.stderr)


# ---- the driver covers the whole of namespace wm -------------------------------------------------------------------------------
def public_names(header_text):
    """The public functions, methods and constructors of namespace wm, as `name` or `Class::name`: the `inline` functions at
    the left margin, and inside every class or struct that starts at the left margin the declarations indented by four
    spaces in a public section.  namespace detail, destructors, operators and deleted members are not wrappers."""
    text = re.sub(r"//[^\n]*", "", header_text)
    text = re.sub(r"namespace detail \{.*?\n\}  ", "", text, flags=re.S)
    names, cls, public = set(), None, True
    for line in text.splitlines():
        m = re.match(r"(class|struct) (\w+)[^;]*\{", line)
        if m and not line.rstrip().endswith("};"):
            cls, public = m.group(2), m.group(1) == "struct"
            continue
        m = re.match(r"(class|struct) (\w+)[^;]*\{.*\};\s*$", line)
        if m:                                                     # a one-line struct: its members are data
            continue
        if line.startswith("};"):
            cls = None
        elif line.startswith("public:") or line.startswith("private:"):
            public = line.startswith("public:")
        elif cls is None:
            m = re.match(r"inline [^(=]*?([\w:]+)\(", line)
            if m and "::" not in m.group(1):                      # Class::name: a member defined outside its class
                names.add(m.group(1))
        elif public and "= delete" not in line:
            m = re.match(r"    (?:template <class \w+> )?(?:static |explicit )*(?:[\w:<>,\*&]+ )*?(~?\w+)\(", line)
            if m and not m.group(1).startswith("~") and m.group(1) != "operator":
                names.add(f"{cls}::{m.group(1)}")
    return names


def test_the_driver_covers_the_whole_of_namespace_wm():
    names = public_names(open(HEADER).read())
    # the extraction itself: it sees what this header is known to hold, and nothing private
    assert {"Reader::base", "Reader::trace", "Writer::mark_copies_rgb8", "Catalogue::match", "locate_scaled", "extract_many", "check",
            "Context::Context", "PinnedBuffer::data", "Placement::whole_frame", "Suspect::Suspect", "Scale::by", "Rotate::job",
            "MarkBuf::from", "ReaderDerived::ReaderDerived", "Tester::similarity", "Error::status", "WriteConfig::c"} <= names
    assert len(names) >= 85 and "Writer::copies" not in names and not any(n.startswith("DeviceFrames") or n.startswith("Free") for n in names)
    driver = open(DRIVER).read()
    table = re.search(r"// Coverage:.*?// End of coverage", driver, re.S).group(0)
    listed = set(re.findall(r"[\w:]+", table))
    code = re.sub(r"//[^\n]*", "", driver)
    for name in sorted(names):
        assert name in listed, f"{name} is not in the coverage table of wrappers_stub_test.cpp"
        cls, _, fn = name.rpartition("::")
        used = re.search(rf"\bwm::{cls}\b", code) if cls == fn else re.search(rf"(?:\.|::){fn}\(", code)
        assert used, f"{name} is not called by wrappers_stub_test.cpp"
    # a wrapper added without a flow fails this
    added = public_names(open(HEADER).read().replace("class Tester {", "inline int brand_new(Context& ctx) { return 0; }\nclass Tester {"))
    assert added - names == {"brand_new"}
