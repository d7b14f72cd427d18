"""The forensic wrappers of include/ssw.hpp, run against the real library: tests/cpp/forensic_wrappers_test.cpp goes through
Writer::mark_copies(_rgb8), both Reader::trace overloads, locate, locate_scaled, signature, Catalogue, mark_many, extract_many, the
16-bit Writer / Reader::base / ReaderDerived and PinnedBuffer on one small scenario from the committed cat, and this module computes
the same through spread_spectrum_watermarking_amd.api on one context.  Both routes end in the same library calls, so every
comparison is np.array_equal or equality of float32 bits (NaN included); there is no tolerance.  The program is built and run once
per module; each test reads its part of the output."""
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, u8_to_f32
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api

pytestmark = pytest.mark.gpu

LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
W, H, K, SK = 192, 128, 64, 32
NONE = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Scenario:
    """The inputs, what the Python route makes of them, and what the C++ program wrote."""


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    from oracle import oracle as O
    t0 = time.time()
    d = tmp_path_factory.mktemp("forensic")
    exe = str(d / "forensic_wrappers_test")
    done = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "forensic_wrappers_test.cpp"), "-o", exe,
                           "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    s = Scenario()
    s.ctx = ctx = api.Context(0)
    cat = np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))["cat"]
    s.B = B = np.ascontiguousarray(cat[100:228, 200:392])
    assert B.shape == (H, W, 3)
    s.marks = marks = np.random.default_rng(7).standard_normal((4, K)).astype(np.float32)
    s.B32 = u8_to_f32(B)
    # the Python route, in the program's order
    writer = api.Writer(B, None, ctx)
    s.copies = copies = writer.mark_copies_rgb8(marks)
    s.again = writer.mark_rgb8([marks[0]])
    s.copies32 = api.Writer(s.B32, None, ctx).mark_copies(marks)
    s.base = api.Reader.base(B, None, ctx)
    s.plain = s.base.trace(list(copies) + [B], marks)
    s.small = api.resample([copies[2]], (96, 64), "bicubic", ctx)[0]
    s.rect = np.ascontiguousarray(B[24:88, 40:120])
    cut = np.zeros((64, 80, 4), np.uint8)
    cut[:, :, :3] = copies[3][24:88, 40:120]
    cut[4:-4, 4:-4, 3] = 255
    s.cut = cut
    s.suspects = [copies[1], s.small, cut]
    s.placements = [api.Placement(0, 0, W, H), api.Placement(0, 0, W, H), api.Placement(40, 24)]
    s.restored = api.trace_many(B, s.suspects, marks, ctx=ctx, placements=s.placements)
    s.restored_handle = s.base.trace(s.suspects, marks, placements=s.placements, base=B)
    s.cut60 = api.resample([np.ascontiguousarray(copies[3][24:88, 40:120])], (60, 48), "bicubic", ctx)[0]
    s.noise = np.random.default_rng(8).integers(0, 256, (35, 33, 3), dtype=np.uint8)
    s.rolled, s.flipped = np.ascontiguousarray(np.roll(B, 40, axis=1)), np.ascontiguousarray(B[::-1])
    s.subs = [np.ascontiguousarray(B[y:y + 64, x:x + 96]) for y, x in ((0, 0), (32, 48), (64, 96))]
    s.short = marks[:3, :SK]
    s.many = api.mark_many(s.subs, s.short, None, ctx)
    s.B16 = B.astype(np.uint16) * 257
    s.marked16 = api.Writer(s.B16, None, ctx).mark([marks[0]])
    s.marked16_u16 = O.f32_to_u16(s.marked16)
    files = {"B.u8": B, "B32.f32": s.B32, "marks.f32": marks, "small.u8": s.small, "cut_rgba.u8": cut, "rect.u8": s.rect, "cut60.u8": s.cut60,
             "noise.u8": s.noise, "rolled.u8": s.rolled, "flipped.u8": s.flipped, "sub0.u8": s.subs[0], "sub1.u8": s.subs[1], "sub2.u8": s.subs[2],
             "marked16.u16": s.marked16_u16}
    ind, outd = d / "in", d / "out"
    ind.mkdir(); outd.mkdir()
    for name, a in files.items():
        np.ascontiguousarray(a).tofile(ind / name)
    run = subprocess.run([exe, str(ind), str(outd)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.splitlines()[-1] == "ok", run.stdout[-2000:] + run.stderr[-2000:]
    s.lines = [line.split() for line in run.stdout.splitlines()]
    s.out = lambda name, dtype, shape=-1: np.fromfile(outd / name, dtype).reshape(shape)
    print(f"forensic scenario: built, computed and run in {time.time() - t0:.1f} s")
    yield s
    ctx.close()


def records(sc, what):
    return [line[1:] for line in sc.lines if line[0] == what]


def same_trace(sc, prefix, ref, n, nm, k):
    assert np.array_equal(bits(sc.out(f"{prefix}_ext.f32", np.float32, (n, k))), bits(ref.extracted))
    assert np.array_equal(bits(sc.out(f"{prefix}_sims.f32", np.float32, (n, nm))), bits(ref.sims))
    assert np.array_equal(sc.out(f"{prefix}_best.u32", np.uint32, n), ref.best)
    assert np.array_equal(bits(sc.out(f"{prefix}_best_sim.f32", np.float32, n)), bits(ref.best_sim))
    assert np.array_equal(sc.out(f"{prefix}_n_exceed.u32", np.uint32, n), ref.n_exceed)


def test_fingerprinting_and_the_writer_stays_usable(sc):
    copies = sc.out("copies8.u8", np.uint8, (4, H, W, 3))
    assert np.array_equal(copies, sc.copies)
    assert all(not np.array_equal(copies[i], copies[j]) for i in range(4) for j in range(i))
    assert np.array_equal(bits(sc.out("copies32.f32", np.float32, (4, H, W, 3))), bits(sc.copies32))
    again = sc.out("again8.u8", np.uint8, (H, W, 3))
    assert np.array_equal(again, sc.again) and np.array_equal(again, copies[0])


def test_plain_trace_every_field(sc):
    same_trace(sc, "plain", sc.plain, 5, 4, K)
    best, best_sim = sc.out("plain_best.u32", np.uint32), sc.out("plain_best_sim.f32", np.float32)
    assert list(best[:4]) == [0, 1, 2, 3]
    # the original itself extracts zeros: no winner, NaN, nothing above the threshold
    assert best[4] == NONE and np.isnan(best_sim[4]) and sc.out("plain_n_exceed.u32", np.uint32)[4] == 0
    assert np.all(np.isnan(sc.out("plain_sims.f32", np.float32, (5, 4))[4]))


def test_restoring_trace_of_a_copy_a_scaled_copy_and_an_rgba_cut_out(sc):
    same_trace(sc, "restored", sc.restored, 3, 4, K)
    same_trace(sc, "restored", sc.restored_handle, 3, 4, K)
    assert list(sc.out("restored_best.u32", np.uint32)) == [1, 2, 3]


def located(rec):
    return [int(v) for v in rec[:5]] + [float.fromhex(rec[5])]


def test_locate_at_the_own_and_at_a_given_size(sc):
    (own,), (sized,) = records(sc, "locate_own"), records(sc, "locate_sized")
    assert located(own) == [40, 24, 80, 64, 0, 0.0]
    ref = api.locate(sc.B, [sc.cut60], [(80, 64)], sc.ctx)[0]
    assert located(sized) == [ref.placement.x, ref.placement.y, 80, 64, ref.sad, ref.mean_abs_diff]


def test_locate_scaled_over_a_ladder_of_five_rungs(sc):
    (found,) = records(sc, "locate_scaled")
    ref = api.locate(sc.B, [sc.cut60], [api.Locate(widths=(64, 96))], sc.ctx)[0]
    assert located(found) == [ref.placement.x, ref.placement.y, ref.placement.w, ref.placement.h, ref.sad, ref.mean_abs_diff]
    assert 64 <= ref.placement.w <= 96 and ref.placement.h == max(1, (2 * 48 * ref.placement.w + 60) // (2 * 60))


def test_signatures_of_three_sizes(sc):
    ref = api.signature([sc.B, sc.cut, sc.noise], sc.ctx)
    assert np.array_equal(sc.out("sigs.u8", np.uint8, (3, 1024)), ref)


def test_catalogue_top_1_top_8_and_after_another_add(sc):
    cat = api.Catalogue(sc.ctx)
    cat.add_many(["B", "rolled", "flipped"], [sc.B, sc.rolled, sc.flipped])
    queries = api.signature([sc.copies[1], sc.rolled], sc.ctx)

    def same(what, top):
        idx, dist = cat.match_signatures(queries, top)
        got = {(int(r[0]), int(r[1])): (int(r[2]), int(r[3])) for r in records(sc, what)}
        assert got == {(s, t): (int(idx[s][t]), int(dist[s][t])) for s in range(2) for t in range(top)}
        return idx, dist

    idx, _ = same("match1", 1)
    assert [int(idx[0][0]), int(idx[1][0])] == [0, 1]
    idx, dist = same("match8", 8)
    assert np.all(idx[:, 3:] == NONE) and np.all(dist[:, 3:] == NONE) and np.all(idx[:, :3] != NONE)
    cat.add("small", sc.small)
    idx, dist = same("match8_four", 8)
    assert np.all(idx[:, 4:] == NONE) and np.all(dist[:, 4:] == NONE) and np.all(idx[:, :4] != NONE)
    assert records(sc, "catalogue") == [["4", "small"]]


def test_mark_many_and_extract_many_with_and_without_marks(sc):
    marked = sc.out("many8.u8", np.uint8, (3, 64, 96, 3))
    assert all(np.array_equal(marked[i], sc.many[i]) for i in range(3))
    ext, sims = api.extract_many(sc.subs, sc.many, SK, sc.short, None, sc.ctx)
    ext_only, no_sims = api.extract_many(sc.subs, sc.many, SK, None, None, sc.ctx)
    assert np.array_equal(bits(sc.out("many_ext.f32", np.float32, (3, SK))), bits(ext))
    assert np.array_equal(bits(sc.out("many_sims.f32", np.float32, 3)), bits(sims))
    assert np.array_equal(bits(sc.out("many_ext_only.f32", np.float32, (3, SK))), bits(ext_only)) and no_sims is None
    assert records(sc, "many") == [["3", "3", "3", "0"]]


def test_sixteen_bit_images_are_marked_and_read(sc):
    assert np.array_equal(bits(sc.out("marked16.f32", np.float32, (H, W, 3))), bits(sc.marked16))
    ref = api.Reader.base(sc.B16, None, sc.ctx).extract(api.Reader.derived(sc.marked16_u16, sc.ctx), K)
    got = sc.out("ext16.f32", np.float32, K)
    assert np.array_equal(bits(got), bits(ref))


def test_pinned_buffer_and_transfer_stats(sc):
    assert records(sc, "pinned") == [[str(1 << 20), "0"]]
    assert records(sc, "transfer_stats") == [[str(len(L.TRANSFER_STATS))]] and len(L.TRANSFER_STATS) == 6      # SSW_TRANSFER_STAT_COUNT


def test_error_paths_of_the_real_library(sc):
    assert dict((name, int(status)) for name, status in records(sc, "error")) == {
        "match_top9": L.SSW_ERR_BAD_ARG, "trace_other_size": L.SSW_ERR_BAD_DIMS, "result_twice": L.SSW_ERR_CONSUMED,
        "locate_too_large": L.SSW_ERR_BAD_ARG, "locate_scaled_below_32": L.SSW_ERR_BAD_ARG}
