"""Fingerprinting on the GPU: ssw_fingerprint_embed(_rgb8) and Writer.mark_copies(_rgb8) against the CPU oracle's
Writer::new(img).mark(&[&mark_i]) and against ssw_batch_embed on replicated frames, with the project's f64 parity bars:
marked f32 frames max |d| <= 2e-7 and >= 99.99 % bit-identical, 8-bit frames >= 99.99 % equal and <= 1 LSB."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_util as G
import spread_spectrum_watermarking_amd as wm
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from gpu_util import assert_f32_bars, assert_u8_bars, fingerprint

pytestmark = pytest.mark.gpu

E, EO, LG = L.ORDER_ENERGY, L.ORDER_ENERGY_ORTHOGONAL, L.ORDER_LEGACY
O1, O2, O3 = L.OPTION1, L.OPTION2, L.OPTION3
OPTION3_MARKED_IDENTICAL = 0.82          # tests/test_config_matrix_gpu.py: device expf vs libm, against the oracle only
# marked frames against the oracle at 4K: the bar ssw_batch_embed's own 4K parity test holds (tests/test_gpu_parity.py, > 0.999;
# measured 0.99985 for copy 0 here); against ssw_batch_embed the full 0.9999
ORACLE_4K_IDENTICAL = 0.999


def marks_for(n, k, seed):
    return np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)


def cat_u8():
    return np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))["cat"]


# 1. the cat, f32 and u8, 4 copies, k = 1000 ------------------------------------------------------------------------------
def test_cat_f32_against_oracle_and_batch():
    rgb = O.u8_to_f32(cat_u8())
    marks = marks_for(4, 1000, 1)
    copies, idx = fingerprint(rgb, marks, want_idx=True)
    coef = O.dct2d(O.rgb_to_yiq(rgb)[0])
    assert np.array_equal(idx, O.indices(coef, k=1000))
    batch = G.batch_embed(np.repeat(rgb[None], 4, 0), marks, want_idx=True)
    assert np.array_equal(batch["idx"][0], idx)
    for i in range(4):
        assert_f32_bars(copies[i], O.embed_frame(rgb, marks[i]), what=f"oracle {i}")
        assert_f32_bars(copies[i], batch["rgb"][i], what=f"batch {i}")


def test_cat_u8_against_oracle_and_batch():
    img = cat_u8()
    marks = marks_for(4, 1000, 2)
    copies = fingerprint(img, marks)
    batch = G.batch_embed_rgb8(np.repeat(img[None], 4, 0), marks)
    for i in range(4):
        assert_u8_bars(copies[i], O.f32_to_u8(O.embed_frame(O.u8_to_f32(img), marks[i])), what=f"oracle {i}")
        assert_u8_bars(copies[i], batch[i], what=f"batch {i}")


# 2. small shapes x every ordering x method ------------------------------------------------------------------------------
SHAPES = [(320, 180), (180, 320), (256, 256), (333, 197)]
CONFIGS = [(o, m) for o in (E, EO, LG) for m in (O1, O2, O3)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("conf", CONFIGS, ids=lambda c: f"o{c[0]}-m{c[1]}")
def test_small_shapes_every_configuration(shape, conf):
    w, h = shape
    ordering, method = conf
    rgb = O.synth_frame(3, w + h, w, h)
    marks = marks_for(3, 300, w * 7 + h + ordering * 3 + method)
    cfg = G.default_config(L.PRECISION_F64, ordering, method, 0.1)
    copies = fingerprint(rgb, marks, cfg)
    batch = G.batch_embed(np.repeat(rgb[None], 3, 0), marks, cfg)["rgb"]
    ident = OPTION3_MARKED_IDENTICAL if method == O3 else 0.9999
    for i in range(3):
        assert_f32_bars(copies[i], O.embed_frame(rgb, marks[i], ordering=ordering, method=method, alpha=0.1), ident, f"oracle {i}")
        assert_f32_bars(copies[i], batch[i], what=f"batch {i}")


# 3. independence and determinism ------------------------------------------------------------------------------------------
def test_copies_independent_of_company_and_position():
    rgb = O.synth_frame(5, 0, 320, 180)
    marks = marks_for(8, 500, 5)
    a, b = fingerprint(rgb, marks), fingerprint(rgb, marks)
    assert np.array_equal(a, b)
    for i in (0, 3, 7):
        assert np.array_equal(fingerprint(rgb, marks[i:i + 1])[0], a[i])
    perm = np.roll(np.arange(8), 3)
    c = fingerprint(rgb, marks[perm])
    for j, i in enumerate(perm):
        assert np.array_equal(c[j], a[i])


# 4. a zero mark is the unmarked Writer::result -----------------------------------------------------------------------------
def test_zero_mark_is_the_unmarked_result():
    rgb = O.synth_frame(6, 1, 256, 144)
    marks = np.zeros((2, 400), np.float32)
    marks[1] = marks_for(1, 400, 6)[0]
    copies = fingerprint(rgb, marks)
    plain = wm.Writer(rgb, ctx=G.ctx()).result()
    assert_f32_bars(copies[0], plain, what="zero mark")
    assert not np.array_equal(copies[1], copies[0])


# 5. 4K synth frame, 8 copies ----------------------------------------------------------------------------------------------
def test_4k_copies_and_tracing():
    w, h, k, n = 3840, 2160, 1000, 8
    rgb = O.synth_frame(7, 0, w, h)
    marks = marks_for(n, k, 7)
    copies = fingerprint(rgb, marks)
    batch = G.batch_embed(np.repeat(rgb[None], n, 0), marks)["rgb"]
    for i in range(n):
        assert_f32_bars(copies[i], batch[i], what=f"batch {i}")
    for i in (0, n - 1):
        assert_f32_bars(copies[i], O.embed_frame(rgb, marks[i]), ORACLE_4K_IDENTICAL, what=f"oracle {i}")
    ext, _ = G.batch_extract(np.repeat(rgb[None], n, 0), copies, k)
    sims = G.similarity_matrix(ext, marks)
    off = sims[~np.eye(n, dtype=bool)]
    assert np.all(np.diag(sims) > 6.0) and np.all(off < 6.0), sims


# 6. larger frames against ssw_batch_embed --------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,k,n", [(7680, 4320, 10000, 2), (1080, 1920, 1000, 4)], ids=["8k-k10000", "portrait-1080x1920"])
def test_large_frames_against_batch(w, h, k, n):
    rgb = O.synth_frame(8, w, w, h)
    marks = marks_for(n, k, 8)
    copies = fingerprint(rgb, marks)
    for i in range(n):
        assert_f32_bars(copies[i], G.batch_embed(rgb[None], marks[i:i + 1])["rgb"][0], what=f"batch {i}")


# 7. the handle form ---------------------------------------------------------------------------------------------------------
def test_handles_match_device_form_and_leave_the_writer_alone():
    img = cat_u8()[:200, :300].copy()
    rgb = O.u8_to_f32(img)
    marks = marks_for(3, 700, 9)
    w = wm.Writer(rgb, ctx=G.ctx())
    assert np.array_equal(w.mark_copies(marks), fingerprint(rgb, marks))
    w8 = wm.Writer(img, ctx=G.ctx())
    assert np.array_equal(w8.mark_copies_rgb8(list(marks)), fingerprint(img, marks))
    # the writers are untouched: mark() afterwards equals a fresh writer's
    m = marks_for(1, 700, 10)[0]
    assert np.array_equal(w.mark([m]), wm.Writer(rgb, ctx=G.ctx()).mark([m]))
    assert np.array_equal(w8.mark_rgb8([m]), wm.Writer(img, ctx=G.ctx()).mark_rgb8([m]))


def test_handles_after_an_embed():
    rgb = O.synth_frame(11, 0, 320, 180)
    m0 = marks_for(1, 300, 11)[0]
    marks = marks_for(3, 500, 12)
    w = wm.Writer(rgb, ctx=G.ctx())
    w.embed([m0])
    copies = w.mark_copies(marks)
    for i in range(3):
        ref = wm.Writer(rgb, ctx=G.ctx())
        ref.embed([m0])
        ref.embed([marks[i]])
        assert_f32_bars(copies[i], ref.result(), what=f"copy {i}")


def test_error_statuses():
    lib, ctx = G.lib(), G.ctx()
    rgb = O.synth_frame(12, 0, 64, 48)
    marks = marks_for(2, 50, 13)
    with pytest.raises(ValueError):
        wm.Writer(rgb, ctx=ctx).mark_copies([marks[0], marks[1][:40]])
    d, dm, out = ctx.to_device(rgb), ctx.to_device(marks), ctx.alloc(2 * rgb.nbytes)
    cfg = G.default_config()
    for bad in (L.Config(L.ORDER_CUSTOM, O2, 0.1, L.PRECISION_F64), L.Config(E, L.METHOD_CUSTOM, 0.1, L.PRECISION_F64),
                G.default_config(L.PRECISION_F32)):
        assert lib.ssw_fingerprint_embed(ctx.handle, C.byref(bad), d.ptr, 64, 48, dm.ptr, 2, 50, out.ptr, None) == L.SSW_ERR_UNSUPPORTED
    assert lib.ssw_fingerprint_embed(ctx.handle, C.byref(cfg), None, 64, 48, dm.ptr, 2, 50, out.ptr, None) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_fingerprint_embed(ctx.handle, C.byref(cfg), d.ptr, 64, 48, None, 2, 50, out.ptr, None) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_fingerprint_embed(ctx.handle, C.byref(cfg), d.ptr, 64, 48, dm.ptr, 2, 50, None, None) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_fingerprint_embed(ctx.handle, None, d.ptr, 64, 48, dm.ptr, 2, 50, out.ptr, None) == L.SSW_ERR_BAD_ARG
    zero_fp = lib.ssw_fingerprint_embed(ctx.handle, C.byref(cfg), d.ptr, 64, 48, dm.ptr, 0, 50, out.ptr, None)
    zero_batch = lib.ssw_batch_embed(ctx.handle, C.byref(cfg), d.ptr, 0, 64, 48, dm.ptr, 50, out.ptr, None, None)
    assert zero_fp == zero_batch
    # a mark longer than w*h - 1 is cut like the batch path
    long_marks = marks_for(1, 64 * 48 + 10, 14)
    assert_f32_bars(fingerprint(rgb, long_marks)[0], G.batch_embed(rgb[None], long_marks)["rgb"][0], what="cut")
    for b in (d, dm, out):
        b.free()
    w = wm.Writer(rgb, ctx=ctx)
    w.result()
    host = np.empty((2, 48, 64, 3), np.float32)
    assert lib.ssw_writer_mark_copies(w._h, marks.ctypes.data, 2, 50, host.ctypes.data) == L.SSW_ERR_CONSUMED
    w2 = wm.Writer(rgb, ctx=ctx)
    assert lib.ssw_writer_mark_copies(w2._h, None, 2, 50, host.ctypes.data) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_writer_mark_copies(None, marks.ctypes.data, 2, 50, host.ctypes.data) == L.SSW_ERR_BAD_ARG
    w3 = wm.Writer(rgb, wm.WriteConfig(precision=wm.Precision.F32), ctx=ctx)
    assert lib.ssw_writer_mark_copies(w3._h, marks.ctypes.data, 2, 50, host.ctypes.data) == L.SSW_ERR_UNSUPPORTED


# 8. the CLI: fingerprint, then `test` names the leaked copy ---------------------------------------------------------------
def test_cli_fingerprint_then_test_names_the_copy(tmp_path):
    import shutil
    src = tmp_path / "cat.jpg"
    shutil.copy(os.path.join(GOLDEN, "porcelain_cat_grey_background.jpg"), src)
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "spread_spectrum_watermarking_amd.cli", *a], cwd=str(tmp_path), env=env,
                                    capture_output=True, text=True, check=True, timeout=600).stdout
    run("fingerprint", str(src), "--copies", "5", "-d", "buyer")
    for i in range(5):
        assert (tmp_path / f"cat_fp{i}.png").exists()
    out = run("test", str(src), str(tmp_path / "cat_fp3.png"), str(tmp_path / "cat_fp.json"))
    assert out.count("Matches: true") == 1, out
    rec = out.split("Matches: true")[1]
    assert 'Description: "buyer #3"' in rec.split("-\n")[0], out
