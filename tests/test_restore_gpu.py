"""Tracing attacked copies on the GPU: ssw_restore_rgb8 (resize back + blend over the original, the recipes of the reference's
tests/attack_resize.rs:31-36 and tests/attack_crop.rs:56-70), the restoring trace forms and the CLI.

The yardstick of ssw_restore_rgb8 is the recipe itself, built from the oracle's CatmullRom resize (one channel triple at a
time: channels are independent, so the alpha plane is the oracle's resize of (A, A, A)) and a numpy restatement of
Rgba<u8>::blend -- compared with np.array_equal.  The trace forms are compared bit for bit with the existing trace forms run
on the frames ssw_restore_rgb8 produces."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gpu_util as G
import spread_spectrum_watermarking_amd as wm
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import Placement

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FIELDS = ("extracted", "sims", "best", "best_sim", "n_exceed")


def cat_u8():
    return np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))["cat"]


def blend_ref(o, r):
    """rgb(Rgba<u8>::blend(opaque o, r)) of `image 0.24.3`, restated: o [.., 3] u8, r [.., 4] u8.  f32, every operation rounded
    on its own, in the order the issue pins."""
    f = np.float32
    a = r[..., 3:4]
    fa, ba = a.astype(f) / f(255), f(1)
    af = (ba + fa) - ba * fa
    bg, fg = o.astype(f) / f(255), r[..., :3].astype(f) / f(255)
    with np.errstate(all="ignore"):
        out = ((fg * fa) + (bg * ba) * (f(1) - fa)) / af
    mixed = (f(255) * out).astype(np.int32).astype(np.uint8)                 # truncated toward zero
    return np.where(a == 0, o, np.where(a == 255, r[..., :3], mixed)).astype(np.uint8)


def resize_ref(s, pw, ph):
    """imageops::resize(S, pw, ph, CatmullRom) on 3 or 4 channels through the oracle's three-channel resize."""
    if (s.shape[1], s.shape[0]) == (pw, ph):
        return s
    rgb = O.resize_rgb8(np.ascontiguousarray(s[..., :3]), pw, ph)
    if s.shape[2] == 3:
        return rgb
    alpha = O.resize_rgb8(np.ascontiguousarray(np.repeat(s[..., 3:4], 3, 2)), pw, ph)[..., :1]
    return np.concatenate([rgb, alpha], 2)


def resolve(p, s, base):
    """The Python surface's rule -> (x, y, pw, ph)."""
    H, W = base.shape[:2]
    p = p or Placement()
    if p.w is not None:
        return p.x, p.y, p.w, p.h
    if (p.x, p.y) == (0, 0) and (s.shape[1], s.shape[0]) != (W, H):
        return 0, 0, W, H
    return p.x, p.y, s.shape[1], s.shape[0]


def restore_ref(base, s, p=None):
    x, y, pw, ph = resolve(p, s, base)
    r = resize_ref(s, pw, ph)
    out = base.copy()
    out[y:y + ph, x:x + pw] = r if r.shape[2] == 3 else blend_ref(base[y:y + ph, x:x + pw], r)
    return out


def rgba(rgb, alpha):
    return np.ascontiguousarray(np.concatenate([rgb, alpha[..., None].astype(np.uint8)], 2))


def roi_rgba(img, x, y, w, h):
    """The literal input of attack_crop.rs: the image with alpha 255 inside the region and 0 elsewhere."""
    a = np.zeros(img.shape[:2], np.uint8)
    a[y:y + h, x:x + w] = 255
    return rgba(img, a)


def other_image(shape, seed):
    """Something that is NOT the base, so that a wrongly kept base pixel shows."""
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def restore_cases(base):
    """(name, suspect, placement) of case 1 of the issue, on the cat (640 x 444)."""
    H, W = base.shape[:2]
    src = np.ascontiguousarray(255 - base)                       # a full-size image that differs from the base everywhere it can
    cut = np.ascontiguousarray(src[60:380, 160:560])             # 400 x 320 from (160, 60)
    ramp = np.tile(np.linspace(0, 255, W).round().astype(np.uint8), (H, 1))
    feather = np.minimum(ramp, ramp[:, ::-1]) * 2 // 1
    half_cut = O.resize_rgb8(cut, 200, 160)
    half_a = O.resize_rgb8(np.repeat(ramp[60:380, 160:560, None], 3, 2), 200, 160)[..., 0]
    cases = [
        ("whole frame from 1/8", O.resize_rgb8(src, 80, 55), None),
        ("whole frame from 1/2", O.resize_rgb8(src, 320, 222), None),
        ("whole frame from 480x300", O.resize_rgb8(src, 480, 300), None),
        ("whole frame from 2x", O.resize_rgb8(src, 1280, 888), None),
        ("rgb cut-out 225x225 at (340, 160)", np.ascontiguousarray(src[160:385, 340:565]), Placement(340, 160)),
        ("attack_crop.rs: rgba roi", roi_rgba(src, 340, 160, 225, 225), None),
        ("rgba feathered", rgba(src, np.clip(feather, 0, 255)), None),
        ("rgba ramp 0..255", rgba(src, ramp), None),
        ("half-scale cut-out rgb", half_cut, Placement(160, 60, 400, 320)),
        ("half-scale cut-out rgba", rgba(half_cut, half_a), Placement(160, 60, 400, 320)),
        ("touches left/top", other_image((50, 70, 3), 1), Placement(0, 0, 70, 50)),
        ("touches right/bottom", other_image((50, 70, 4), 2), Placement(W - 70, H - 50)),
        ("touches right, resized", other_image((31, 45, 3), 3), Placement(W - 91, 7, 91, 63)),
        ("touches bottom, resized rgba", other_image((31, 45, 4), 4), Placement(3, H - 63, 91, 63)),
        ("1x1 rgb", other_image((1, 1, 3), 5), Placement(321, 123)),
        ("1x1 rgba", np.array([[[10, 200, 30, 128]]], np.uint8), Placement(639, 443)),
        ("1x1 rectangle from 8x8", other_image((8, 8, 3), 6), Placement(5, 9, 1, 1)),
        ("odd x, odd widths rgb", other_image((37, 53, 3), 7), Placement(101, 77)),
        ("odd x, odd widths rgba", other_image((37, 53, 4), 8), Placement(203, 11)),
        ("odd everything, resized rgb", other_image((37, 53, 3), 9), Placement(11, 13, 75, 49)),
        ("odd everything, resized rgba", other_image((37, 53, 4), 10), Placement(401, 301, 75, 49)),
        ("untouched: same size, rgb, whole frame", src, None),
    ]
    return cases


def test_restore_equals_the_recipe_bit_for_bit():
    base = cat_u8()
    assert base.shape == (444, 640, 3)
    cases = restore_cases(base)
    ctx = G.ctx()
    bad = []
    for name, s, p in cases:                                      # one call per case
        got = wm.restore(base, [s], [p], ctx=ctx)[0]
        ref = restore_ref(base, s, p)
        if not np.array_equal(got, ref):
            bad.append((name, int((got != ref).sum()), int(np.abs(got.astype(int) - ref).max())))
    assert not bad, bad
    # one call holding all of the above at once, the order kept
    got = wm.restore(base, [s for _, s, _ in cases], [p for _, _, p in cases], ctx=ctx)
    for (name, s, p), g in zip(cases, got):
        assert np.array_equal(g, restore_ref(base, s, p)), name


def test_restore_on_a_frame_whose_rows_are_not_multiples_of_four():
    """W * 3 and sw * c not multiples of 4, frames of a call at odd addresses (W * H * 3 is odd)."""
    base = np.ascontiguousarray(cat_u8()[:333, :431])
    assert (base.shape[1] * 3) % 4 and (base.size % 2)
    cases = [(other_image((41, 57, 3), 20), Placement(3, 5)), (other_image((41, 57, 4), 21), Placement(373, 291)),
             (other_image((41, 57, 3), 22), Placement(100, 100, 113, 81)), (other_image((41, 57, 4), 23), Placement(1, 1, 29, 21)),
             (O.resize_rgb8(255 - base, 215, 166), None), (rgba(255 - base, other_image(base.shape[:2], 24)), None)]
    got = wm.restore(base, [s for s, _ in cases], [p for _, p in cases], ctx=G.ctx())
    for i, ((s, p), g) in enumerate(zip(cases, got)):
        assert np.array_equal(g, restore_ref(base, s, p)), i


# The fused tile's shared front end (csrc/resize_common.hpp) at its edges; what pick_resize_tile chooses for each shape, printed
# from a scratch build, is in the comment.  Every last tile is partial in both axes.  (suspect w, h, channels, rectangle w, h,
# bytes the suspect's pointer is offset by)
RESTORE_TILE_CASES = [
    (505, 487, 3, 61, 59, 0),    # rows of 1515 B (% 4 = 3): tile 8 x 16, full rows of tiles 4-word vertical pieces, the last (3 x 13) 2-word
    (505, 487, 4, 61, 59, 1),    # aligned rows behind a pointer that is not: the byte loads; tile 4 x 16, 2-word
    (53, 37, 3, 75, 49, 1),      # rows of 159 B: one tile 64 x 128 of 76544 B of LDS (> 64 KB), 49 x 75 of it used
    (211, 173, 4, 417, 341, 0),  # up-scaling with alpha: tile 32 x 128, 4 x 11 tiles, last 21 x 33
]


@pytest.mark.parametrize("sw,sh,c,pw,ph,off", RESTORE_TILE_CASES)
def test_restore_tile_edges_equal_the_recipe(sw, sh, c, pw, ph, off):
    lib, ctx = G.lib(), G.ctx()
    base = np.ascontiguousarray(cat_u8()[:ph + 7, :pw + 5])              # the rectangle at an odd position of a frame with odd rows
    s = other_image((sh, sw, c), sw + c)
    p = Placement(3, 5, pw, ph)
    H, W = base.shape[:2]
    db, dout = ctx.to_device(base), ctx.to_device(np.zeros_like(base))
    ds = ctx.to_device(np.concatenate([np.zeros(off, np.uint8), s.reshape(-1)]))
    ptrs = (C.c_void_p * 1)(ds.ptr.value + off)
    pl = (L.Placement * 1)(L.Placement(sw, sh, c, p.x, p.y, pw, ph))
    rc = lib.ssw_restore_rgb8(ctx.handle, db.ptr, W, H, ptrs, pl, 1, dout.ptr)
    got = dout.to_host(np.uint8, base.shape)
    for b in (db, ds, dout):
        b.free()
    assert rc == L.SSW_OK
    assert np.array_equal(got, restore_ref(base, s, p))


# ---- the trace forms ---------------------------------------------------------------------------------------------------------
def same(a, b, what=""):
    for name in FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (what, name)


def attack_list(copy_of, j):
    """Attack j of the issue's list on copy j -> (suspect, placement).  copy_of(j): the marked copy."""
    c = copy_of(j)
    H, W = c.shape[:2]
    rs = lambda img, w, h: G.resize_rgb8(img[None], w, h)[0]
    x, y, cw, ch = W // 4, H * 60 // 444, W * 5 // 8, H * 320 // 444          # the cat's 400 x 320 cut-out from (160, 60), scaled to the frame
    rx, ry, rw = W * 340 // 640, H * 160 // 444, W * 225 // 640
    cut = np.ascontiguousarray(c[y:y + ch, x:x + cw])
    return [lambda: (rs(c, W // 8, H // 8), None),
            lambda: (rs(c, W // 2, H // 2), None),
            lambda: (rs(c, W * 3 // 4, H * 300 // 444), None),
            lambda: (roi_rgba(c, rx, ry, rw, rw), None),
            lambda: (cut, Placement(x, y)),
            lambda: (rs(cut, cw // 2, ch // 2), Placement(x, y, cw, ch))][j % 6]()


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_trace_restored_forms_equal_trace_on_restored_frames(pinned, monkeypatch):
    """Host form (pageable and pinned suspects) and handle form against the existing forms on the pre-restored frames; the
    call mixes untouched and restored suspects and wraps the ring (3 slots) several times."""
    monkeypatch.setenv("SSW_STREAM_GROUP", "2")
    w, h, k = 768, 256, 200
    marks = np.random.default_rng(71).standard_normal((6, k)).astype(np.float32)
    base = O.f32_to_u8(O.synth_frame(71, 0, w, h))
    copies = G.fingerprint(base, marks)
    sus, pls = [], []
    for j in range(17):                                           # 9 groups of 2: the ring wraps three times
        if j % 3 == 2:
            sus.append(copies[j % 6].copy()); pls.append(None)    # untouched
        else:
            s, p = attack_list(lambda i: copies[i % 6], j)
            sus.append(s); pls.append(p)
    ctx = G.ctx()
    frames = wm.restore(base, sus, pls, ctx=ctx)
    for j in range(17):
        if j % 3 == 2:
            assert np.array_equal(frames[j], sus[j])
    if pinned:
        bufs = []
        for s in sus:
            b = ctx.pinned_empty(s.shape, np.uint8)
            b[...] = s
            bufs.append(b)
    else:
        bufs = [s.copy() for s in sus]
    ref = wm.trace_many(base, frames, list(marks), ctx=ctx)
    got = wm.trace_many(base, bufs, list(marks), ctx=ctx, placements=pls)
    same(got, ref, "host form")
    reader = wm.Reader.base(base, ctx=ctx)
    same(reader.trace(bufs, list(marks), placements=pls, base=base), reader.trace(frames, list(marks)), "handle form")
    only = reader.trace(bufs[:3], None, k=k, placements=pls[:3], base=base)       # extraction only
    assert np.array_equal(only.extracted, ref.extracted[:3])


def test_end_to_end_six_attacks_on_the_cat_name_their_copies():
    base = cat_u8()
    k = 1000
    marks = np.random.default_rng(5).standard_normal((6, k)).astype(np.float32)
    ctx = G.ctx()
    copies = wm.Writer(base, wm.WriteConfig(), ctx).mark_copies_rgb8(list(marks))
    sus = [O.resize_rgb8(copies[0], 80, 55), O.resize_rgb8(copies[1], 320, 222), O.resize_rgb8(copies[2], 480, 300),
           roi_rgba(copies[3], 340, 160, 225, 225), np.ascontiguousarray(copies[4][60:380, 160:560]),
           O.resize_rgb8(np.ascontiguousarray(copies[5][60:380, 160:560]), 200, 160)]
    pls = [None, None, None, None, Placement(160, 60), Placement(160, 60, 400, 320)]
    res = wm.trace_many(base, sus, list(marks), ctx=ctx, placements=pls)
    print("best", res.best, "best_sim", res.best_sim, "n_exceed", res.n_exceed)
    frames = wm.restore(base, sus, pls, ctx=ctx)
    for j in range(6):
        assert np.array_equal(frames[j], restore_ref(base, sus[j], pls[j])), j
        assert res.best[j] == j and res.best_sim[j] > 6.0 and res.n_exceed[j] == 1, (j, res.best, res.best_sim, res.n_exceed)
        ref_ext, _ = O.extract_frame(O.u8_to_f32(base), O.u8_to_f32(frames[j]), marks[j])
        assert G.ext_within_1e5(res.extracted[j], ref_ext), j


def test_4k_twelve_suspects():
    w, h, k = 3840, 2160, 1000
    marks = np.random.default_rng(9).standard_normal((12, k)).astype(np.float32)
    base = G.convert_f32_to_u8(G.synth(11, 0, 1, w, h))[0]
    ctx = G.ctx()
    copies = wm.Writer(base, wm.WriteConfig(), ctx).mark_copies_rgb8(list(marks))
    sus, pls = zip(*[attack_list(lambda i: copies[i], j) for j in range(12)])
    frames = wm.restore(base, sus, pls, ctx=ctx)
    ref = wm.trace_many(base, frames, list(marks), ctx=ctx)
    ctx.reset_timing()
    got = wm.trace_many(base, list(sus), list(marks), ctx=ctx, placements=list(pls))
    same(got, ref, "4K host form")
    print("4K best_sim", got.best_sim)
    assert list(got.best) == list(range(12)), (got.best, got.best_sim)
    assert ctx.prune_stats()["redone_chunks"] == 0 and ctx.select_stats()["exact_fallback_frames"] == 0


def test_pass_through_and_the_unmarked_original(monkeypatch):
    monkeypatch.setenv("SSW_STREAM_GROUP", "2")
    base = cat_u8()
    k = 500
    marks = np.random.default_rng(3).standard_normal((5, k)).astype(np.float32)
    ctx = G.ctx()
    copies = wm.Writer(base, wm.WriteConfig(), ctx).mark_copies_rgb8(list(marks))
    sus = [c.copy() for c in copies] + [base.copy()]
    H, W = base.shape[:2]
    for pls in ([None] * 6, [Placement(0, 0, W, H)] * 6, [Placement()] * 6):
        same(wm.trace_many(base, sus, list(marks), ctx=ctx, placements=pls), wm.trace_many(base, sus, list(marks), ctx=ctx), "pass-through")
    ctx.reset_timing(); ctx.enable_timing(True)
    wm.trace_many(base, sus, list(marks), ctx=ctx, placements=[None] * 6)
    ctx.synchronize()
    t = ctx.timing()
    ctx.enable_timing(False)
    assert t["resize"]["launches"] == 0, t["resize"]               # not touched by any restore launch
    # the unmarked original at half size: nobody's copy
    res = wm.trace_many(base, [O.resize_rgb8(base, W // 2, H // 2)], list(marks), ctx=ctx, placements=[None])
    assert res.n_exceed[0] == 0 and not (res.best_sim[0] > 6.0), (res.best_sim, res.sims)


def test_status_codes():
    lib, ctx = G.lib(), G.ctx()
    w, h, k = 64, 48, 50
    base = O.f32_to_u8(O.synth_frame(81, 0, w, h))
    s = other_image((24, 32, 4), 1)
    db, ds, dout = ctx.to_device(base), ctx.to_device(s), ctx.alloc(w * h * 3)
    ptrs = (C.c_void_p * 1)(ds.ptr.value)
    P = lambda *a: (L.Placement * 1)(L.Placement(*a))
    call = lambda pl, n=1: lib.ssw_restore_rgb8(ctx.handle, db.ptr, w, h, ptrs, pl, n, dout.ptr)
    assert call(P(32, 24, 4, 0, 0, 0, 0)) == L.SSW_OK
    assert call(P(32, 24, 4, 32, 24, 0, 0)) == L.SSW_OK                               # touches right and bottom
    assert call(P(32, 24, 4, 33, 24, 0, 0)) == L.SSW_ERR_BAD_ARG                      # leaves the frame
    assert call(P(32, 24, 4, 0, 25, 0, 0)) == L.SSW_ERR_BAD_ARG
    assert call(P(32, 24, 4, 0, 0, 65, 10)) == L.SSW_ERR_BAD_ARG
    assert call(P(32, 24, 4, 0xFFFFFFF0, 0, 32, 24)) == L.SSW_ERR_BAD_ARG             # x + pw wraps in 32 bits
    for ch in (0, 1, 2, 5):
        assert call(P(32, 24, ch, 0, 0, 0, 0)) == L.SSW_ERR_BAD_ARG
    assert call(P(0, 24, 4, 0, 0, 8, 8)) == L.SSW_ERR_BAD_ARG and call(P(32, 0, 4, 0, 0, 8, 8)) == L.SSW_ERR_BAD_ARG
    assert call(P(32, 24, 4, 0, 0, 8, 0)) == L.SSW_ERR_BAD_ARG and call(P(32, 24, 4, 0, 0, 0, 8)) == L.SSW_ERR_BAD_ARG
    assert call(P(32, 24, 4, 99, 99, 0, 0), 0) == L.SSW_OK                            # n == 0
    for b in (db, ds, dout):
        b.free()
    # the trace forms
    marks = np.random.default_rng(1).standard_normal((3, k)).astype(np.float32)
    hp = (C.c_void_p * 1)(s.ctypes.data)
    ext, sims, best, bs, ne = np.empty((1, k), np.float32), np.empty((1, 3), np.float32), np.empty(1, np.uint32), np.empty(1, np.float32), np.empty(1, np.uint32)
    outs = (ext.ctypes.data, sims.ctypes.data, best.ctypes.data, bs.ctypes.data, ne.ctypes.data)
    th = C.c_float(6.0)
    host = lambda cfg, pl, n, kk: lib.ssw_fingerprint_trace_restored_host_rgb8(ctx.handle, C.byref(cfg), base.ctypes.data, w, h, hp, pl, n, kk,
                                                                               marks.ctypes.data, 3, th, *outs)
    cfg = G.default_config()
    ok = P(32, 24, 4, 5, 7, 0, 0)
    assert host(cfg, ok, 1, k) == L.SSW_OK
    assert host(cfg, ok, 0, k) == L.SSW_OK
    assert host(cfg, ok, 1, w * h) == L.SSW_ERR_K_TOO_LARGE
    assert host(cfg, P(32, 24, 4, 40, 7, 0, 0), 1, k) == L.SSW_ERR_BAD_ARG
    assert host(cfg, P(32, 24, 2, 0, 0, 0, 0), 1, k) == L.SSW_ERR_BAD_ARG
    for bad in (L.Config(L.ORDER_CUSTOM, L.OPTION2, 0.1, L.PRECISION_F64), L.Config(L.ORDER_ENERGY, L.METHOD_CUSTOM, 0.1, L.PRECISION_F64)):
        assert host(bad, ok, 1, k) == L.SSW_ERR_UNSUPPORTED
    reader = wm.Reader.base(base, ctx=ctx)
    handle = lambda rd, b, pl, n, kk: lib.ssw_reader_trace_restored_host_rgb8(rd._h, b, hp, pl, n, kk, marks.ctypes.data, 3, th, *outs)
    assert handle(reader, base.ctypes.data, ok, 1, k) == L.SSW_OK
    assert handle(reader, base.ctypes.data, ok, 0, k) == L.SSW_OK
    assert handle(reader, base.ctypes.data, ok, 1, w * h) == L.SSW_ERR_K_TOO_LARGE
    assert handle(reader, None, ok, 1, k) == L.SSW_ERR_BAD_ARG                        # an RGBA suspect needs the original's pixels
    assert handle(reader, base.ctypes.data, P(32, 24, 4, 40, 7, 0, 0), 1, k) == L.SSW_ERR_BAD_ARG
    derived = wm.Reader(base, False, wm.ReadConfig(), ctx)
    assert handle(derived, base.ctypes.data, ok, 1, k) == L.SSW_ERR_NOT_BASE
    with pytest.raises(wm.SswError) as e:
        derived.trace([s], list(marks), placements=[None], base=base)
    assert e.value.status == L.SSW_ERR_NOT_BASE
    with pytest.raises(wm.SswError) as e:                          # placements=None: a mismatched shape raises as before
        reader.trace([np.ascontiguousarray(base[:24, :32])], list(marks))
    assert e.value.status == L.SSW_ERR_LENGTH_MISMATCH


def test_cli_traces_resized_cropped_and_placed_copies(tmp_path):
    from PIL import Image
    src = tmp_path / "cat.jpg"
    shutil.copy(os.path.join(GOLDEN, "porcelain_cat_grey_background.jpg"), src)
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(*a):
        r = subprocess.run([sys.executable, "-m", "spread_spectrum_watermarking_amd.cli", *a], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, check=True, timeout=600)
        return r.stdout, r.stderr
    run("fingerprint", str(src), "--copies", "4", "-d", "buyer")
    fp = [str(tmp_path / f"cat_fp{i}.png") for i in range(4)]
    imgs = [np.asarray(Image.open(p).convert("RGB")) for p in fp]
    H, W = imgs[0].shape[:2]
    half, crop, cut = str(tmp_path / "half.png"), str(tmp_path / "crop.png"), str(tmp_path / "cut.png")
    Image.fromarray(O.resize_rgb8(imgs[1], W // 2, H // 2)).save(half)
    Image.fromarray(roi_rgba(imgs[2], 340, 160, 225, 225), "RGBA").save(crop)
    Image.fromarray(np.ascontiguousarray(imgs[3][60:380, 160:560])).save(cut)
    marks = str(tmp_path / "cat_fp.json")
    today, _ = run("trace", str(src), "--suspects", fp[0], "--marks", marks)
    out, err = run("trace", str(src), "--suspects", fp[0], half, crop, cut, "--marks", marks, "--place", f"{cut}=160,60")
    records = out.split("-\n")[1:]
    assert len(records) == 4, out
    assert "-\n" + records[0] == today and "Restored:" not in records[0], (today, records[0])
    expect = [None, f"resize {W // 2}x{H // 2} -> {W}x{H}", "alpha blended over the base", "placed 400x320 at 160,60"]
    for i, path in enumerate([fp[0], half, crop, cut]):
        assert f'Suspect: "{path}"' in records[i] and "Matches: true" in records[i], out
        assert f'Description: "buyer #{i}"' in records[i] and "Also:" not in records[i], out
        if expect[i]:
            assert f'Restored: "{expect[i]}"' in records[i], out
    assert "smaller than the base" in err and half in err, err      # the whole-frame rule, said once on stderr
    assert cut not in err
