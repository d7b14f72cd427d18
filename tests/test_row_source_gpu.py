"""Replay of recorded answers through every row pre-pass and every source it reads.

The operand pre-passes of a forward row pass (csrc/dct_pair_prep.hip, dct_pair_prep_light.hip, dct_pair_derived.hip) read an
f32 plane or an interleaved RGB frame (f32, 8-bit, 16-bit), form Y -- and I, Q for the writer -- and fold Y into the f64
operand planes.  tests/golden/row_source_digests.json holds one SHA-256 per case below, recorded from a library built from the
commit BEFORE the pre-passes were given one typed row source (loaded through SSW_LIB_PATH): the loaded library must reproduce
every one of them, bit for bit.  The file is a recorded fact -- never regenerate it from the code under test.

A case is (row kernel) x (source) x (with I/Q: ssw_batch_embed*, the writer | without: ssw_batch_extract*, the reader |
f32 plane: ssw_dct2d forward and orthonormal).  Widths are chosen so that only the named kernel can take them; every case
asserts through ssw_ctx_transform_plan, the prune counters and the bytes the colour-conversion stage was billed that it took
the path it is named for, so a case that silently falls to another kernel fails instead of passing.

Inputs: ssw_synth_frames(seed 7); 8- and 16-bit frames are those f32 frames quantised once on the host, round half up."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "row_source_digests.json")
K = 16                                   # mark length: prune capacity 64 columns, so frames of 256 columns and more prune
FMTS = ("f32", "u8", "u16")
PIX_BYTES = {"f32": 4, "u8": 1, "u16": 2}
FUSED_FRAMES = 28                        # smallest batch of 256-column frames whose forward transform fuses (found on the parent)
FUSED_TUNING = dict(efold_min=256, efold_cols_min=64, deep_min_cols=128)

# (group, tuning, dct folding or None, [(w, h, frames, derived route, plan flags that must be set, ... that must be clear)])
# derived route of ssw_batch_extract*: "full" -- the prune set-up declines (capacity * 4 > w), the derived frame takes the same
# pre-pass as the base frame; "gathered" -- pruned_rows_gathered: the pre-pass with null I/Q, then the subset products;
# "onekernel" -- prep16_derived_fused_kernel.  The 144- and 160-column shapes decline (4 * 64 > w): the gathered route reaches
# the 4- and 8-level kernels on 272 and 288 columns instead (w % 64 != 0: not deep; 288 % 32 == 0 under forced folding).
GROUPS = [
    ("4-level", {}, None, [(80, 48, 3, "full", ("pair_f64",), ("rows_deep",)),                 # w % 16 == 0, w < 128: no odd split
                           (144, 64, 3, "full", ("pair_f64",), ("rows_deep",)),                # w >= 128, w % 64 != 0: split odd half
                           (272, 64, 3, "gathered", ("pair_f64",), ("rows_deep",))]),
    ("8-level", {}, None, [(3104, 16, 2, "gathered", ("pair_f64",), ("rows_deep",))]),        # w >= 3072, w % 32 == 0, w % 64 != 0
    ("8-level-forced", {}, 6, [(160, 64, 3, "full", ("pair_f64",), ("rows_deep",)),
                               (288, 64, 3, "gathered", ("pair_f64",), ("rows_deep",))]),
    ("16-level-l1", {}, None, [(256, 64, 3, "gathered", ("rows_deep",), ("rows_level2",))]),  # deep_min_rows = 256 <= w < efold_min
    ("16-level-l2-register", dict(efold_min=256, prep_light=0), None, [(256, 64, 3, "gathered", ("rows_level2",), ("fused_cols",))]),
    ("16-level-l2-light", dict(efold_min=256), None, [(256, 64, 3, "gathered", ("rows_level2",), ("fused_cols",)),
                                                      (320, 64, 3, "gathered", ("rows_level2",), ("fused_cols",))]),   # w / 16 = 20: padding branch
    # unit-ordered lines of the fused forward transform.  256 x 128 cannot fuse at any frame count (its 8 units per frame are
    # fewer than the two k-blocks an operand plane has at least): it stays here as a level-2 case that must NOT report fused_cols;
    # 256 x 256 fuses without padding units, 256 x 144 (9 units in 16) with them.
    ("fused-light", FUSED_TUNING, None, [(256, 256, FUSED_FRAMES, "gathered", ("rows_level2", "cols_level2", "fused_cols"), ()),
                                         (256, 144, FUSED_FRAMES, "gathered", ("rows_level2", "cols_level2", "fused_cols"), ()),
                                         (256, 128, FUSED_FRAMES, "gathered", ("rows_level2",), ("fused_cols",))]),
    ("fused-register", dict(FUSED_TUNING, prep_light=0), None,
     [(256, 256, FUSED_FRAMES, "gathered", ("rows_level2", "cols_level2", "fused_cols"), ()),
      (256, 144, FUSED_FRAMES, "gathered", ("rows_level2", "cols_level2", "fused_cols"), ())]),
]
# derived frame only (ssw_batch_extract*): n * h above merge_max_lines takes the one-kernel pruned row pass
DERIVED = [
    ("derived-onekernel", dict(efold_min=256, merge_max_lines=1024), [(256, 128, 9, "onekernel")]),
    ("derived-gathered", dict(efold_min=256, merge_max_lines=1024, derived_fused=0), [(256, 128, 9, "gathered"), (256, 128, 1, "gathered")]),
]
PLANE_GROUPS = ("8-level", "8-level-forced", "16-level-l1", "16-level-l2-register", "16-level-l2-light", "fused-light", "fused-register")


def _quantise(f32, fmt):
    if fmt == "f32":
        return f32
    top, dt = (255.0, np.uint8) if fmt == "u8" else (65535.0, np.uint16)
    return np.floor(np.clip(f32.astype(np.float64), 0.0, 1.0) * top + 0.5).astype(dt)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class _Run:
    """One context under one tuning: the calls of a case, their digests and their path assertions."""

    def __init__(self, ctx, digests, problems):
        from spread_spectrum_watermarking_amd import _lib as L
        self.L, self.ctx, self.lib = L, ctx, ctx._lib
        self.digests, self.problems = digests, problems
        self.cfg = L.Config(L.ORDER_ENERGY, L.OPTION2, 0.1, L.PRECISION_F64)
        self.frames = {}
        ctx.enable_timing(True)

    def expect(self, ok, what):
        if not ok:
            self.problems.append(what)

    def synth(self, w, h, n, fmt):
        """2 n frames: the first n are base frames, the others derived ones."""
        from spread_spectrum_watermarking_amd.api import check
        if (w, h, n) not in self.frames:
            d = self.ctx.alloc(2 * n * h * w * 12)
            check(self.lib.ssw_synth_frames(self.ctx.handle, 7, 0, 2 * n, w, h, d.ptr), "ssw_synth_frames")
            self.frames = {(w, h, n): {"f32": d.to_host(np.float32, (2 * n, h, w, 3))}}      # (one shape at a time)
            d.free()
        by_fmt = self.frames[(w, h, n)]
        if fmt not in by_fmt:
            by_fmt[fmt] = _quantise(by_fmt["f32"], fmt)
        return by_fmt[fmt]

    def rgb_bytes(self):
        return self.ctx.timing()["rgb_to_yiq"]["work"]

    def plan(self, key, n, w, h, must, must_not):
        p = self.ctx.transform_plan(self.ctx.pass_frames(n, w, h), w, h)
        self.expect(all(p[f] for f in must) and not any(p[f] for f in must_not), f"{key}: plan {p}")

    def embed(self, key, fmt, w, h, n, offset=0, fused=True):
        from spread_spectrum_watermarking_amd.api import check
        ctx, lib = self.ctx, self.lib
        frames = self.synth(w, h, n, fmt)[:n]
        marks = np.random.default_rng(3).standard_normal((n, K)).astype(np.float32)
        src = ctx.alloc(frames.nbytes + 16)
        at = C.c_void_p(src.ptr.value + offset)
        check(lib.ssw_copy_to_dev(ctx.handle, at, frames.ctypes.data, frames.nbytes), "ssw_copy_to_dev")
        dm = ctx.to_device(marks)
        px = n * h * w
        ctx.reset_timing()
        if fmt == "f32":
            out, coef, idx = ctx.alloc(px * 12), ctx.alloc(px * 4), ctx.alloc(n * K * 4)
            check(lib.ssw_batch_embed(ctx.handle, C.byref(self.cfg), at, n, w, h, dm.ptr, K, out.ptr, coef.ptr, idx.ptr), key)
            got = [out.to_host(np.float32, (n, h, w, 3)), coef.to_host(np.float32, (n, h, w)), idx.to_host(np.uint32, (n, K))]
            bufs = [out, coef, idx]
        elif fmt == "u8":
            out = ctx.alloc(px * 3)
            check(lib.ssw_batch_embed_rgb8(ctx.handle, C.byref(self.cfg), at, n, w, h, dm.ptr, K, out.ptr), key)
            got, bufs = [out.to_host(np.uint8, (n, h, w, 3))], [out]
        else:
            out = ctx.alloc(px * 12)
            check(lib.ssw_batch_embed_rgb16(ctx.handle, C.byref(self.cfg), at, n, w, h, dm.ptr, K, out.ptr), key)
            got, bufs = [out.to_host(np.float32, (n, h, w, 3))], [out]
        # the fused pre-pass reads the frame and writes Y's operands (8 B/px) and I, Q; the separate kernel writes three f32 planes
        want = px * (3.0 * PIX_BYTES[fmt] + (16.0 if fused else 12.0))
        self.expect(self.rgb_bytes() == want, f"{key}: colour stage billed {self.rgb_bytes()} bytes, the named path bills {want}")
        for b in bufs + [src, dm]:
            b.free()
        self.digests[key] = _sha(*got)

    def extract(self, key, fmt, w, h, n, route):
        from spread_spectrum_watermarking_amd.api import check
        ctx, lib = self.ctx, self.lib
        frames = self.synth(w, h, n, fmt)
        marks = np.random.default_rng(4).standard_normal((n, K)).astype(np.float32)
        base, derived, dm = ctx.to_device(frames[:n]), ctx.to_device(frames[n:]), ctx.to_device(marks)
        ext, sims = ctx.alloc(n * K * 4), ctx.alloc(n * 4)
        fn = {"f32": lib.ssw_batch_extract, "u8": lib.ssw_batch_extract_rgb8, "u16": lib.ssw_batch_extract_rgb16}[fmt]
        ctx.reset_timing()                                          # (zeroes the prune counters too)
        check(fn(ctx.handle, C.byref(self.cfg), base.ptr, derived.ptr, n, w, h, K, ext.ptr, dm.ptr, sims.ptr), key)
        got = [ext.to_host(np.float32, (n, K)), sims.to_host(np.float32, (n,))]
        stats = ctx.prune_stats()
        pruned, redone = stats["pruned_chunks"], stats["redone_chunks"]
        self.expect((pruned > 0) == (route != "full") and redone == 0, f"{key}: route {route}, pruned chunks {pruned}, redone {redone}")
        px, pb = n * h * w, 3.0 * PIX_BYTES[fmt]
        cap = 64                                                    # prune capacity of k = 16
        want = px * (pb + 8.0) + (px * pb + n * h * cap * 4.0 if route == "onekernel" else px * (pb + 8.0))
        self.expect(self.rgb_bytes() == want, f"{key}: colour stage billed {self.rgb_bytes()} bytes, route {route} bills {want}")
        for b in (base, derived, dm, ext, sims):
            b.free()
        self.digests[key] = _sha(*got)

    def planes(self, key, w, h, n):
        from spread_spectrum_watermarking_amd.api import check
        ctx, lib, L = self.ctx, self.lib, self.L
        rgb = ctx.to_device(self.synth(w, h, n, "f32")[:n])
        y = ctx.alloc(n * h * w * 4)
        check(lib.ssw_rgb_to_yiq(ctx.handle, rgb.ptr, n, w, h, y.ptr, None, None), "ssw_rgb_to_yiq")
        y0 = y.to_host(np.float32, (n, h, w))
        for kind, name in ((L.DCT2, "forward"), (L.DCT2_ORTHOGONAL, "orthonormal")):
            t = ctx.to_device(y0)
            check(lib.ssw_dct2d(ctx.handle, kind, L.PRECISION_F64, n, w, h, t.ptr), key)
            self.digests[f"{key} {name}"] = _sha(t.to_host(np.float32, (n, h, w)))
            t.free()
        rgb.free(); y.free()


def generate(problems=None):
    """{case: sha256} of the loaded library; path assertions that fail are appended to `problems` (None: raised at the end)."""
    import spread_spectrum_watermarking_amd as wm
    from spread_spectrum_watermarking_amd import tuning
    digests, found = {}, [] if problems is None else problems
    for group, tune, folding, shapes in GROUPS:
        with tuning(**tune):
            ctx = wm.Context(0)
            if folding is not None:
                ctx.set_dct_folding(folding)
            run = _Run(ctx, digests, found)
            if "prep_light" in tune or "light" in group:
                run.expect(tuning.get("prep_light") == (0 if "register" in group else 1), f"{group}: prep_light")
            for (w, h, n, route, must, must_not) in shapes:
                tag = f"{group} {w}x{h}x{n}"
                run.plan(tag, n, w, h, must, must_not)
                if group.startswith("fused") and "fused_cols" in must:      # the smallest batch that fuses
                    p = ctx.transform_plan(FUSED_FRAMES - 1, w, h)
                    run.expect(not p["fused_cols"], f"{tag}: {FUSED_FRAMES - 1} frames fuse already")
                if group.startswith("fused") and "fused_cols" in must_not:
                    run.expect(not any(ctx.transform_plan(m, w, h)["fused_cols"] for m in (1, 8, 64, 512, 4096)), f"{tag}: fuses")
                for fmt in FMTS:
                    run.embed(f"{tag} embed {fmt}", fmt, w, h, n)
                    run.extract(f"{tag} extract {fmt}", fmt, w, h, n, route)
                if group in PLANE_GROUPS:
                    run.planes(f"{tag} plane", w, h, n)
            ctx.close()
    for group, tune, shapes in DERIVED:
        with tuning(**tune):
            ctx = wm.Context(0)
            run = _Run(ctx, digests, found)
            for (w, h, n, route) in shapes:
                run.plan(f"{group} {w}x{h}x{n}", n, w, h, ("rows_level2",), ())
                for fmt in FMTS:
                    run.extract(f"{group} {w}x{h}x{n} extract {fmt}", fmt, w, h, n, route)
            ctx.close()
    # an 8-bit frame pointer one byte off: the alignment mask declines the fused pre-pass, the separate colour conversion runs
    ctx = wm.Context(0)
    run = _Run(ctx, digests, found)
    run.plan("misaligned 256x64x3", 3, 256, 64, ("rows_deep",), ("rows_level2",))
    run.embed("misaligned 256x64x3 embed u8", "u8", 256, 64, 3, offset=1, fused=False)
    # a 16-bit single-image handle
    w, h = 256, 64
    frame = run.synth(w, h, 1, "u16")[0]
    mark = np.random.default_rng(5).standard_normal(K).astype(np.float32)
    run.plan("handle-u16 256x64", 1, w, h, ("rows_deep",), ("rows_level2",))
    writer = wm.Writer(frame, wm.WriteConfig(), ctx)
    coef = writer.coefficient_image()
    marked = writer.mark([mark])
    reader = wm.Reader.base(frame, wm.ReadConfig(), ctx)
    idx = reader.indices(K)
    ext = reader.extract(wm.Reader.derived(_quantise(marked, "u16"), ctx), K)
    digests["handle-u16 256x64 writer"] = _sha(coef, marked)
    digests["handle-u16 256x64 reader"] = _sha(idx, ext)
    del writer, reader
    ctx.close()
    if problems is None:
        assert not found, "\n".join(found)
    return digests


@pytest.fixture(scope="module")
def replay():
    return generate()


with open(GOLDEN) as _f:
    _WANT = json.load(_f)["digests"]


@pytest.mark.gpu
def test_every_recorded_case_is_still_a_case(replay):
    assert set(replay) == set(_WANT)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_WANT))
def test_row_source_reproduces_the_recorded_digest(replay, case):
    assert replay.get(case) == _WANT[case], case
