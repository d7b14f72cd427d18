#!/usr/bin/env python3
"""Bit-for-bit A/B of two builds of the library (e.g. lib/libssw_hip.so against a variant of tools/build_variant.sh): every build
runs in a child process (SSW_LIB_PATH), transforms the same synthetic frames -- ssw_dct2d forward, orthonormal and inverse on
shapes of every strategy, one batch embed + extract, one trace at two chunks, one handle extract against a derived frame that
is still RGB (the three users of the pruned derived transform) -- and prints a digest per case; the parent compares the digests.
usage: python tools/lib_ab_check.py [--stages] LIB_A LIB_B
       --stages: also the stage accounts of every case (ssw_ctx_get_timing launch counts, ssw_ctx_get_work, ssw_ctx_get_traffic),
                 the cases again at folding levels 0, 1, 3, 4, 6 and with the odd split off on the 4K, 1080p and 512 x 272 shapes,
                 and every case in SSW_PRECISION_F32 (the dense f32 kernels)
       python tools/lib_ab_check.py --golden LIB OUT.json     (writes the digests of one build, in the format of
                                                              tests/golden/gemm_digests.json: the r5 kernel's digests, kept as recorded)"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2160, 3840, 8), (2160, 3840, 1), (1080, 1920, 12), (720, 1280, 20), (4320, 7680, 2), (272, 512, 40), (444, 640, 3), (2160, 3840, 3)]
BATCH = ((2160, 3840, 8), (1080, 1920, 12), (272, 512, 40))
# --stages: non-default strategy settings, each on these shapes (the first tag is the default, covered by SHAPES)
SETTINGS = (("fold0", "set_dct_folding", 0), ("fold1", "set_dct_folding", 1), ("fold3", "set_dct_folding", 3),
            ("fold4", "set_dct_folding", 4), ("fold6", "set_dct_folding", 6), ("nosplit", "set_odd_split", False))
SETTING_SHAPES = ((2160, 3840, 8), (1080, 1920, 12), (272, 512, 40))


def child():
    import ctypes as C
    import numpy as np
    sys.path.insert(0, ROOT)
    import spread_spectrum_watermarking_amd as wm
    from spread_spectrum_watermarking_amd import _lib as L
    from spread_spectrum_watermarking_amd.api import check
    ctx = wm.Context(0)
    lib = ctx._lib
    stages = os.environ.get("SSW_AB_STAGES") == "1"
    if stages:
        ctx.enable_timing(True)
        ctx.reset_timing()

    def accounts(case):
        # launches, work and traffic of every stage the case used (one token: the parent compares it like a digest)
        if not stages:
            return
        t = ctx.timing()
        acc = ",".join(f"{s}:{v['launches']}:{v['work']!r}:{v['bytes']!r}" for s, v in t.items() if v["launches"] or v["work"] or v["bytes"])
        print(f"DIGEST stages {case} {acc}", flush=True)
        ctx.reset_timing()

    cases = [(h, w, n, "") for (h, w, n) in SHAPES]
    if stages:
        cases += [(h, w, n, tag) for tag, _, _ in SETTINGS for (h, w, n) in SETTING_SHAPES]
        cases += [(h, w, n, "f32") for (h, w, n) in SHAPES]
    for (h, w, n, tag) in cases:
        prec = L.PRECISION_F32 if tag == "f32" else L.PRECISION_F64
        for t, fn, val in SETTINGS:
            if t == tag:
                getattr(ctx, fn)(val)
        pre = f"{tag} " if tag else ""
        rgb = ctx.alloc(n * h * w * 12)
        check(lib.ssw_synth_frames(ctx.handle, 7, 0, n, w, h, rgb.ptr), "synth")
        y = ctx.alloc(n * h * w * 4)
        check(lib.ssw_rgb_to_yiq(ctx.handle, rgb.ptr, n, w, h, y.ptr, None, None), "yiq")
        y0 = y.to_host(np.float32, (n, h, w))
        if stages:
            ctx.reset_timing()
        for kind, name in ((L.DCT2, "fwd"), (L.DCT2_ORTHOGONAL, "ortho"), (L.DCT3, "inv")):
            t = ctx.to_device(y0)
            check(lib.ssw_dct2d(ctx.handle, kind, prec, n, w, h, t.ptr), "dct")
            out = t.to_host(np.float32, (n, h, w))
            print(f"DIGEST {pre}dct {h}x{w}x{n} {name} {hashlib.sha256(out.tobytes()).hexdigest()[:16]}", flush=True)
            accounts(f"{pre}dct {h}x{w}x{n} {name}")
            t.free()
        if (h, w, n) in BATCH:
            k = 500
            marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
            dm = ctx.to_device(marks)
            out, ext, sims = ctx.alloc(n * h * w * 12), ctx.alloc(n * k * 4), ctx.alloc(n * 4)
            cfg = L.Config(L.ORDER_ENERGY, L.OPTION2, 0.1, prec)
            check(lib.ssw_batch_embed(ctx.handle, C.byref(cfg), rgb.ptr, n, w, h, dm.ptr, k, out.ptr, None, None), "embed")
            check(lib.ssw_batch_extract(ctx.handle, C.byref(cfg), rgb.ptr, out.ptr, n, w, h, k, ext.ptr, dm.ptr, sims.ptr), "extract")
            for nm, b, shp in (("marked", out, (n, h, w, 3)), ("ext", ext, (n, k)), ("sims", sims, (n,))):
                print(f"DIGEST {pre}batch {h}x{w}x{n} {nm} {hashlib.sha256(b.to_host(np.float32, shp).tobytes()).hexdigest()[:16]}", flush=True)
            accounts(f"{pre}batch {h}x{w}x{n}")
            for b in (dm, out, ext, sims):
                b.free()
        rgb.free(); y.free()
        if tag:
            ctx.set_dct_folding(True)
            ctx.set_odd_split(True)
    if os.environ.get("SSW_AB_PRUNE_USERS") == "1":      # the A/B only: tests/golden/gemm_digests.json predates these cases
        # the other two users of the pruned derived transform: ssw_fingerprint_trace at two chunks (the call's tables, read by both
        # chunks), and a handle Reader.extract against a derived frame that is still RGB (lane 0's tables, one frame)
        h, w, n, k = 1080, 1920, 6, 500
        cfg = L.Config(L.ORDER_ENERGY, L.OPTION2, 0.1, L.PRECISION_F64)
        marks = np.random.default_rng(4).standard_normal((n, k)).astype(np.float32)
        base, dm = ctx.alloc(h * w * 12), ctx.to_device(marks)
        check(lib.ssw_synth_frames(ctx.handle, 7, 0, 1, w, h, base.ptr), "synth")
        sus, ext, sims = ctx.alloc(n * h * w * 12), ctx.alloc(n * k * 4), ctx.alloc(n * n * 4)
        best, best_sim, n_exceed = ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4)
        check(lib.ssw_fingerprint_embed(ctx.handle, C.byref(cfg), base.ptr, w, h, dm.ptr, n, k, sus.ptr, None), "fingerprint")
        ctx.set_chunk_frames(3)
        if stages:
            ctx.reset_timing()
        check(lib.ssw_fingerprint_trace(ctx.handle, C.byref(cfg), base.ptr, sus.ptr, n, w, h, k, dm.ptr, n, C.c_float(6.0), ext.ptr, sims.ptr,
                                        best.ptr, best_sim.ptr, n_exceed.ptr), "trace")
        ctx.set_chunk_frames(0)
        for nm, b, dt, shp in (("ext", ext, np.float32, (n, k)), ("sims", sims, np.float32, (n, n)), ("best", best, np.uint32, (n,))):
            print(f"DIGEST trace {h}x{w}x{n} {nm} {hashlib.sha256(b.to_host(dt, shp).tobytes()).hexdigest()[:16]}", flush=True)
        accounts(f"trace {h}x{w}x{n}")
        frame, copy = base.to_host(np.float32, (h, w, 3)), sus.to_host(np.float32, (n, h, w, 3))[0]
        for b in (base, dm, sus, ext, sims, best, best_sim, n_exceed):
            b.free()
        reader = wm.Reader.base(frame, wm.ReadConfig(precision=wm.Precision.F64), ctx)
        if stages:
            ctx.reset_timing()
        got = reader.extract(wm.Reader.derived(copy, ctx, wm.Precision.F64), k)
        print(f"DIGEST handle {h}x{w} ext {hashlib.sha256(np.asarray(got, np.float32).tobytes()).hexdigest()[:16]}", flush=True)
        accounts(f"handle {h}x{w}")
    ctx.close()


def digests(lib=None, env=None):
    """{case: digest} of one build (None: the default library), computed in a child process."""
    e = dict(os.environ, **(env or {}))
    if lib:
        e["SSW_LIB_PATH"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=e, capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-3000:])
    return {" ".join(l.split()[1:-1]): l.split()[-1] for l in r.stdout.splitlines() if l.startswith("DIGEST")}


def main():
    if sys.argv[1] == "--golden":
        import json
        d = digests(sys.argv[2])
        with open(sys.argv[3], "w") as f:
            # (the committed tests/golden/gemm_digests.json was written from the r5 register-staged GEMM kernel, which is no longer
            # built: it records that kernel's planes, do not regenerate it)
            json.dump({"_how": "python tools/lib_ab_check.py --golden <library> OUT.json "
                               "-- sha256[:16] of the f32 outputs on ssw_synth_frames(seed 7) inputs",
                       "digests": d}, f, indent=1)
        print(f"{len(d)} digests -> {sys.argv[3]}")
        return 0
    args = [a for a in sys.argv[1:] if a != "--stages"]
    env = {"SSW_AB_PRUNE_USERS": "1"}
    if "--stages" in sys.argv:
        env["SSW_AB_STAGES"] = "1"
    libs = args[:2]
    try:
        res = [digests(lib, env) for lib in libs]
    except RuntimeError as e:
        print(e)
        return 2
    bad = 0
    for key in res[0]:
        same = res[0][key] == res[1].get(key)
        bad += not same
        print(("same   " if same else "DIFFER ") + key, res[0][key], res[1].get(key))
    print(f"{len(res[0])} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        sys.exit(main())
