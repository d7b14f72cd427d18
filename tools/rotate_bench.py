"""Rotation attack throughput (ssw_affine_rgb8, ssw_unrotate_rgb8, strength_report(rotations=...)), timed in one process.

    python tools/rotate_bench.py [--shape 4k] [--frames 64] [--threads 16] [--skip-pil] [--skip-report] [--skip-cat] [--json OUT]

1. N u8 frames turned by 1 and by 30 degrees with BILINEAR and BICUBIC in one ssw_affine_rgb8 call, and turned back in one
   ssw_unrotate_rgb8 call (the fused undo): device events on the library's stream, a warm-up, then the median of 5.  The N frames
   (1.6 GB at 4K and 64) are far larger than the 256 MiB Infinity Cache and every call goes through all of them in order, so no
   call finds its input there.  Reported: the time; the bytes the call bills (include/ssw.h: frame in, frame out) over that time
   as a fraction of the HBM read bandwidth (6.29 TB/s measured for a float4 copy, the figure tools/resample_bench.py uses); the
   f64 operations a pixel executes (counted from csrc/affine.hip: every multiply, add, negation, floor and conversion one
   operation, nothing fused) over that time as a fraction of the f64 vector issue rate (39.3e12 operations a second: the
   78.6 TFLOPS of the data sheet count a fused multiply-add twice, and nothing here is fused); and whether frame 0 equals
   PIL.Image.rotate byte for byte.
2. Pillow doing the same N rotations on the host, on one thread and on --threads threads (its transform releases the GIL).
3. One strength_report (3 alphas, 8 copies, the defaults) on one frame with and without three rotations: host clock, a warm-up,
   then the median of 3.
4. The cat (tests/golden/cat_decoded_u8.npz): k = 1000, 8 copies, seed 3, alpha 0.02 and 0.1, rotations 0.25, 1 and 5 degrees in
   BICUBIC and BILINEAR -- the table of DESIGN.md 4.17."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from spread_spectrum_watermarking_amd import _lib as L  # noqa: E402
from spread_spectrum_watermarking_amd import api  # noqa: E402
from spread_spectrum_watermarking_amd.api import Context, Rotate, check  # noqa: E402
from resample_bench import HBM_READ, SHAPES, synth_u8, timed  # noqa: E402

F64_ISSUE = 39.3e12                      # f64 vector operations / s (data sheet: 78.6 TFLOPS with a fused multiply-add as two)
# operations a pixel under the frame executes: the sample point and base position (16), per channel the taps' conversions and
# the filter (BILINEAR 4 + 9, BICUBIC 16 + 5 cubics of 16), the conversion back; the undo adds four forward sample points
OPS = {"bilinear": 16 + 3 * (4 + 9 + 1), "bicubic": 16 + 3 * (16 + 80 + 1), "undo": 16 + 3 * (16 + 80 + 1) + 4 * 8}


def pil_rotate(img, angle, name):
    from PIL import Image
    return np.asarray(Image.fromarray(img).rotate(angle, resample={"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[name]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4k")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-pil", action="store_true")
    ap.add_argument("--skip-report", action="store_true")
    ap.add_argument("--skip-cat", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    lib = L.load()
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    def wall_once(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def wall(fn, reps=3):
        fn()
        ts = []
        for _ in range(reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    w, h = SHAPES[args.shape]
    n = args.frames
    frames = synth_u8(ctx, lib, w, h, 0, n)
    host = frames.cpu().numpy()
    out = torch.empty_like(frames)
    base = frames[0].clone()
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    fill = (C.c_uint8 * 3)(0, 0, 0)
    billed = n * 6 * w * h

    def figures(t, ops):
        return {"billed_bytes": billed, "GB_per_s_billed": round(billed / t / 1e6, 1), "fraction_of_hbm_read": round(billed / (t * 1e-3) / HBM_READ, 3),
                "f64_ops_per_pixel": ops, "fraction_of_f64_issue": round(n * w * h * ops / (t * 1e-3) / F64_ISSUE, 3)}

    for angle in (1.0, 30.0):
        m = (C.c_double * 6)(*api.rotation_matrix(angle, w, h))
        for name in ("bilinear", "bicubic"):
            f = L.AFFINE_FILTERS[name]
            t, ts = timed(stream, lambda: check(lib.ssw_affine_rgb8(ctx.handle, ptr(frames), n, w, h, w, h, m, f, fill, ptr(out)), "affine"))
            r = {"what": "rotate", "angle": angle, "filter": name, "shape": args.shape, "frames": n, "ms": round(t, 4), "ms_all": ts, **figures(t, OPS[name]),
                 "frame0_equals_pillow": bool(np.array_equal(out[0].cpu().numpy(), pil_rotate(host[0], angle, name)))}
            if not args.skip_pil:
                pil_rotate(host[0], angle, name)
                t1 = wall_once(lambda: [pil_rotate(im, angle, name) for im in host])
                with ThreadPoolExecutor(args.threads) as pool:
                    list(pool.map(lambda im: pil_rotate(im, angle, name), host[:args.threads]))
                    tn = wall_once(lambda: list(pool.map(lambda im: pil_rotate(im, angle, name), host)))
                r.update({"pillow_one_thread_ms": round(t1, 1), "threads": args.threads, "pillow_threads_ms": round(tn, 1),
                          "device_speedup_over_one_thread": round(t1 / t, 1), "device_speedup_over_threads": round(tn / t, 1)})
            emit(r)
        jobs = (L.RotateJob * n)(*[Rotate(angle).job(i, w, h) for i in range(n)])
        turned = out.clone()                                             # the BICUBIC rotation above: the suspects
        t, ts = timed(stream, lambda: check(lib.ssw_unrotate_rgb8(ctx.handle, ptr(base), ptr(turned), n, w, h, jobs, ptr(out)), "unrotate"))
        emit({"what": "unrotate", "angle": angle, "shape": args.shape, "frames": n, "ms": round(t, 4), "ms_all": ts, **figures(t, OPS["undo"]),
              "kept": round(Rotate(angle).kept(w, h), 4)})
        del turned
    del frames, out
    torch.cuda.empty_cache()
    ctx.set_stream(None)

    if not args.skip_report:
        img = host[0]
        alphas, ro = [0.02, 0.05, 0.1], [Rotate(0.5), Rotate(2, "bilinear"), Rotate(-1)]
        t_kept_host = wall_once(lambda: [r.kept(w, h) for r in ro])
        t_kept = wall(lambda: api._kept_shares(ctx, ro, w, h))
        t_plain = wall(lambda: api.strength_report(img, alphas, seed=3, ctx=ctx))
        t_rot = wall(lambda: api.strength_report(img, alphas, seed=3, rotations=ro, ctx=ctx))
        emit({"what": "strength_report", "shape": args.shape, "alphas": alphas, "copies": 8, "rotations": [r.label for r in ro], "ms": round(t_plain, 2),
              "with_rotations_ms": round(t_rot, 2), "of_which_kept_shares_ms": round(t_kept, 2), "kept_shares_in_numpy_on_the_host_ms": round(t_kept_host, 2), "rotated_frames": len(alphas) * 8 * len(ro)})

    if not args.skip_cat:
        cat = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "cat_decoded_u8.npz"))["cat"])
        ro = [Rotate(a, name) for name in ("bicubic", "bilinear") for a in (0.25, 1, 5)]
        rows = api.strength_report(cat, [0.02, 0.1], k=1000, copies=8, seed=3, rotations=ro, ctx=ctx)
        emit({"what": "cat", "k": 1000, "copies": 8, "seed": 3, "rows": [
            {"alpha": r.alpha, "rotations": [{"rotation": s.rotation, "kept": round(s.kept, 4), "survived": s.survived, "accused": s.accused,
                                              "weakest_own": round(s.weakest_own, 2), "strongest_innocent": round(s.strongest_innocent, 2),
                                              "psnr_min": round(s.psnr_min, 2), "psnr_max": round(s.psnr_max, 2)} for s in r.rotations]} for r in rows]})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
