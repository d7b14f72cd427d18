"""Scale attack throughput (ssw_resample_rgb8, ssw_scale_attack_rgb8, strength_report(scales=...)), timed in one process.

    python tools/resample_bench.py [--shape 4k] [--frames 64] [--threads 16] [--skip-pil] [--skip-report] [--skip-cat] [--json OUT]

1. N u8 frames to 1/2, 1/4 and 1/8 with BICUBIC and LANCZOS in one ssw_resample_rgb8 call: device events on the library's
   stream, a warm-up, then the median of 5.  The N frames (1.6 GB at 4K and 64) are far larger than the 256 MiB Infinity Cache
   and every call goes through all of them in order, so no call finds its input there.  Reported: the time; the bytes the call
   bills (include/ssw.h: frame in, plane out and in, thumbnail out) over that time as a fraction of the HBM read bandwidth
   (6.29 TB/s measured for a float4 copy, the figure tools/identify_bench.py uses); ssw_resize_rgb8 (the CatmullRom resize that is
   already in the tree) at the same shapes in the same run; and whether frame 0 equals PIL.Image.resize byte for byte.
2. Pillow doing the same N resizes on the host, on one thread and on --threads threads (its resize releases the GIL).
3. One strength_report (3 alphas, 8 copies, the defaults) on one frame with and without three scales, and the rows of the three
   scales through the host wrappers (mark_copies_rgb8 -> scale_attack -> trace_many -> quality): host clock, a warm-up, then the
   median of 3.
4. The cat (tests/golden/cat_decoded_u8.npz): k = 1000, 8 copies, seed 3, alpha 0.02 and 0.1, scales 0.5, 0.25 and 0.125 in
   BICUBIC and LANCZOS -- the table of DESIGN.md 4.16."""
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
from spread_spectrum_watermarking_amd import _lib as L  # noqa: E402
from spread_spectrum_watermarking_amd import api  # noqa: E402
from spread_spectrum_watermarking_amd.api import Context, Scale, check  # noqa: E402

SHAPES = {"4k": (3840, 2160), "8k": (7680, 4320), "1080p": (1920, 1080), "cat": (640, 444)}
HBM_READ = 6.29e12                       # bytes / s, measured (float4 copy)


def timed(stream, fn, reps=5):
    fn()
    stream.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def pil_resize(img, nw, nh, name):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((nw, nh), {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]))


def synth_u8(ctx, lib, w, h, first, n):
    """n image-like 8-bit frames from the library's own generator, on the device"""
    f32, u8 = ctx.alloc(w * h * 12), torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for i in range(n):
        check(lib.ssw_synth_frames(ctx.handle, 7, first + i, 1, w, h, f32.ptr), "ssw_synth_frames")
        check(lib.ssw_convert_f32_to_rgb8(ctx.handle, f32.ptr, w * h * 3, C.c_void_p(u8[i].data_ptr())), "ssw_convert_f32_to_rgb8")
    ctx.synchronize()
    f32.free()
    return u8


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
    gen = torch.Generator(device="cuda").manual_seed(1)
    frames = (frames.to(torch.int16) + torch.randint(-6, 7, frames.shape, dtype=torch.int16, device="cuda", generator=gen)).clamp_(0, 255).to(torch.uint8)
    host = frames.cpu().numpy()
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)
    for div in (2, 4, 8):
        nw, nh = w // div, h // div
        out = torch.empty((n, nh, nw, 3), dtype=torch.uint8, device="cuda")
        t_crate, _ = timed(stream, lambda: check(lib.ssw_resize_rgb8(ctx.handle, C.c_void_p(frames.data_ptr()), n, w, h, nw, nh, C.c_void_p(out.data_ptr())), "resize"))
        for name in ("bicubic", "lanczos"):
            f = L.RESAMPLE_FILTERS[name]
            t, ts = timed(stream, lambda: check(lib.ssw_resample_rgb8(ctx.handle, C.c_void_p(frames.data_ptr()), n, w, h, nw, nh, f, C.c_void_p(out.data_ptr())), "resample"))
            billed = n * (3 * w * h + 6 * nw * h + 3 * nw * nh)
            r = {"what": "resample", "filter": name, "shape": args.shape, "to": [nw, nh], "frames": n, "ms": round(t, 4), "ms_all": ts,
                 "billed_bytes": billed, "GB_per_s_billed": round(billed / t / 1e6, 1), "fraction_of_hbm_read": round(billed / (t * 1e-3) / HBM_READ, 3),
                 "ssw_resize_rgb8_ms": round(t_crate, 4), "frame0_equals_pillow": bool(np.array_equal(out[0].cpu().numpy(), pil_resize(host[0], nw, nh, name)))}
            if not args.skip_pil:
                pil_resize(host[0], nw, nh, name)
                t1 = wall_once(lambda: [pil_resize(im, nw, nh, name) for im in host])
                with ThreadPoolExecutor(args.threads) as pool:
                    list(pool.map(lambda im: pil_resize(im, nw, nh, name), host[:args.threads]))
                    tn = wall_once(lambda: list(pool.map(lambda im: pil_resize(im, nw, nh, name), host)))
                r.update({"pillow_one_thread_ms": round(t1, 1), "threads": args.threads, "pillow_threads_ms": round(tn, 1),
                          "device_speedup_over_one_thread": round(t1 / t, 1), "device_speedup_over_threads": round(tn / t, 1)})
            emit(r)
        del out
    del frames
    torch.cuda.empty_cache()
    ctx.set_stream(None)

    if not args.skip_report:
        img = host[0]
        alphas, sc = [0.02, 0.05, 0.1], [Scale(0.5), Scale(0.25), Scale(0.125, "lanczos")]
        t_plain = wall(lambda: api.strength_report(img, alphas, seed=3, ctx=ctx))
        t_scales = wall(lambda: api.strength_report(img, alphas, seed=3, scales=sc, ctx=ctx))
        marks = np.random.default_rng(3).standard_normal((8, 1000)).astype(np.float32)

        def through_the_host():
            for a in alphas:
                copies = api.Writer(img, api.WriteConfig(insertion=api.Insertion.Option2(a)), ctx).mark_copies_rgb8(list(marks))
                per = api.scale_attack(list(copies), sc, ctx)
                attacked = [per[i][j] for j in range(len(sc)) for i in range(8)]
                api.trace_many(img, attacked, list(marks), config=api.ReadConfig(extraction=api.Extraction.Option2(a)), ctx=ctx)
                api.quality(img, attacked, ctx)
        t_host = wall(through_the_host)
        emit({"what": "strength_report", "shape": args.shape, "alphas": alphas, "copies": 8, "scales": [s.label for s in sc], "ms": round(t_plain, 2),
              "with_scales_ms": round(t_scales, 2), "scale_rows_through_host_wrappers_ms": round(t_host, 2), "scaled_frames": len(alphas) * 8 * len(sc)})

    if not args.skip_cat:
        cat = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "cat_decoded_u8.npz"))["cat"])
        sc = [Scale(f, name) for name in ("bicubic", "lanczos") for f in (0.5, 0.25, 0.125)]
        rows = api.strength_report(cat, [0.02, 0.1], k=1000, copies=8, seed=3, scales=sc, ctx=ctx)
        emit({"what": "cat", "k": 1000, "copies": 8, "seed": 3, "rows": [
            {"alpha": r.alpha, "scales": [{"scale": s.scale, "size": list(s.size), "survived": s.survived, "accused": s.accused,
                                           "weakest_own": round(s.weakest_own, 2), "strongest_innocent": round(s.strongest_innocent, 2),
                                           "psnr_min": round(s.psnr_min, 2), "psnr_max": round(s.psnr_max, 2)} for s in r.scales]} for r in rows]})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
