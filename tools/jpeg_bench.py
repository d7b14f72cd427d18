"""JPEG attack throughput (ssw_jpeg_rgb8, strength_report(jpeg=...)), timed in one process.

    python tools/jpeg_bench.py [--shape 4k] [--frames 64] [--quality 75] [--threads 16] [--skip-pil] [--skip-report] [--json OUT]

1. N u8 frames at one quality in one call: device events on the library's stream, a warm-up, then the median of 5.  The N frames
   and their N results (1.6 GB each at 4K and 64) are each far larger than the 256 MiB Infinity Cache and every call goes through
   all of them in order, so no call finds its input there.  Reported: the time, the bytes the two passes move (per job the
   frame in and out and the decoded planes out and in again, about 9 B/px) over that time as a fraction of the HBM read
   bandwidth (6.29 TB/s measured for a float4 copy, the figure tools/identify_bench.py uses), and whether frame 0 equals PIL's
   round trip byte for byte.
2. PIL (libjpeg-turbo) doing the same N save / open round trips on the host, on one thread and on --threads threads (the codec
   releases the GIL): what the docs recommended before the device call existed.  The frames are on the host already; the two
   PCIe crossings per frame that the host route also needs are not counted.
3. One strength_report (3 alphas, 8 copies, the defaults) on one frame with and without jpeg=(90, 75, 50, 25): host clock, a
   warm-up, then the median of 3."""
import argparse
import ctypes as C
import io
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
from spread_spectrum_watermarking_amd.api import Context, check  # noqa: E402

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


def pil_round_trip(img, quality):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", quality=quality)
    f.seek(0)
    return np.asarray(Image.open(f).convert("RGB"))


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
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-pil", action="store_true")
    ap.add_argument("--skip-report", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    lib = L.load()
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    w, h = SHAPES[args.shape]
    fb, n, q = w * h * 3, args.frames, args.quality
    frames = synth_u8(ctx, lib, w, h, 0, n)
    # a little noise on top: the generator's frames are smooth, and smooth blocks quantise to nothing but their DC
    gen = torch.Generator(device="cuda").manual_seed(1)
    frames = (frames.to(torch.int16) + torch.randint(-6, 7, frames.shape, dtype=torch.int16, device="cuda", generator=gen)).clamp_(0, 255).to(torch.uint8)
    out = torch.empty_like(frames)
    jobs = (L.JpegJob * n)(*[L.JpegJob(i, q) for i in range(n)])
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)
    t, ts = timed(stream, lambda: check(lib.ssw_jpeg_rgb8(ctx.handle, C.c_void_p(frames.data_ptr()), n, w, h, jobs, n, C.c_void_p(out.data_ptr())), "jpeg"))
    moved = n * (2 * fb + 2 * (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)))
    host = frames.cpu().numpy()
    got0 = out[0].cpu().numpy()
    emit({"what": "jpeg", "shape": args.shape, "frames": n, "quality": q, "ms": round(t, 4), "ms_all": ts, "ms_per_frame": round(t / n, 5),
          "Mpix_per_s": round(n * w * h / t / 1e3, 1), "bytes_moved": moved, "GB_per_s": round(moved / t / 1e6, 1),
          "fraction_of_hbm_read": round(moved / (t * 1e-3) / HBM_READ, 3), "frame0_equals_pil": bool(np.array_equal(got0, pil_round_trip(host[0], q)))})
    del out
    torch.cuda.empty_cache()

    if not args.skip_pil:
        def wall(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        pil_round_trip(host[0], q)
        t1 = wall(lambda: [pil_round_trip(f, q) for f in host])
        with ThreadPoolExecutor(args.threads) as pool:
            list(pool.map(lambda f: pil_round_trip(f, q), host[:args.threads]))
            tn = wall(lambda: list(pool.map(lambda f: pil_round_trip(f, q), host)))
        emit({"what": "pil", "shape": args.shape, "frames": n, "quality": q, "one_thread_ms": round(t1, 1), "threads": args.threads,
              "threads_ms": round(tn, 1), "device_speedup_over_one_thread": round(t1 / t, 1), "device_speedup_over_threads": round(tn / t, 1)})
    del frames
    torch.cuda.empty_cache()

    if not args.skip_report:
        ctx.set_stream(None)
        img = synth_u8(ctx, lib, w, h, 0, 1)[0].cpu().numpy()
        alphas, qs = [0.02, 0.05, 0.1], (90, 75, 50, 25)

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

        t_plain = wall(lambda: api.strength_report(img, alphas, seed=3, ctx=ctx))
        t_jpeg = wall(lambda: api.strength_report(img, alphas, seed=3, jpeg=qs, ctx=ctx))
        rows = api.strength_report(img, alphas, seed=3, jpeg=qs, ctx=ctx)
        emit({"what": "strength_report", "shape": args.shape, "alphas": alphas, "copies": 8, "jpeg": list(qs), "ms": round(t_plain, 2),
              "with_jpeg_ms": round(t_jpeg, 2), "jpeg_frames": len(alphas) * 8 * len(qs),
              "survived": {str(r.alpha): [j.survived for j in r.jpeg] for r in rows},
              "weakest_own": {str(r.alpha): [round(j.weakest_own, 2) for j in r.jpeg] for r in rows}})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
