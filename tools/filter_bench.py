"""Filter attack throughput (ssw_filter_rgb8, strength_report(filters=...)), timed in one process.

    python tools/filter_bench.py [--shape 4k] [--frames 64] [--threads 16] [--skip-pil] [--skip-report] [--json OUT]

1. N u8 frames under one filter in one call -- MEDIAN3, BLUR at radius 1 and at radius 8, UNSHARP(2, 150, 3): device events on the
   library's stream, a warm-up, then the median of 5.  The N frames and their N results (1.6 GB each at 4K and 64) are each far
   larger than the 256 MiB Infinity Cache and every call goes through all of them in order, so no call finds its input there.
   Reported: the time; the 6 B/px of the definition (a frame in, a frame out) and the bytes the kernels actually move (tile
   halos, the row-blurred plane out and in again, UNSHARP's second read of the frame) over that time, each as a fraction of the
   HBM read bandwidth (6.29 TB/s measured for a float4 copy, the figure tools/identify_bench.py uses); and whether frame 0 equals
   Pillow's filter byte for byte.
2. Pillow doing the same N filters on the host, on one thread and on --threads threads (its filters release the GIL).  The
   frames are on the host already; the two PCIe crossings per frame that the host route also needs are not counted.
3. One strength_report (3 alphas, 8 copies, the defaults) on one frame with and without four filters: host clock, a warm-up,
   then the median of 3."""
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
from spread_spectrum_watermarking_amd.api import Context, Filter, check  # noqa: E402

SHAPES = {"4k": (3840, 2160), "8k": (7680, 4320), "1080p": (1920, 1080), "cat": (640, 444)}
HBM_READ = 6.29e12                       # bytes / s, measured (float4 copy)
ROW_TILE, COL_TILE, MEDIAN_TILE = (256, 16), (64, 96), (64, 32)      # csrc/filter.hip: pixels x rows


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


def pil_filter(img, f):
    from PIL import Image, ImageFilter
    flt = {L.FILTER_BLUR: lambda: ImageFilter.GaussianBlur(f.radius), L.FILTER_UNSHARP: lambda: ImageFilter.UnsharpMask(f.radius, f.percent, f.threshold),
           L.FILTER_MEDIAN3: lambda: ImageFilter.MedianFilter(3)}[f.kind]()
    return np.asarray(Image.fromarray(img).filter(flt))


def box_radius(radius):
    """r of a blur's box passes (include/ssw.h); float64 is close enough for a byte count"""
    s2 = radius * radius / 3
    l = np.floor((np.sqrt(12 * s2 + 1) - 1) / 2)
    return int(l + (2 * l + 1) * (l * (l + 1) - 3 * s2) / (6 * (s2 - (l + 1) ** 2)))


def bytes_per_pixel(f):
    """what the kernels of csrc/filter.hip read and write per pixel of a large frame"""
    if f.kind == L.FILTER_MEDIAN3:
        return 3 * (MEDIAN_TILE[0] + 2) * (MEDIAN_TILE[1] + 2) / (MEDIAN_TILE[0] * MEDIAN_TILE[1]) + 3
    halo = 3 * (box_radius(f.radius) + 1)
    rows = 3 * (ROW_TILE[0] + halo + (halo + 3) // 4 * 4) / ROW_TILE[0] + 3
    cols = 3 * (COL_TILE[1] + 2 * halo) / COL_TILE[1] + 3
    return rows + cols + (3 if f.kind == L.FILTER_UNSHARP else 0)


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

    w, h = SHAPES[args.shape]
    fb, n = w * h * 3, args.frames
    frames = synth_u8(ctx, lib, w, h, 0, n)
    # a little noise on top: the generator's frames are smooth, and a median of a smooth frame changes next to nothing
    gen = torch.Generator(device="cuda").manual_seed(1)
    frames = (frames.to(torch.int16) + torch.randint(-6, 7, frames.shape, dtype=torch.int16, device="cuda", generator=gen)).clamp_(0, 255).to(torch.uint8)
    out = torch.empty_like(frames)
    host = frames.cpu().numpy()
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)
    for f in (Filter.median(), Filter.blur(1), Filter.blur(8), Filter.unsharp(2, 150, 3)):
        jobs = (L.FilterJob * n)(*[f.job(i) for i in range(n)])
        t, ts = timed(stream, lambda: check(lib.ssw_filter_rgb8(ctx.handle, C.c_void_p(frames.data_ptr()), n, w, h, jobs, n, C.c_void_p(out.data_ptr())), "filter"))
        moved = n * w * h * bytes_per_pixel(f)
        got0 = out[0].cpu().numpy()
        r = {"what": "filter", "filter": f.label, "shape": args.shape, "frames": n, "ms": round(t, 4), "ms_all": ts, "ms_per_frame": round(t / n, 5),
             "Mpix_per_s": round(n * w * h / t / 1e3, 1), "fraction_of_hbm_read_on_6_bytes_per_pixel": round(2 * n * fb / (t * 1e-3) / HBM_READ, 3),
             "bytes_per_pixel_moved": round(bytes_per_pixel(f), 2), "GB_per_s_moved": round(moved / t / 1e6, 1),
             "fraction_of_hbm_read_on_bytes_moved": round(moved / (t * 1e-3) / HBM_READ, 3),
             "frame0_equals_pillow": bool(np.array_equal(got0, pil_filter(host[0], f)))}
        if not args.skip_pil:
            pil_filter(host[0], f)
            t1 = wall_once(lambda: [pil_filter(im, f) for im in host])
            with ThreadPoolExecutor(args.threads) as pool:
                list(pool.map(lambda im: pil_filter(im, f), host[:args.threads]))
                tn = wall_once(lambda: list(pool.map(lambda im: pil_filter(im, f), host)))
            r.update({"pillow_one_thread_ms": round(t1, 1), "threads": args.threads, "pillow_threads_ms": round(tn, 1),
                      "device_speedup_over_one_thread": round(t1 / t, 1), "device_speedup_over_threads": round(tn / t, 1)})
        emit(r)
    del out, frames
    torch.cuda.empty_cache()

    if not args.skip_report:
        ctx.set_stream(None)
        img = synth_u8(ctx, lib, w, h, 0, 1)[0].cpu().numpy()
        alphas, fs = [0.02, 0.05, 0.1], [Filter.blur(1), Filter.blur(3), Filter.median(), Filter.unsharp()]

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
        t_filters = wall(lambda: api.strength_report(img, alphas, seed=3, filters=fs, ctx=ctx))
        rows = api.strength_report(img, alphas, seed=3, filters=fs, ctx=ctx)
        emit({"what": "strength_report", "shape": args.shape, "alphas": alphas, "copies": 8, "filters": [f.label for f in fs], "ms": round(t_plain, 2),
              "with_filters_ms": round(t_filters, 2), "filtered_frames": len(alphas) * 8 * len(fs),
              "survived": {str(r.alpha): [j.survived for j in r.filters] for r in rows},
              "weakest_own": {str(r.alpha): [round(j.weakest_own, 2) for j in r.filters] for r in rows}})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
