"""SSIM throughput (ssw_ssim_rgb8, strength_report(ssim=True)), timed in one process.

    python tools/ssim_bench.py [--shape 4k] [--copies 64] [--skip-torch] [--skip-report] [--json OUT]

1. N u8 copies against one original in one call: device events on the library's stream, a warm-up, then the median of 5.  The
   copies (1.6 GB at 4K and 64) are far larger than the 256 MiB Infinity Cache and every call goes through all of them in order,
   so no call finds its input there.  Reported: the time, the call's algorithmic bytes ((1 + N) 3 w h + 16 N) over that time, and
   that rate as a fraction of the HBM read bandwidth (6.29 TB/s measured for a float4 copy, the figure tools/identify_bench.py
   uses).  The same with a map.
2. The same frames through ssw_quality_rgb8: the same bytes through a kernel without windows, as the yardstick.
3. A torch formulation of the same sums: lumas as f64 planes, avg_pool2d (4 x 4, stride 4) for the cells and (2 x 2, stride 1)
   for the windows -- exact, every sum is an integer below 2^53 -- then the same f64 division; in groups of 8 copies.  Its sum
   per copy must equal the library's.
4. One strength_report (3 alphas, 8 copies, the defaults) on one frame with and without ssim=True: host clock, a warm-up, then the
   median of 3."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spread_spectrum_watermarking_amd import _lib as L  # noqa: E402
from spread_spectrum_watermarking_amd import api  # noqa: E402
from spread_spectrum_watermarking_amd.api import Context, check  # noqa: E402

SHAPES = {"4k": (3840, 2160), "8k": (7680, 4320), "1080p": (1920, 1080), "cat": (640, 444)}
HBM_READ = 6.29e12                       # bytes / s, measured (float4 copy)
TORCH_GROUP = 8


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


def synth_u8(ctx, lib, w, h, first, n):
    """n image-like 8-bit frames from the library's own generator, on the device"""
    f32, u8 = ctx.alloc(w * h * 12), torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for i in range(n):
        check(lib.ssw_synth_frames(ctx.handle, 7, first + i, 1, w, h, f32.ptr), "ssw_synth_frames")
        check(lib.ssw_convert_f32_to_rgb8(ctx.handle, f32.ptr, w * h * 3, C.c_void_p(u8[i].data_ptr())), "ssw_convert_f32_to_rgb8")
    ctx.synchronize()
    f32.free()
    return u8


def torch_luma(frames):
    p = frames.to(torch.int32)
    return ((77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8).to(torch.float64)


def torch_ssim_sums(base, copies):
    """the definition of include/ssw.h with avg_pool2d on f64 planes -> the sum of t per copy (int64)"""
    F = torch.nn.functional
    win = lambda x: F.avg_pool2d(F.avg_pool2d(x[:, None], 4, 4) * 16.0, 2, 1)[:, 0] * 4.0
    a = torch_luma(base)[None]
    out = []
    for g0 in range(0, copies.shape[0], TORCH_GROUP):
        b = torch_luma(copies[g0:g0 + TORCH_GROUP])
        s1, s2, ss, s12 = win(a), win(b), win(a * a + b * b), win(a * b)
        vars_, covar = 64.0 * ss - s1 * s1 - s2 * s2, 64.0 * s12 - s1 * s2
        q = ((2.0 * s1 * s2 + 416.0) * (2.0 * covar + 235963.0)) / ((s1 * s1 + s2 * s2 + 416.0) * (vars_ + 235963.0))
        out.append(torch.floor(q * float(L.SSIM_ONE) + 0.5).to(torch.int64).sum(dim=(1, 2)))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4k")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--skip-torch", action="store_true")
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
    fb, n = w * h * 3, args.copies
    nx, ny = w // 4 - 1, h // 4 - 1
    base = synth_u8(ctx, lib, w, h, 0, 1)[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    copies = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for i in range(n):                                      # what marked copies are: the original and a little noise, each its own
        copies[i] = (base.to(torch.int16) + torch.randint(-6, 7, base.shape, dtype=torch.int16, device="cuda", generator=gen)).clamp_(0, 255).to(torch.uint8)
    stats = torch.empty((n, L.SSIM_STATS), dtype=torch.int64, device="cuda")
    qstats = torch.empty((n, L.QUALITY_STATS), dtype=torch.int64, device="cuda")
    tmap = torch.empty((n, ny, nx), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def rate(what, t, ts, moved, **more):
        emit({"what": what, "shape": args.shape, "copies": n, "ms": round(t, 4), "ms_all": ts, "ms_per_copy": round(t / n, 5),
              "bytes_moved": moved, "GB_per_s": round(moved / t / 1e6, 1), "fraction_of_hbm_read": round(moved / (t * 1e-3) / HBM_READ, 3), **more})

    t, ts = timed(stream, lambda: check(lib.ssw_ssim_rgb8(ctx.handle, ptr(base), 1, ptr(copies), n, w, h, ptr(stats), None), "ssim"))
    sums = stats[:, 0].clone()
    rate("ssim", t, ts, (1 + n) * fb + 16 * n, mean_ssim=[round(float(s) / (L.SSIM_ONE * nx * ny), 6) for s in sums[:2].tolist()])
    t, ts = timed(stream, lambda: check(lib.ssw_ssim_rgb8(ctx.handle, ptr(base), 1, ptr(copies), n, w, h, ptr(stats), ptr(tmap)), "ssim"))
    rate("ssim_with_map", t, ts, (1 + n) * fb + 16 * n + 4 * nx * ny * n, map_sums_equal=bool(torch.equal(tmap.sum(dim=(1, 2), dtype=torch.int64), sums)))
    t, ts = timed(stream, lambda: check(lib.ssw_quality_rgb8(ctx.handle, ptr(base), 1, ptr(copies), n, w, h, ptr(qstats)), "quality"))
    rate("quality", t, ts, (1 + n) * fb + 48 * n)

    if not args.skip_torch:
        with torch.cuda.stream(stream):
            t, ts = timed(stream, lambda: torch_ssim_sums(base, copies))
            got = torch_ssim_sums(base, copies)
        stream.synchronize()
        emit({"what": "torch_avg_pool2d_f64", "shape": args.shape, "copies": n, "ms": round(t, 3), "ms_all": ts, "group": TORCH_GROUP,
              "equals_library": bool(torch.equal(got, sums)), "library_speedup": round(t / results[0]["ms"], 1)})
    del copies, tmap
    torch.cuda.empty_cache()

    if not args.skip_report:
        ctx.set_stream(None)
        img = base.cpu().numpy()
        alphas = [0.02, 0.05, 0.1]

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
        t_ssim = wall(lambda: api.strength_report(img, alphas, seed=3, ssim=True, ctx=ctx))
        rows = api.strength_report(img, alphas, seed=3, ssim=True, ctx=ctx)
        emit({"what": "strength_report", "shape": args.shape, "alphas": alphas, "copies": 8, "ms": round(t_plain, 2), "with_ssim_ms": round(t_ssim, 2),
              "ssim": {str(r.alpha): [round(min(s.mean for s in r.ssim), 5), round(max(s.mean for s in r.ssim), 5)] for r in rows},
              "worst_window": {str(r.alpha): round(min(s.worst_value for s in r.ssim), 4) for r in rows}})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
