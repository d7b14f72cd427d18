"""Strength-report throughput (ssw_quality_rgb8, ssw_collude_rgb8, strength_report), timed in one process with device events on
the library's stream (a warm-up, then the median of 5).

    python tools/collude_bench.py [--shape 4k] [--copies 64] [--pool 16] [--rotate 64] [--skip-report] [--json OUT]

1. Quality of N u8 copies against one original: time, its algorithmic bytes ((1 + N) w h 3 + 48 N) over that time as a fraction
   of the HBM read bandwidth (6.29 TB/s measured for a float4 copy, the figure tools/identify_bench.py uses), and the same
   arithmetic in torch on the same device -- per copy d = copy.int() - base.int(), (d * d).sum(dtype=int64) per channel, the luma
   the same way, (d != 0).sum(), d.abs().max().  The results of the two are compared exactly.
2. Collude: 24 coalitions (6 methods x the first c = 2, 4, 8, 16 of 16 copies) in one call: time, the sum of (c + 1) w h 3 bytes
   over that time as a fraction of the same bandwidth, and torch -- sum(dtype=int32) for AVERAGE, torch.sort along the members
   for MEDIAN / MIN / MAX / MINMAX, a gather through the tile map for MOSAIC.  Compared exactly.  Two fractions: of the
   algorithmic bytes (what the stage timer bills), and of the bytes that move at least once -- MOSAIC billed 2 frames, not
   c + 1, since it reads one member per pixel.  Either way the 16 copies are read by many coalitions of the call, so part
   of the traffic is cache-served.  Then every coalition alone, which tells the HBM-bound ones from a VALU-bound one: the
   members of successive calls rotate through --rotate frames (1.6 GB at 4K, far beyond the 256 MiB Infinity Cache), so no
   call finds its members in a cache.
3. One strength_report (3 alphas, the defaults) on one frame, host clock, beside the sum of its parts through the host wrappers
   (mark_copies_rgb8 + collude + quality + trace_many per alpha)."""
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
METHODS = list(L.COLLUDE_METHODS)


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
    return float(np.median(ts))


def torch_luma(x):
    return (77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8


def torch_quality(base, copies):
    """The same six values per copy in torch: int32 differences, int64 sums."""
    b = base.int()
    lb = torch_luma(b)
    out = torch.empty((copies.shape[0], 6), dtype=torch.int64, device=copies.device)
    for i in range(copies.shape[0]):
        c = copies[i].int()
        d = c - b
        dl = torch_luma(c) - lb
        out[i, 0:3] = (d * d).sum((0, 1), dtype=torch.int64)
        out[i, 3] = (dl * dl).sum(dtype=torch.int64)
        out[i, 4] = (d != 0).sum()
        out[i, 5] = d.abs().max()
    return out


def torch_collude(copies, method, c, tiles):
    v = copies[:c]
    if method == "average":
        return ((v.sum(0, dtype=torch.int32) + c // 2) // c).to(torch.uint8)
    if method == "mosaic":
        return torch.gather(v, 0, (tiles % c)[None, :, :, None].expand(1, -1, -1, 3))[0]
    s = torch.sort(v, dim=0).values.int()
    r = {"median": (s[(c - 1) // 2] + s[c // 2] + 1) >> 1, "min": s[0], "max": s[c - 1], "minmax": (s[0] + s[c - 1] + 1) >> 1}[method]
    return r.to(torch.uint8)


def synth_u8(ctx, lib, w, h):
    """One image-like 8-bit frame from the library's own generator (noise would give the transform nothing to rank)."""
    f32, u8 = ctx.alloc(w * h * 12), ctx.alloc(w * h * 3)
    check(lib.ssw_synth_frames(ctx.handle, 7, 0, 1, w, h, f32.ptr), "ssw_synth_frames")
    check(lib.ssw_convert_f32_to_rgb8(ctx.handle, f32.ptr, w * h * 3, u8.ptr), "ssw_convert_f32_to_rgb8")
    img = u8.to_host(np.uint8, (h, w, 3))
    f32.free(); u8.free()
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4k")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--rotate", type=int, default=64, help="frames the single-coalition timings rotate their members through")
    ap.add_argument("--skip-report", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    lib = L.load()
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    w, h = SHAPES[args.shape]
    fb = w * h * 3
    gen = torch.Generator(device="cuda").manual_seed(1)
    # copies that differ from their original by a little, as marked copies do
    base = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=gen)
    n = args.copies
    copies = (base[None].to(torch.int16) + torch.randint(-4, 5, (n, h, w, 3), dtype=torch.int16, device="cuda", generator=gen)).clamp_(0, 255).to(torch.uint8)
    stats = torch.empty((n, 6), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t = timed(stream, lambda: check(lib.ssw_quality_rgb8(ctx.handle, C.c_void_p(base.data_ptr()), 1, C.c_void_p(copies.data_ptr()), n, w, h,
                                                         C.c_void_p(stats.data_ptr())), "quality"))
    with torch.cuda.stream(stream):
        t_torch = timed(stream, lambda: torch_quality(base, copies), reps=3)
        ref = torch_quality(base, copies)
    stream.synchronize()
    moved = (1 + n) * fb + 48 * n
    emit({"what": "quality", "shape": args.shape, "copies": n, "ms": round(t, 4), "GB_per_s": round(moved / t / 1e6, 1),
          "fraction_of_hbm_read": round(moved / (t * 1e-3) / HBM_READ, 3), "torch_ms": round(t_torch, 3),
          "speedup_over_torch": round(t_torch / t, 1), "equal_torch": bool((ref == stats).all().item())})
    del copies, ref
    torch.cuda.empty_cache()

    n, nrot = args.pool, max(args.rotate, args.pool)
    rot = (base[None].to(torch.int16) + torch.randint(-4, 5, (nrot, h, w, 3), dtype=torch.int16, device="cuda", generator=gen)).clamp_(0, 255).to(torch.uint8)
    pool = rot[:n]
    plan = [(m, c) for m in METHODS for c in (2, 4, 8, 16) if c <= n]
    co = (L.Coalition * len(plan))(*[api._coalition(m, range(c), n) for m, c in plan])
    out = torch.empty((len(plan), h, w, 3), dtype=torch.uint8, device="cuda")
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    tiles = (xx >> 5) + (yy >> 5)
    torch.cuda.synchronize()
    t = timed(stream, lambda: check(lib.ssw_collude_rgb8(ctx.handle, C.c_void_p(pool.data_ptr()), n, w, h, co, len(plan), C.c_void_p(out.data_ptr())), "collude"))
    with torch.cuda.stream(stream):
        t_torch = timed(stream, lambda: [torch_collude(pool, m, c, tiles) for m, c in plan], reps=3)
        same = all(bool((torch_collude(pool, m, c, tiles) == out[i]).all().item()) for i, (m, c) in enumerate(plan))
    stream.synchronize()
    billed = sum(c + 1 for _, c in plan) * fb
    moved = sum(2 if m == "mosaic" else c + 1 for m, c in plan) * fb
    emit({"what": "collude", "shape": args.shape, "copies": n, "coalitions": len(plan), "ms": round(t, 4), "GB_per_s": round(billed / t / 1e6, 1),
          "fraction_of_hbm_read": round(billed / (t * 1e-3) / HBM_READ, 3), "fraction_mosaic_as_2_frames": round(moved / (t * 1e-3) / HBM_READ, 3),
          "torch_ms": round(t_torch, 3), "speedup_over_torch": round(t_torch / t, 1), "equal_torch": same})
    cursor = 0
    for i, (m, c) in enumerate(plan):
        # one descriptor per call of timed() (a warm-up + 5), made beforehand: c fresh frames each, the result in a fresh slot
        ones = []
        for _ in range(6):
            ones.append((L.Coalition * 1)(api._coalition(m, [(cursor + j) % nrot for j in range(c)], nrot)))
            cursor = (cursor + c) % nrot
        calls = iter(range(6))

        def one_call():
            r = next(calls)
            check(lib.ssw_collude_rgb8(ctx.handle, C.c_void_p(rot.data_ptr()), nrot, w, h, ones[r], 1, C.c_void_p(out[(i + r) % len(plan)].data_ptr())), "collude")

        t = timed(stream, one_call)
        emit({"what": "collude_one", "method": m, "count": c, "rotated_through_frames": nrot, "ms": round(t, 4),
              "fraction_of_hbm_read": round((2 if m == "mosaic" else c + 1) * fb / (t * 1e-3) / HBM_READ, 3)})
    del pool, rot, out, base
    torch.cuda.empty_cache()

    if not args.skip_report:
        ctx.set_stream(None)
        img = synth_u8(ctx, lib, w, h)
        alphas, k, copies, sizes = [0.02, 0.05, 0.1], 1000, 8, (2, 4)
        marks = np.random.default_rng(3).standard_normal((copies, k)).astype(np.float32)
        plan = [(m, range(c)) for m in METHODS for c in sizes]

        def report():
            return api.strength_report(img, alphas, seed=3, ctx=ctx)

        def parts():
            rows = []
            for a in alphas:
                cp = api.Writer(img, api.WriteConfig(insertion=api.Insertion.Option2(a)), ctx).mark_copies_rgb8(list(marks))
                forged = api.collude(cp, plan, ctx)
                q = api.quality(img, cp, ctx)
                tr = api.trace_many(img, forged, list(marks), config=api.ReadConfig(extraction=api.Extraction.Option2(a)), ctx=ctx)
                rows.append((q, tr.sims))
            return rows

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

        t_report, t_parts = wall(report), wall(parts)
        rows, ref = report(), parts()
        same = all(r.quality == q and all(c.weakest_colluder == float(s[i, :c.size].min()) for i, c in enumerate(r.collusions))
                   for r, (q, s) in zip(rows, ref))
        emit({"what": "strength_report", "shape": args.shape, "alphas": alphas, "copies": copies, "coalitions": len(plan),
              "ms": round(t_report, 2), "host_wrappers_ms": round(t_parts, 2), "speedup": round(t_parts / t_report, 2), "equal_parts": same,
              "psnr": [round(r.quality[0].psnr, 2) for r in rows],
              "found": {f"{c.method}/{c.size}": [r.collusions[i].found for r in rows] for i, c in enumerate(rows[0].collusions)}})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
