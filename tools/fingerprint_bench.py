"""Fingerprinting throughput: ssw_fingerprint_embed(_rgb8) on one frame with N marks against ssw_batch_embed(_rgb8) on N
replicated frames with the same marks, timed in the same process with device events (median of 5 after a warm-up).

    python tools/fingerprint_bench.py [--shapes 4k,8k] [--copies 1,16,64] [--k 1000] [--json OUT]

Prints per (shape, format, N): the fingerprint call, the batch call, their ratio, R (distinct first-pass lines of the index
list) and the per-copy slope of the fingerprint call between the two largest N."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spread_spectrum_watermarking_amd import _lib as L  # noqa: E402
from spread_spectrum_watermarking_amd.api import Context, check  # noqa: E402

SHAPES = {"4k": (3840, 2160), "8k": (7680, 4320), "1080p": (1920, 1080)}


def timed(stream, fn, reps=5):
    """Median device time of fn() on `stream` (the library's stream: ssw_ctx_set_stream), events recorded around it."""
    fn()                                                   # warm-up (workspaces, bases)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4k,8k")
    ap.add_argument("--copies", default="1,16,64")
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--formats", default="u8,f32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)                     # the library enqueues on a torch stream: events time it directly
    lib = L.load()
    cfg = L.Config(L.ORDER_ENERGY, L.OPTION2, 0.1, L.PRECISION_F64)
    ns = [int(x) for x in args.copies.split(",")]
    results = []
    for shape in args.shapes.split(","):
        w, h = SHAPES[shape]
        n_max = max(ns)
        rgbf = torch.empty((n_max, h, w, 3), dtype=torch.float32, device="cuda")
        check(lib.ssw_synth_frames(ctx.handle, 7, 0, 1, w, h, C.c_void_p(rgbf.data_ptr())), "synth")
        ctx.synchronize()
        rgbf[1:] = rgbf[0]
        rgb8 = (rgbf[0:1].clamp(0, 1) * 255).round().to(torch.uint8).repeat(n_max, 1, 1, 1)
        torch.cuda.synchronize()                           # the library's stream reads what the default stream wrote
        marks = torch.from_numpy(np.random.default_rng(1).standard_normal((n_max, args.k)).astype(np.float32)).cuda()
        for fmt in args.formats.split(","):
            u8 = fmt == "u8"
            src = rgb8 if u8 else rgbf
            per = [src.new_empty((n, h, w, 3)) for n in ns]
            idx = torch.empty(args.k, dtype=torch.int32, device="cuda")
            row = []
            for n, out in zip(ns, per):
                def fp():
                    fn = lib.ssw_fingerprint_embed_rgb8 if u8 else lib.ssw_fingerprint_embed
                    check(fn(ctx.handle, C.byref(cfg), C.c_void_p(src.data_ptr()), w, h, C.c_void_p(marks.data_ptr()), n, args.k,
                             C.c_void_p(out.data_ptr()), C.c_void_p(idx.data_ptr())), "fingerprint")

                def batch():
                    if u8:
                        check(lib.ssw_batch_embed_rgb8(ctx.handle, C.byref(cfg), C.c_void_p(src.data_ptr()), n, w, h,
                                                       C.c_void_p(marks.data_ptr()), args.k, C.c_void_p(out.data_ptr())), "batch")
                    else:
                        check(lib.ssw_batch_embed(ctx.handle, C.byref(cfg), C.c_void_p(src.data_ptr()), n, w, h,
                                                  C.c_void_p(marks.data_ptr()), args.k, C.c_void_p(out.data_ptr()), None, None), "batch")
                t_fp = timed(stream, fp)
                t_b = timed(stream, batch)
                ix = idx.cpu().numpy().astype(np.int64)
                lines = ix // w if w >= h else ix % w
                r = {"shape": shape, "format": fmt, "n": n, "k": args.k, "R": int(np.unique(lines).size),
                     "fingerprint_ms": round(t_fp, 3), "batch_ms": round(t_b, 3), "speedup": round(t_b / t_fp, 2)}
                row.append(r)
                print(json.dumps(r), flush=True)
            if len(row) >= 2:
                a, b = row[-2], row[-1]
                slope = (b["fingerprint_ms"] - a["fingerprint_ms"]) / (b["n"] - a["n"]) * 1000.0
                print(json.dumps({"shape": shape, "format": fmt, "slope_us_per_copy": round(slope, 2),
                                  "between": [a["n"], b["n"]]}), flush=True)
                row.append({"shape": shape, "format": fmt, "slope_us_per_copy": round(slope, 2)})
            results += row
            del per
        del rgbf, rgb8
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
