"""Catalogue search throughput (ssw_signature_rgb8, ssw_signature_match), timed in one process with device events on the
library's stream (a warm-up, then the median of 5).

    python tools/identify_bench.py [--frames 128] [--shape 4k] [--queries 128] [--entries 100000,1000000] [--json OUT]

1. Signatures of N u8 frames: time and the fraction of the HBM read bandwidth (6.29 TB/s measured for a float4 copy) that
   w h 3 bytes per frame amount to.
2. Match of Q queries against each catalogue size, top = 8: time, against the torch formulation of the same sums on the same
   device -- chunked (q[:, None].int() - c[None].int()).abs().sum(-1), then topk -- and against the v_sad_u8 issue bound
   Q nc 256 / (256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz).  The answers of the two are compared: distances exactly; indices too, but torch.topk
   does not order tied distances by index, so that comparison can read false where distances tie (exact indices are checked
   against numpy by tests/test_identify_gpu.py)."""
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
HBM_READ = 6.29e12                       # bytes / s, measured (float4 copy)
SAD_LANES_PER_S = 256 * 4 * 32 * 2.4e9   # one v_sad_u8 per lane: a wave64 instruction issues over 2 cycles on a SIMD-32


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


def torch_match(q, c, top, chunk=2048):
    """The same sums in torch: distances of every query against catalogue chunks, a running top-k of (distance, index)."""
    best_d = torch.full((q.shape[0], 0), 0, dtype=torch.int32, device=q.device)
    best_i = torch.full((q.shape[0], 0), 0, dtype=torch.int64, device=q.device)
    qi = q[:, None].int()
    for c0 in range(0, c.shape[0], chunk):
        d = (qi - c[None, c0:c0 + chunk].int()).abs().sum(-1, dtype=torch.int32)
        i = torch.arange(c0, c0 + d.shape[1], device=q.device)[None].expand_as(d)
        best_d, best_i = torch.cat([best_d, d], 1), torch.cat([best_i, i], 1)
        k = min(top, best_d.shape[1])
        best_d, sel = torch.topk(best_d, k, dim=1, largest=False, sorted=True)
        best_i = torch.gather(best_i, 1, sel)
    return best_d, best_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--shape", default="4k")
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--entries", default="100000,1000000")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    lib = L.load()
    results = []

    w, h = SHAPES[args.shape]
    n = args.frames
    gen = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=gen)
    sigs = torch.empty((n, 1024), dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * n)(*[frames[i].data_ptr() for i in range(n)])
    shapes = (L.ImageShape * n)(*[L.ImageShape(w, h, 3)] * n)
    torch.cuda.synchronize()
    for count in sorted({1, n}):
        t = timed(stream, lambda: check(lib.ssw_signature_rgb8(ctx.handle, ptrs, shapes, count, C.c_void_p(sigs.data_ptr())), "signature"))
        read = count * w * h * 3
        r = {"what": "signature", "shape": args.shape, "frames": count, "ms": round(t, 4), "read_GB_per_s": round(read / t / 1e6, 1),
             "fraction_of_hbm_read": round(read / (t * 1e-3) / HBM_READ, 3)}
        results.append(r)
        print(json.dumps(r), flush=True)
    del frames
    torch.cuda.empty_cache()

    nq, top = args.queries, 8
    for nc in [int(x) for x in args.entries.split(",")]:
        cat = torch.randint(0, 256, (nc, 1024), dtype=torch.uint8, device="cuda", generator=gen)
        q = torch.randint(0, 256, (nq, 1024), dtype=torch.uint8, device="cuda", generator=gen)
        pick = torch.randint(0, nc, (nq,), device="cuda", generator=gen)
        q[: nq // 2] = cat[pick[: nq // 2]]                                    # half of the queries have an exact copy
        idx = torch.empty((nq, top), dtype=torch.int32, device="cuda")
        dst = torch.empty((nq, top), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t = timed(stream, lambda: check(lib.ssw_signature_match(ctx.handle, C.c_void_p(q.data_ptr()), nq, C.c_void_p(cat.data_ptr()), nc, top,
                                                                C.c_void_p(idx.data_ptr()), C.c_void_p(dst.data_ptr()), None), "match"))
        with torch.cuda.stream(stream):
            t_torch = timed(stream, lambda: torch_match(q, cat, top), reps=1 if nc > 200000 else 3)
            td, ti = torch_match(q, cat, top)
        stream.synchronize()
        same_d = bool((td == dst).all().item())
        clear = td[:, -1:] != td                                               # a slot whose distance differs from the last one's is not a boundary tie
        same_i = bool(((ti == idx.long()) | ~clear).all().item())
        bound = nq * nc * 256 / SAD_LANES_PER_S * 1e3
        r = {"what": "match", "queries": nq, "entries": nc, "top": top, "ms": round(t, 3), "torch_ms": round(t_torch, 3),
             "speedup_over_torch": round(t_torch / t, 1), "sad_issue_bound_ms": round(bound, 3), "fraction_of_issue_bound": round(bound / t, 3),
             "catalogue_GB_per_s": round(nc * 1024 / t / 1e6, 1), "distances_equal_torch": same_d, "indices_equal_torch": same_i}
        results.append(r)
        print(json.dumps(r), flush=True)
        del cat, q
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
