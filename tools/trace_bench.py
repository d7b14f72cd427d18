"""Tracing throughput: ssw_fingerprint_trace_rgb8 (ONE base frame, S resident suspects, M stored marks) against what the same
question cost before it -- ssw_batch_extract_rgb8 with the base replicated S times, then ssw_similarity_matrix -- timed in the
same process with device events, the two forms alternating, median of 5 after a warm-up; then one pass of each with the
library's stage timers on (per-stage milliseconds; the compact column pass is what `dct_col` holds in the trace call).

    python tools/trace_bench.py [--cases 4k:128:1000:1024,4k:16:1000:1024,8k:32:10000:1024] [--json OUT]

A case is shape:S:k:M.  Prints one JSON line per case."""
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


def once(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stages(ctx, stream, fn):
    """Per-stage milliseconds of one fn() with the library's timers on (only the stages that ran)."""
    ctx.enable_timing(True)
    ctx.reset_timing()
    fn()
    stream.synchronize()
    t = ctx.timing()
    ctx.enable_timing(False)
    return {s: round(v["ms"], 3) for s, v in t.items() if v["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="4k:128:1000:1024,4k:16:1000:1024,8k:32:10000:1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)                     # the library enqueues on a torch stream: events time it directly
    lib = L.load()
    cfg = L.Config(L.ORDER_ENERGY, L.OPTION2, 0.1, L.PRECISION_F64)
    p = lambda t: C.c_void_p(t.data_ptr())
    results = []
    for case in args.cases.split(","):
        shape, S, k, M = case.split(":")
        S, k, M = int(S), int(k), int(M)
        w, h = SHAPES[shape]
        f32 = torch.empty((1, h, w, 3), dtype=torch.float32, device="cuda")
        check(lib.ssw_synth_frames(ctx.handle, 7, 0, 1, w, h, p(f32)), "synth")
        ctx.synchronize()
        base = (f32[0].clamp(0, 1) * 255).round().to(torch.uint8).contiguous()
        del f32
        marks = torch.from_numpy(np.random.default_rng(1).standard_normal((max(M, S), k)).astype(np.float32)).cuda()
        suspects = torch.empty((S, h, w, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                           # the library's stream reads what the default stream wrote
        # suspect s carries mark s: the copies ssw_fingerprint_embed_rgb8 hands out
        check(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), p(base), w, h, p(marks), S, k, p(suspects), None), "fingerprint")
        ctx.synchronize()
        replicated = base[None].repeat(S, 1, 1, 1)
        ext = torch.empty((S, k), dtype=torch.float32, device="cuda")
        sims = torch.empty((S, M), dtype=torch.float32, device="cuda")
        best = torch.empty(S, dtype=torch.int32, device="cuda")
        best_sim = torch.empty(S, dtype=torch.float32, device="cuda")
        n_exceed = torch.empty(S, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def trace():
            check(lib.ssw_fingerprint_trace_rgb8(ctx.handle, C.byref(cfg), p(base), p(suspects), S, w, h, k, p(marks), M, C.c_float(6.0),
                                                 p(ext), p(sims), p(best), p(best_sim), p(n_exceed)), "trace")

        def pairs():
            check(lib.ssw_batch_extract_rgb8(ctx.handle, C.byref(cfg), p(replicated), p(suspects), S, w, h, k, p(ext), None, None), "batch_extract")
            check(lib.ssw_similarity_matrix(ctx.handle, p(ext), S, p(marks), M, k, p(sims)), "similarity_matrix")

        trace(); pairs(); stream.synchronize()             # warm-up: workspaces, bases
        t_trace, t_pairs = [], []
        for _ in range(args.reps):                         # alternating
            t_trace.append(once(stream, trace))
            t_pairs.append(once(stream, pairs))
        found = int((best.cpu().numpy()[:min(S, M)] == np.arange(min(S, M))).sum())
        st_trace, st_pairs = stages(ctx, stream, trace), stages(ctx, stream, pairs)
        mt, mp = float(np.median(t_trace)), float(np.median(t_pairs))
        r = {"shape": shape, "suspects": S, "k": k, "marks": M, "trace_ms": round(mt, 3), "replicated_ms": round(mp, 3),
             "speedup": round(mp / mt, 2), "trace_all_ms": [round(x, 3) for x in t_trace], "replicated_all_ms": [round(x, 3) for x in t_pairs],
             "suspects_named": found, "prune": ctx.prune_stats(), "trace_stages_ms": st_trace, "replicated_stages_ms": st_pairs,
             "compact_column_share": round(st_trace.get("dct_col", 0.0) / max(sum(v for s, v in st_trace.items() if not s.endswith("_main")), 1e-9), 3)}
        results.append(r)
        print(json.dumps(r), flush=True)
        del suspects, replicated, ext, sims
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
