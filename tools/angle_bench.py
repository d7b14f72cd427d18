"""The angle search (ssw_find_angle_rgb8) against the same search done with what there was before it, timed in one process.

    python tools/angle_bench.py [--shape 4k] [--copies 16] [--angle 1.3] [--range 10] [--old-suspects 2] [--json profiles/angle_bench.json]

Workload: N marked copies of one frame (ssw_fingerprint_embed_rgb8, k = 1000), each turned by --angle degrees as Pillow does it
(ssw_affine_rgb8, BICUBIC), searched over +---range degrees.
1. The search: one ssw_find_angle_rgb8 call for all N.  Device events on the library's stream, a warm-up, then the median of 5,
   alternating with (2).  The share of the ladder is what the call bills to SSW_STAGE_LOCATE_COARSE of what it bills to
   SSW_STAGE_LOCATE (the library's own event timers, a run of its own); the rest is the planes, the refinement and the two
   small kernels.
2. The same search with what the library offered before: per candidate angle one ssw_unrotate_rgb8 and one ssw_quality_rgb8
   (the luma SSE), over the SAME rungs and then the SAME refinement candidates around the 4 best rungs, the best taken on the
   host -- on --old-suspects of the suspects (it is slow).
3. What each suspect's answer is against the truth, and the similarity ssw_fingerprint_trace_rgb8 gives a copy turned back by
   the angle found beside the one it gives with the true angle."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from spread_spectrum_watermarking_amd import _lib as L  # noqa: E402
from spread_spectrum_watermarking_amd import api  # noqa: E402
from spread_spectrum_watermarking_amd.api import Context, Rotate, check  # noqa: E402
from resample_bench import SHAPES, synth_u8  # noqa: E402

STEP, KEEP, NEAR = 8, 4, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4k")
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--angle", type=float, default=1.3)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--old-suspects", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    lib = L.load()
    w, h = SHAPES[args.shape]
    n, k, fb = args.copies, 1000, w * h * 3
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cfg = api.WriteConfig.default()._c()

    base = synth_u8(ctx, lib, w, h, 0, 1)[0]
    marks = torch.from_numpy(np.random.default_rng(5).standard_normal((n, k)).astype(np.float32)).cuda()
    copies = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    suspects = torch.empty_like(copies)
    check(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), ptr(base), w, h, ptr(marks), n, k, ptr(copies), None), "ssw_fingerprint_embed_rgb8")
    m = (C.c_double * 6)(*api.rotation_matrix(args.angle, w, h))
    check(lib.ssw_affine_rgb8(ctx.handle, ptr(copies), n, w, h, w, h, m, L.AFFINE_BICUBIC, (C.c_uint8 * 3)(0, 0, 0), ptr(suspects)), "ssw_affine_rgb8")
    ctx.synchronize()
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)

    lo, hi = -args.range, args.range
    j0, j1 = int(np.floor(4 * lo)), int(np.ceil(4 * hi))
    n_rungs = j1 - j0 + 1
    found = (L.AngleFound * n)()

    def search():
        check(lib.ssw_find_angle_rgb8(ctx.handle, ptr(base), ptr(suspects), n, w, h, lo, hi, found, None), "ssw_find_angle_rgb8")

    # the parent's route: one suspect turned back by every candidate and compared with the original
    m_old = min(args.old_suspects, n)
    undone = torch.empty((m_old, h, w, 3), dtype=torch.uint8, device="cuda")
    stats = torch.zeros((m_old, L.QUALITY_STATS), dtype=torch.int64, device="cuda")
    old_answers, old_candidates = [], []

    def luma_sse(a32):
        """per suspect of the first m_old: the luma SSE of the suspect turned back by a32 / 32 degrees against the original"""
        jobs = (L.RotateJob * m_old)(*[Rotate(a32 / 32.0).job(i, w, h) for i in range(m_old)])
        check(lib.ssw_unrotate_rgb8(ctx.handle, ptr(base), ptr(suspects), m_old, w, h, jobs, ptr(undone)), "ssw_unrotate_rgb8")
        check(lib.ssw_quality_rgb8(ctx.handle, ptr(base), 1, ptr(undone), m_old, w, h, ptr(stats)), "ssw_quality_rgb8")
        stream.synchronize()                                                # (the best is taken on the host)
        return stats[:, 3].cpu().numpy().astype(np.float64)

    def old_search():
        rungs = np.stack([luma_sse(STEP * j) for j in range(j0, j1 + 1)])   # [rung][suspect]
        old_answers.clear()
        old_candidates.clear()
        for s in range(m_old):
            kept = np.argsort(rungs[:, s], kind="stable")[:KEEP]
            cand = sorted({a for i in kept for a in range(STEP * (j0 + int(i)) - NEAR, STEP * (j0 + int(i)) + NEAR + 1) if STEP * j0 <= a <= STEP * j1})
            old_candidates.append(len(cand))
        # every suspect's candidates in one sweep over their union: the calls take all m_old suspects at a time
        union = sorted({a for s in range(m_old) for i in np.argsort(rungs[:, s], kind="stable")[:KEEP]
                        for a in range(STEP * (j0 + int(i)) - NEAR, STEP * (j0 + int(i)) + NEAR + 1) if STEP * j0 <= a <= STEP * j1})
        fine = np.stack([luma_sse(a) for a in union])
        for s in range(m_old):
            old_answers.append(union[int(np.argmin(fine[:, s]))] / 32.0)
        return n_rungs + len(union)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    search()
    calls = old_search()
    stream.synchronize()
    new_ms, old_ms = [], []
    for _ in range(args.reps):                                              # the two paths alternate
        new_ms.append(event_ms(search))
        old_ms.append(event_ms(old_search))
    t_new, t_old = float(np.median(new_ms)), float(np.median(old_ms))

    # the shares, from the library's own timers (a run of its own)
    ctx.enable_timing(True)
    ctx.reset_timing()
    search()
    ctx.synchronize()
    t = ctx.timing()
    ctx.enable_timing(False)
    ladder, total = t["locate_coarse"]["ms"], t["locate"]["ms"]

    answers = [f.n / 32.0 for f in found]
    means = [f.sad / max(1, f.count) for f in found]

    # what trace makes of a copy turned back by the angle found, beside the true angle
    def similarities(angles):
        jobs = (L.RotateJob * n)(*[Rotate(a).job(i, w, h) for i, a in enumerate(angles)])
        back = torch.empty_like(suspects)
        check(lib.ssw_unrotate_rgb8(ctx.handle, ptr(base), ptr(suspects), n, w, h, jobs, ptr(back)), "ssw_unrotate_rgb8")
        ext = torch.empty((n, k), dtype=torch.float32, device="cuda")
        sims = torch.empty((n, n), dtype=torch.float32, device="cuda")
        best = torch.empty(n, dtype=torch.int32, device="cuda")
        best_sim = torch.empty(n, dtype=torch.float32, device="cuda")
        n_exceed = torch.empty(n, dtype=torch.int32, device="cuda")
        check(lib.ssw_fingerprint_trace_rgb8(ctx.handle, C.byref(cfg), ptr(base), ptr(back), n, w, h, k, ptr(marks), n, C.c_float(6.0), ptr(ext), ptr(sims),
                                             ptr(best), ptr(best_sim), ptr(n_exceed)), "ssw_fingerprint_trace_rgb8")
        ctx.synchronize()
        return [round(float(v), 2) for v in best_sim.cpu().numpy()], [int(v) for v in best.cpu().numpy()]

    sim_found, best_found = similarities(answers)
    sim_true, best_true = similarities([args.angle] * n)
    ctx.set_stream(None)

    r = {"what": "angle search", "shape": args.shape, "suspects": n, "true_angle": args.angle, "range": [lo, hi], "rungs": n_rungs,
         "find_angle_ms": round(t_new, 3), "find_angle_ms_all": [round(v, 3) for v in new_ms], "per_suspect_ms": round(t_new / n, 3),
         "library_timers": {"locate_ms": round(total, 3), "ladder_ms": round(ladder, 3), "ladder_share": round(ladder / total, 3),
                            "planes_refinement_and_rest_share": round(1 - ladder / total, 3)},
         "old_route": {"suspects": m_old, "candidates": calls, "refined_per_suspect": old_candidates, "ms": round(t_old, 1), "ms_all": [round(v, 1) for v in old_ms],
                       "per_suspect_ms": round(t_old / m_old, 1), "answers": old_answers},
         "old_route_per_suspect_over_find_angle_per_suspect": round((t_old / m_old) / (t_new / n), 1),
         "answers": answers, "mean_luma_difference": [round(v, 3) for v in means], "nearest_grid_angle": round(args.angle * 32) / 32,
         "similarity_with_found_angle": sim_found, "similarity_with_true_angle": sim_true,
         "named_right_with_found_angle": best_found == list(range(n)), "named_right_with_true_angle": best_true == list(range(n))}
    print(json.dumps(r), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
