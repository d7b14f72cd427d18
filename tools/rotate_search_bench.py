"""The unknown-angle row's call (ssw_rotate_search_attack_rgb8) against the same result made of the entry points there were before
it, timed in one process.

    python tools/rotate_search_bench.py [--shape 4k] [--copies 8] [--range 10] [--json profiles/rotate_search_bench.json]

Workload: N marked copies of one frame (ssw_fingerprint_embed_rgb8, k = 1000) under three rotations (0.5 and -1 degrees BICUBIC,
2 degrees BILINEAR), rotation-major: 3 N jobs, the angle searched over +---range degrees.
(a) the new entry: one ssw_rotate_search_attack_rgb8 call -- angle_cost_shared_kernel, the turned original made once per
    (tile, candidate) for the copies of a rotation.
(b) the same result of the parent's entry points: one ssw_affine_rgb8 per rotation, ONE ssw_find_angle_rgb8 call for the 3 N
    suspects (angle_cost_kernel, per suspect), ssw_unrotate_rgb8 with the angles found and ssw_unrotate_kept.
Device events on the library's stream, a warm-up, then the median of 5, the two routes alternating; the results are compared.
The search alone, (a) against (b), from the library's stage timers in a run of their own.  Then a strength report (3 alphas) with
the three rotations searched against the same report with them known: host clock, a warm-up then the median of 3."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from spread_spectrum_watermarking_amd import _lib as L  # noqa: E402
from spread_spectrum_watermarking_amd import api  # noqa: E402
from spread_spectrum_watermarking_amd.api import Context, Rotate, check  # noqa: E402
from resample_bench import SHAPES, synth_u8  # noqa: E402

ROTATIONS = [(0.5, "bicubic"), (-1.0, "bicubic"), (2.0, "bilinear")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4k")
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    lib = L.load()
    w, h = SHAPES[args.shape]
    n, k, fb = args.copies, 1000, w * h * 3
    m = n * len(ROTATIONS)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    cfg = api.WriteConfig.default()._c()

    base = synth_u8(ctx, lib, w, h, 0, 1)[0]
    marks = torch.from_numpy(np.random.default_rng(5).standard_normal((n, k)).astype(np.float32)).cuda()
    copies = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    check(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), ptr(base), w, h, ptr(marks), n, k, ptr(copies), None), "ssw_fingerprint_embed_rgb8")
    ctx.synchronize()
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)

    lo, hi = -args.range, args.range
    rotations = [Rotate(a, f) for a, f in ROTATIONS]
    jobs = (L.RotateJob * m)(*[r.job(c, w, h) for r in rotations for c in range(n)])
    out_a, out_b, turned_b = (torch.empty((m, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(3))
    found_a, found_b = (L.AngleFound * m)(), (L.AngleFound * m)()
    kept_a, kept_b = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
    fill = (C.c_uint8 * 3)(0, 0, 0)

    def new_route():
        check(lib.ssw_rotate_search_attack_rgb8(ctx.handle, ptr(base), ptr(copies), n, w, h, jobs, m, lo, hi, ptr(out_a), None, found_a, None,
                                                kept_a.ctypes.data), "ssw_rotate_search_attack_rgb8")

    def old_route():
        for i, r in enumerate(rotations):
            check(lib.ssw_affine_rgb8(ctx.handle, ptr(copies), n, w, h, w, h, jobs[i * n].forward, L.AFFINE_FILTERS[r.filter], fill, ptr(turned_b, i * n * fb)),
                  "ssw_affine_rgb8")
        check(lib.ssw_find_angle_rgb8(ctx.handle, ptr(base), ptr(turned_b), m, w, h, lo, hi, found_b, None), "ssw_find_angle_rgb8")
        undo = (L.RotateJob * m)(*[Rotate(f.n / L.ANGLE_PER_DEGREE).job(i, w, h) for i, f in enumerate(found_b)])
        check(lib.ssw_unrotate_rgb8(ctx.handle, ptr(base), ptr(turned_b), m, w, h, undo, ptr(out_b)), "ssw_unrotate_rgb8")
        check(lib.ssw_unrotate_kept(ctx.handle, w, h, undo, m, kept_b.ctypes.data), "ssw_unrotate_kept")

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    new_route()
    old_route()
    stream.synchronize()
    answers_a, answers_b = [(f.n, f.sad, f.count) for f in found_a], [(f.n, f.sad, f.count) for f in found_b]
    same = answers_a == answers_b and kept_a.tolist() == kept_b.tolist() and bool(torch.equal(out_a, out_b))
    new_ms, old_ms = [], []
    for _ in range(args.reps):                                              # the two routes alternate
        new_ms.append(event_ms(new_route))
        old_ms.append(event_ms(old_route))
    t_new, t_old = float(np.median(new_ms)), float(np.median(old_ms))

    # the search alone, from the library's own timers (a run of its own for each route)
    def stages(fn):
        ctx.enable_timing(True)
        ctx.reset_timing()
        fn()
        ctx.synchronize()
        t = ctx.timing()
        ctx.enable_timing(False)
        return {s: {"ms": round(t[s]["ms"], 3), "regions": t[s]["launches"]} for s in ("locate", "locate_coarse", "resize", "convert")}

    stages_new, stages_old = stages(new_route), stages(old_route)
    ctx.set_stream(None)

    # the report: three searched rotations against the same three known ones
    image = base.cpu().numpy()
    searched = [Rotate(a, f, (lo, hi)) for a, f in ROTATIONS]

    def report_ms(ro):
        t0 = time.perf_counter()
        rows = api.strength_report(image, [0.02, 0.05, 0.1], k=k, copies=n, seed=5, ctx=ctx, rotations=ro)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, rows

    report_ms(rotations), report_ms(searched)
    known_ms, searched_ms, none_ms = [], [], []
    for _ in range(3):
        known_ms.append(report_ms(rotations)[0])
        ms, rows = report_ms(searched)
        searched_ms.append(ms)
        none_ms.append(report_ms([])[0])
    known_rows = report_ms(rotations)[1]

    def row(r):
        return {"rotation": r.rotation, "kept": round(r.kept, 4), "found": [r.found_min, r.found_max] if r.search else None, "survived": r.survived,
                "accused": r.accused, "weakest_own": round(r.weakest_own, 2), "strongest_innocent": round(r.strongest_innocent, 2)}

    r = {"what": "rotation attack undone by the angle found", "shape": args.shape, "copies": n, "rotations": ROTATIONS, "jobs": m, "range": [lo, hi],
         "rungs": found_a[0].n_rungs,
         "new_entry_ms": round(t_new, 3), "new_entry_ms_all": [round(v, 3) for v in new_ms],
         "parent_entry_points_ms": round(t_old, 3), "parent_entry_points_ms_all": [round(v, 3) for v in old_ms],
         "parent_over_new": round(t_old / t_new, 2), "same_results": same,
         "library_timers_new": stages_new, "library_timers_parent_entry_points": stages_old,
         "search_ms_new_over_parent": [stages_new["locate"]["ms"], stages_old["locate"]["ms"]],
         "answers": [f[0] / L.ANGLE_PER_DEGREE for f in answers_a], "kept": [int(v) for v in kept_a],
         "report_3_alphas_ms": {"no_rotations": round(float(np.median(none_ms)), 1), "three_known": round(float(np.median(known_ms)), 1),
                                "three_searched": round(float(np.median(searched_ms)), 1), "known_all": [round(v, 1) for v in known_ms],
                                "searched_all": [round(v, 1) for v in searched_ms]},
         "report_rows_alpha_0.1": {"searched": [row(x) for x in rows[-1].rotations], "known": [row(x) for x in known_rows[-1].rotations]}}
    print(json.dumps(r), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
