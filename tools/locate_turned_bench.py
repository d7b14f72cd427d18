"""The search for cut-outs of a turned copy (ssw_locate_turned_rgb8) against the same search done with what there was before it,
timed in one process.

    python tools/locate_turned_bench.py [--shape 4k] [--cut 1920x1080] [--copies 16] [--angle 1.3] [--range 10] [--old-suspects 2]
                                        [--reps 5] [--old-reps 5] [--old-budget-s 150] [--json profiles/locate_turned_bench.json]

Workload: N marked copies of one frame (ssw_fingerprint_embed_rgb8, k = 1000), each turned by --angle degrees as Pillow does it
(ssw_affine_rgb8, BICUBIC) and cropped to --cut at a position of its own inside the part the turn left whole, searched over
+---range degrees.
1. The search: one ssw_locate_turned_rgb8 call for all N.  Device events on the library's stream, a warm-up, then the median of
   --reps, alternating with (2).  The stage timers (the library's own event timers) come from a run of their own.
2. The same search with what the library offered before: per candidate angle one ssw_affine_rgb8 of the suspect turned back about
   its centre and one ssw_locate_rgb8 of its centred inscribed rectangle (the template's size), over the SAME rungs and then the
   SAME refinement candidates around the 4 best rungs, the best taken on the host -- on --old-suspects of the suspects, one at a
   time (it is slow; --old-reps runs of it).
3. How many suspects are found within 1/32 degree and one pixel of the truth."""
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
from spread_spectrum_watermarking_amd.api import Context, check  # noqa: E402
from resample_bench import SHAPES, synth_u8  # noqa: E402

STEP, KEEP, NEAR = 8, 4, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4k")
    ap.add_argument("--cut", default="1920x1080")
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--angle", type=float, default=1.3)
    ap.add_argument("--range", type=float, default=10.0)
    ap.add_argument("--old-suspects", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-reps", type=int, default=5)
    ap.add_argument("--old-budget-s", type=float, default=150.0, help="no further run of the old route once its runs have taken this long")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    lib = L.load()
    w, h = SHAPES[args.shape]
    cw, ch = (int(v) for v in args.cut.split("x"))
    n, k = args.copies, 1000
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cfg = api.WriteConfig.default()._c()
    black = (C.c_uint8 * 3)(0, 0, 0)

    base = synth_u8(ctx, lib, w, h, 0, 1)[0]
    marks = torch.from_numpy(np.random.default_rng(5).standard_normal((n, k)).astype(np.float32)).cuda()
    copies = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    turned = torch.empty_like(copies)
    check(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), ptr(base), w, h, ptr(marks), n, k, ptr(copies), None), "ssw_fingerprint_embed_rgb8")
    fwd = api.rotation_matrix(args.angle, w, h)
    check(lib.ssw_affine_rgb8(ctx.handle, ptr(copies), n, w, h, w, h, (C.c_double * 6)(*fwd), L.AFFINE_BICUBIC, black, ptr(turned)), "ssw_affine_rgb8")
    ctx.synchronize()
    # the cuts: spread over the part of the frame the turn left whole
    margin = int(np.ceil(max(w, h) * np.sin(np.radians(abs(args.angle))))) + 4
    rng = np.random.default_rng(9)
    at = [(int(rng.integers(margin, w - cw - margin + 1)), int(rng.integers(margin, h - ch - margin + 1))) for _ in range(n)]
    suspects = [turned[i, y:y + ch, x:x + cw].contiguous() for i, (x, y) in enumerate(at)]
    # where each cut's centre lay in the original: Pillow's matrix maps positions of the turned frame to the original's
    truth = [(fwd[0] * (x + cw / 2.0) + fwd[1] * (y + ch / 2.0) + fwd[2], fwd[3] * (x + cw / 2.0) + fwd[4] * (y + ch / 2.0) + fwd[5]) for x, y in at]
    del copies, turned
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)

    lo, hi = -args.range, args.range
    j0, j1 = int(np.floor(4 * lo)), int(np.ceil(4 * hi))
    n_rungs = j1 - j0 + 1
    found = (L.TurnedFound * n)()
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in suspects])
    shapes = (L.TurnedShape * n)(*[L.TurnedShape(cw, ch, 3) for _ in range(n)])

    def search():
        check(lib.ssw_locate_turned_rgb8(ctx.handle, ptr(base), w, h, ptrs, shapes, n, lo, hi, found, None), "ssw_locate_turned_rgb8")

    # the parent's route: a suspect turned back by every candidate, its centred rectangle searched for with ssw_locate_rgb8
    m_old = min(args.old_suspects, n)
    back = torch.empty((ch, cw, 3), dtype=torch.uint8, device="cuda")
    old_answers = []

    def template_size(a32):
        tw, th = C.c_uint32(0), C.c_uint32(0)
        check(lib.ssw_locate_turned_rung_boxes(ctx.handle, ptr(suspects[0]), cw, ch, a32, C.byref(tw), C.byref(th), None), "ssw_locate_turned_rung_boxes")
        return tw.value, th.value

    def old_cost(s, a32):
        """(mean luma difference, angle, x, y, tw, th) of suspect s turned back by a32 / 32 degrees"""
        tw, th = template_size(a32)
        m = (C.c_double * 6)(*api.rotation_matrix(-a32 / 32.0, cw, ch))
        check(lib.ssw_affine_rgb8(ctx.handle, ptr(suspects[s]), 1, cw, ch, cw, ch, m, L.AFFINE_BICUBIC, black, ptr(back)), "ssw_affine_rgb8")
        x0, y0 = (cw - tw) // 2, (ch - th) // 2
        with torch.cuda.stream(stream):                                 # (the copy goes where the library's calls go)
            t = back[y0:y0 + th, x0:x0 + tw].contiguous()
        pl = (L.Placement * 1)(L.Placement(tw, th, 3, 0, 0, tw, th))
        sad = (C.c_uint64 * 1)()
        check(lib.ssw_locate_rgb8(ctx.handle, ptr(base), w, h, (C.c_void_p * 1)(t.data_ptr()), pl, 1, sad), "ssw_locate_rgb8")
        return sad[0] / (tw * th), a32, int(pl[0].x), int(pl[0].y), tw, th

    def old_search():
        old_answers.clear()
        calls = 0
        for s in range(m_old):
            rungs = [old_cost(s, STEP * j) for j in range(j0, j1 + 1)]
            kept = sorted(range(n_rungs), key=lambda i: rungs[i][0])[:KEEP]
            cand = sorted({a for i in kept for a in range(STEP * (j0 + i) - NEAR, STEP * (j0 + i) + NEAR + 1) if STEP * j0 <= a <= STEP * j1})
            best = min(old_cost(s, a) for a in cand)
            old_answers.append({"angle": best[1] / 32.0, "centre": [best[2] + best[4] / 2.0, best[3] + best[5] / 2.0], "mean": round(best[0], 3)})
            calls += n_rungs + len(cand)
        return calls

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    search()
    old_cost(0, 0)
    stream.synchronize()
    print("warm-up of both paths done", flush=True)
    new_ms, old_ms, calls = [], [], 0
    for r in range(max(args.reps, args.old_reps)):                      # the two paths alternate
        if r < args.reps:
            new_ms.append(event_ms(search))
        if r < args.old_reps and sum(old_ms) < 1000.0 * args.old_budget_s:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            calls = old_search()
            b.record(stream)
            b.synchronize()
            old_ms.append(a.elapsed_time(b))
        print("rep", r, new_ms[-1:], old_ms[-1:], flush=True)
    t_new = float(np.median(new_ms))
    t_old = float(np.median(old_ms)) if old_ms else None

    # the stages, from the library's own timers (a run of its own)
    ctx.enable_timing(True)
    ctx.reset_timing()
    search()
    ctx.synchronize()
    t = ctx.timing()
    ctx.enable_timing(False)
    ctx.set_stream(None)

    answers = [{"angle": f.n / 32.0, "centre": [f.x + f.tw / 2.0, f.y + f.th / 2.0], "template": [f.tw, f.th], "mean": round(f.sad / (f.tw * f.th), 3)} for f in found]
    near = lambda a, tr: abs(a["angle"] - args.angle) <= 1 / 32 and abs(a["centre"][0] - tr[0]) <= 1.0 and abs(a["centre"][1] - tr[1]) <= 1.0
    r = {"what": "turned cut-out search", "shape": args.shape, "cut": [cw, ch], "suspects": n, "true_angle": args.angle, "range": [lo, hi], "rungs": n_rungs,
         "locate_turned_ms": round(t_new, 3), "locate_turned_ms_all": [round(v, 3) for v in new_ms], "per_suspect_ms": round(t_new / n, 3),
         "library_timers_ms": {s: round(t[s]["ms"], 3) for s in ("resize", "locate", "locate_coarse")},
         "library_timers_launches": {s: t[s]["launches"] for s in ("resize", "locate", "locate_coarse")},
         "found_within_1_32_degree_and_a_pixel": sum(near(a, tr) for a, tr in zip(answers, truth)),
         "answers": answers, "true_centres": [[round(v, 3) for v in tr] for tr in truth],
         "old_route": None if t_old is None else {
             "suspects": m_old, "calls_of_each_kind": calls, "ms": round(t_old, 1), "ms_all": [round(v, 1) for v in old_ms], "runs": len(old_ms),
             "per_suspect_ms": round(t_old / m_old, 1), "answers": old_answers,
             "found_within_1_32_degree_and_a_pixel": sum(near(a, tr) for a, tr in zip(old_answers, truth))},
         "old_route_per_suspect_over_locate_turned_per_suspect": None if t_old is None else round((t_old / m_old) / (t_new / n), 1)}
    print(json.dumps(r), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
