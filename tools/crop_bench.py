"""The crop rows' calls (ssw_crop_attack_rgb8, ssw_crop_search_attack_rgb8) against the same frames made of the entry points
there were before them, timed in one process.

    python tools/crop_bench.py [--shape 4k] [--copies 64] [--search-copies 8] [--json profiles/crop_bench.json]

Workload: N marked copies of one frame (ssw_fingerprint_embed_rgb8, k = 1000), one half-size centred crop of each.
(a) placed: one ssw_crop_attack_rgb8 call (crop_complement_kernel: one pass, no piece) against a strided device copy of every
    piece followed by ssw_restore_rgb8 -- the new call skips the pass that writes the pieces and the one that reads them back.
    Beside it a float4 copy of the same number of frames: the new call's share of that bandwidth, billed at 6 B per pixel.
(b) searched: one ssw_crop_search_attack_rgb8 call for the first --search-copies jobs against the strided copy, ssw_locate_rgb8
    and ssw_restore_rgb8.
Device events on the library's stream, a warm-up, then the median of 5 (3 for the search), the two routes alternating; the
results are compared.  Then a strength report (alpha 0.1, 8 copies) with three crops -- one placed, one searched, one scaled
and searched over 1800 .. 2040 -- against the report without them: host clock, a warm-up then the median of 3."""
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
from spread_spectrum_watermarking_amd.api import Context, Crop, check  # noqa: E402
from resample_bench import SHAPES, synth_u8  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4k")
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--search-copies", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    stream = torch.cuda.Stream()
    lib = L.load()
    w, h = SHAPES[args.shape]
    n, ns, k, fb = args.copies, min(args.search_copies, args.copies), 1000, w * h * 3
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    cfg = api.WriteConfig.default()._c()

    base = synth_u8(ctx, lib, w, h, 0, 1)[0]
    marks = torch.from_numpy(np.random.default_rng(5).standard_normal((n, k)).astype(np.float32)).cuda()
    copies = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    check(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), ptr(base), w, h, ptr(marks), n, k, ptr(copies), None), "ssw_fingerprint_embed_rgb8")
    ctx.synchronize()
    torch.cuda.synchronize()
    ctx.set_stream(stream.cuda_stream)

    crop = Crop(0.5)
    x, y, cw, ch = crop.rect_in(w, h)
    pb = cw * ch * 3
    jobs = (L.CropJob * n)(*[crop.job(c, w, h) for c in range(n)])
    out_a, out_b = (torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    pieces = torch.empty((n, ch, cw, 3), dtype=torch.uint8, device="cuda")
    piece_ptrs = (C.c_void_p * n)(*[pieces.data_ptr() + i * pb for i in range(n)])
    placed = (L.Placement * n)(*[L.Placement(cw, ch, 3, x, y, cw, ch) for _ in range(n)])

    def cut_pieces(m):
        with torch.cuda.stream(stream):
            pieces[:m].copy_(copies[:m, y:y + ch, x:x + cw])             # a strided device copy

    def new_placed():
        check(lib.ssw_crop_attack_rgb8(ctx.handle, ptr(base), ptr(copies), n, w, h, jobs, n, ptr(out_a), None), "ssw_crop_attack_rgb8")

    def old_placed():
        cut_pieces(n)
        check(lib.ssw_restore_rgb8(ctx.handle, ptr(base), w, h, piece_ptrs, placed, n, ptr(out_b)), "ssw_restore_rgb8")

    def float4_copy():
        with torch.cuda.stream(stream):
            out_b.view(-1).view(torch.float32).view(-1, 4).copy_(out_a.view(-1).view(torch.float32).view(-1, 4))

    searches = (L.CropSearch * ns)()
    found_a, found_b = (L.Placement * ns)(), (L.Placement * ns)(*[L.Placement(cw, ch, 3, 0, 0, 0, 0) for _ in range(ns)])
    sad_a, sad_b = np.zeros(ns, np.uint64), (C.c_uint64 * ns)()

    def new_searched():
        check(lib.ssw_crop_search_attack_rgb8(ctx.handle, ptr(base), ptr(copies), n, w, h, jobs, searches, ns, ptr(out_a), None, found_a, sad_a.ctypes.data),
              "ssw_crop_search_attack_rgb8")

    def old_searched():
        cut_pieces(ns)
        check(lib.ssw_locate_rgb8(ctx.handle, ptr(base), w, h, piece_ptrs, found_b, ns, sad_b), "ssw_locate_rgb8")
        back = (L.Placement * ns)(*[L.Placement(cw, ch, 3, f.x, f.y, cw, ch) for f in found_b])
        check(lib.ssw_restore_rgb8(ctx.handle, ptr(base), w, h, piece_ptrs, back, ns, ptr(out_b)), "ssw_restore_rgb8")

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def pair(new, old, reps, third=None):
        new(), old()
        if third:
            third()
        stream.synchronize()
        times = [[], [], []]
        for _ in range(reps):                                               # the routes alternate
            for t, fn in zip(times, (new, old, third)):
                if fn:
                    t.append(event_ms(fn))
        return times

    new_placed(), old_placed()
    stream.synchronize()
    same_placed = bool(torch.equal(out_a, out_b))
    t_new, t_old, t_copy = pair(new_placed, old_placed, args.reps, float4_copy)
    new_searched(), old_searched()
    stream.synchronize()
    same_searched = (bool(torch.equal(out_a[:ns], out_b[:ns])) and [(f.x, f.y) for f in found_a] == [(f.x, f.y) for f in found_b]
                     and sad_a.tolist() == list(sad_b))
    s_new, s_old, _ = pair(new_searched, old_searched, 3)
    ctx.set_stream(None)

    med = lambda v: float(np.median(v))
    spread = lambda v: [round(min(v), 3), round(max(v), 3)]
    copy_gbs = 2.0 * n * fb / (med(t_copy) * 1e-3) / 1e9
    new_gbs = 6.0 * n * w * h / (med(t_new) * 1e-3) / 1e9

    # the report: three crops against none
    image = base.cpu().numpy()
    three = [Crop(0.5), Crop(0.5, search=True), Crop(0.5, scale=0.5, search=(1800, 2040))]

    def report_ms(cr):
        t0 = time.perf_counter()
        rows = api.strength_report(image, [0.1], k=k, copies=8, seed=5, ctx=ctx, crops=cr)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, rows

    report_ms(three), report_ms([])
    with_ms, without_ms = [], []
    for _ in range(3):
        ms, rows = report_ms(three)
        with_ms.append(ms)
        without_ms.append(report_ms([])[0])

    def row(r):
        return {"crop": r.crop, "rect": list(r.rect), "thumb": r.thumb, "kept": round(r.kept, 4), "search": r.search, "found_exact": r.found_exact,
                "worst_offset": list(r.worst_offset), "worst_size_error": list(r.worst_size_error), "survived": r.survived, "accused": r.accused,
                "weakest_own": round(r.weakest_own, 2), "strongest_innocent": round(r.strongest_innocent, 2)}

    r = {"what": "crop attack, placed and searched", "shape": args.shape, "copies": n, "rect": [x, y, cw, ch],
         "placed_new_ms": round(med(t_new), 3), "placed_new_ms_spread": spread(t_new), "placed_new_ms_all": [round(v, 3) for v in t_new],
         "placed_copy_then_restore_ms": round(med(t_old), 3), "placed_copy_then_restore_ms_spread": spread(t_old),
         "placed_copy_then_restore_ms_all": [round(v, 3) for v in t_old], "placed_old_over_new": round(med(t_old) / med(t_new), 2), "placed_same_frames": same_placed,
         "float4_copy_ms": round(med(t_copy), 3), "float4_copy_gb_s": round(copy_gbs, 1), "placed_new_gb_s_at_6_bytes_per_pixel": round(new_gbs, 1),
         "placed_new_fraction_of_float4_copy": round(new_gbs / copy_gbs, 3),
         "searched_copies": ns, "searched_new_ms": round(med(s_new), 3), "searched_new_ms_all": [round(v, 3) for v in s_new],
         "searched_parts_ms": round(med(s_old), 3), "searched_parts_ms_all": [round(v, 3) for v in s_old], "searched_same_results": same_searched,
         "report_alpha_0.1_8_copies_ms": {"three_crops": round(med(with_ms), 1), "no_crops": round(med(without_ms), 1), "three_crops_all": [round(v, 1) for v in with_ms],
                                          "no_crops_all": [round(v, 1) for v in without_ms]},
         "report_rows": [row(x) for x in rows[-1].crops]}
    print(json.dumps(r), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(r, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
