"""Locating cut-outs of unknown scale (ssw_locate_scaled_rgb8) on one GPU against what the library could do before it:
16 cut-outs of 1920 x 1080, each from its own marked 4K copy at its own (odd) position, halved to 960 x 540; the finder only
knows that the cut-out was between 960 and 3840 wide in the original.

Reported (device events around each call, median of 5 after one warm-up call each, the two paths alternating):
  scaled           ssw_locate_scaled_rgb8, width range 960..3840: ms per call and per suspect, and from the stage timers (a
                   second set of 5 timed calls) the shares of SSW_STAGE_RESIZE (rung tiles + the refinement's resizes),
                   SSW_STAGE_LOCATE_COARSE (both coarse searches) and the rest of SSW_STAGE_LOCATE; what is left of the wall
                   time is the host (tap tables, the choice of rungs) and the two waits.  The stage timers do not separate
                   ladder from refinement.
  per width        the parent's capability: ssw_locate_rgb8 given one entry per rung width of the same ladder (361 entries per
                   suspect), best mean SAD taken on the host.  Fewer widths than an exhaustive search over 960..3840 would
                   take, so the ratio is conservative.  Run on --baseline-suspects of the 16 (default 2): ms per suspect.
  found            how many suspects each path put within one pixel of the truth in width, x and y

    python tools/locate_scale_bench.py [--out profiles/locate_scale_bench_4k.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import spread_spectrum_watermarking_amd as wm  # noqa: E402
from spread_spectrum_watermarking_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--suspects", type=int, default=16)
    ap.add_argument("--baseline-suspects", type=int, default=2)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_scale_bench_4k.json"))
    a = ap.parse_args()
    W, H, S, k = 3840, 2160, a.suspects, a.k
    cw, ch, sw, sh, wmin, wmax = W // 2, H // 2, W // 4, H // 4, W // 4, W
    B = min(a.baseline_suspects, S)
    ctx = wm.Context(0)
    lib, chk = ctx._lib, L.check
    cfg = L.Config()
    lib.ssw_config_default(C.byref(cfg))
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(1)
    marks = torch.from_numpy(rng.standard_normal((S, k)).astype(np.float32)).to(dev)
    where = [(int(rng.integers(0, (W - cw) // 2)) * 2 + 1, int(rng.integers(0, (H - ch) // 2)) * 2 + 1) for _ in range(S)]
    with torch.cuda.stream(stream):
        base_f = torch.empty((1, H, W, 3), dtype=torch.float32, device=dev)
        chk(lib.ssw_synth_frames(ctx.handle, 7, 0, 1, W, H, base_f.data_ptr()))
        base = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        chk(lib.ssw_convert_f32_to_rgb8(ctx.handle, base_f.data_ptr(), base_f.numel(), base.data_ptr()))
        del base_f
        copies = torch.empty((S, H, W, 3), dtype=torch.uint8, device=dev)
        chk(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), base.data_ptr(), W, H, marks.data_ptr(), S, k, copies.data_ptr(), None))
        stream.synchronize()
        cuts = torch.stack([copies[i, y:y + ch, x:x + cw] for i, (x, y) in enumerate(where)]).contiguous()
        del copies
        small = torch.empty((S, sh, sw, 3), dtype=torch.uint8, device=dev)
        chk(lib.ssw_resize_rgb8(ctx.handle, cuts.data_ptr(), S, cw, ch, sw, sh, small.data_ptr()))
    stream.synchronize()
    del cuts
    ptrs = (C.c_void_p * S)(*[small[i].data_ptr() for i in range(S)])
    pl = (L.Placement * S)(*[L.Placement(sw, sh, 3, 0, 0, 0, 0) for _ in range(S)])
    rg = (L.ScaleRange * S)(*[L.ScaleRange(wmin, wmax) for _ in range(S)])
    sad = (C.c_uint64 * S)()
    rungs = list(range(wmin, wmax + 1, 8))
    heights = [max(1, (2 * sh * pw + sw) // (2 * sw)) for pw in rungs]
    nb = B * len(rungs)
    bptrs = (C.c_void_p * nb)(*[small[i].data_ptr() for i in range(B) for _ in rungs])
    bpl = (L.Placement * nb)(*[L.Placement(sw, sh, 3, 0, 0, pw, ph) for _ in range(B) for pw, ph in zip(rungs, heights)])
    bsad = (C.c_uint64 * nb)()

    def scaled():
        chk(lib.ssw_locate_scaled_rgb8(ctx.handle, base.data_ptr(), W, H, ptrs, pl, rg, S, sad), "ssw_locate_scaled_rgb8")

    def per_width():
        chk(lib.ssw_locate_rgb8(ctx.handle, base.data_ptr(), W, H, bptrs, bpl, nb, bsad), "ssw_locate_rgb8")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    timed(scaled), timed(per_width)                  # warm-up: workspace, cached tap tables
    t_scaled, t_width = [], []
    for _ in range(a.repeats):
        t_scaled.append(timed(scaled))
        t_width.append(timed(per_width))
    near = lambda pw, x, y, xy: abs(pw - cw) <= 1 and abs(x - xy[0]) <= 1 and abs(y - xy[1]) <= 1
    found = sum(near(p.pw, p.x, p.y, xy) for p, xy in zip(pl, where))
    exact = sum((p.pw, p.ph, p.x, p.y) == (cw, ch) + xy for p, xy in zip(pl, where))
    bfound = 0
    for i in range(B):
        j = min(range(len(rungs)), key=lambda j: (bsad[i * len(rungs) + j] / (rungs[j] * heights[j]), j))
        p = bpl[i * len(rungs) + j]
        bfound += near(p.pw, p.x, p.y, where[i])
    stages = {"resize": [], "locate_coarse": [], "locate": []}
    ctx.enable_timing(True)
    for _ in range(a.repeats):
        ctx.reset_timing()
        scaled()
        t = ctx.timing()
        for name in stages:
            stages[name].append(t[name]["ms"])
    ctx.enable_timing(False)
    med = lambda v: float(np.median(v))
    s_ms, w_ms = med(t_scaled), med(t_width)
    r_ms, c_ms, l_ms = med(stages["resize"]), med(stages["locate_coarse"]), med(stages["locate"])
    res = {
        "gpu": torch.cuda.get_device_name(0), "frame": [W, H], "cut_out": [cw, ch], "suspect": [sw, sh], "widths": [wmin, wmax],
        "rungs": len(rungs), "suspects": S, "repeats": a.repeats,
        "scaled_call_ms": t_scaled, "scaled_median_ms": s_ms, "scaled_ms_per_suspect": s_ms / S,
        "scaled_stage_ms": {"resize": r_ms, "locate_coarse": c_ms, "locate_other": l_ms - c_ms},
        "scaled_stage_share_of_call": {"resize": r_ms / s_ms, "locate_coarse": c_ms / s_ms, "locate_other": (l_ms - c_ms) / s_ms,
                                       "host_and_waits": max(0.0, 1.0 - (r_ms + l_ms) / s_ms)},
        "per_width_suspects": B, "per_width_entries_per_suspect": len(rungs),
        "per_width_call_ms": t_width, "per_width_median_ms": w_ms, "per_width_ms_per_suspect": w_ms / B,
        "per_width_over_scaled_per_suspect": (w_ms / B) / (s_ms / S),
        "scaled_found_within_one_pixel": int(found), "scaled_found_exactly": int(exact), "per_width_found_within_one_pixel": int(bfound),
        "mean_luma_difference_at_answer": float(np.mean([s / (p.pw * p.ph) for s, p in zip(sad, pl)])),
    }
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
