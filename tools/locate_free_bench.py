"""Locating scaled cut-outs whose aspect ratio was not kept exactly (ssw_locate_free_rgb8) on one GPU: 16 cut-outs of
1920 x 1080, each from its own marked 4K copy at its own (odd) position, halved by Pillow (BICUBIC) to 960 x 541 -- off the
aspect ratio by rounding --; the finder knows that the cut-out was between 1800 and 2040 wide in the original.

Reported (device events around each call, median of 5 after one warm-up call each, the routes alternating):
  free a=2, a=4    ssw_locate_free_rgb8 with slack 2 and 4: ms per call, and from the stage timers (a second set of timed
                   calls) what SSW_STAGE_LOCATE and SSW_STAGE_RESIZE grow by over the ladder's
  scaled           ssw_locate_scaled_rgb8 on the same input, from the same build: the ladder the stage follows; the difference
                   is the stage's cost
  per size         what a caller had to do before for the same 25 sizes of a = 2: one ssw_locate_rgb8 call per (pw, ph) around
                   the ladder's answer, each a search of the whole frame.  Run on --baseline-suspects of the 16 (default 1)
  exact            how many of the 16 each route answers exactly (1920 x 1080 at its position)

    python tools/locate_free_bench.py [--out profiles/locate_free_bench.json]
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
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--suspects", type=int, default=16)
    ap.add_argument("--baseline-suspects", type=int, default=1)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_free_bench.json"))
    a = ap.parse_args()
    W, H, S, k = 3840, 2160, a.suspects, a.k
    cw, ch, sw, sh, wmin, wmax = 1920, 1080, 960, 541, 1800, 2040
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
        cuts = [copies[i, y:y + ch, x:x + cw].contiguous().cpu().numpy() for i, (x, y) in enumerate(where)]
        del copies
    thumbs = np.stack([np.asarray(Image.fromarray(c).resize((sw, sh), Image.BICUBIC)) for c in cuts])
    small = torch.from_numpy(np.ascontiguousarray(thumbs)).to(dev)
    stream.synchronize()
    ptrs = (C.c_void_p * S)(*[small[i].data_ptr() for i in range(S)])
    rg = (L.ScaleRange * S)(*[L.ScaleRange(wmin, wmax) for _ in range(S)])
    new_pl = lambda: (L.Placement * S)(*[L.Placement(sw, sh, 3, 0, 0, 0, 0) for _ in range(S)])
    pls = {"scaled": new_pl(), "free2": new_pl(), "free4": new_pl()}
    sads = {name: (C.c_uint64 * S)() for name in pls}
    slack = {2: (C.c_uint32 * S)(*[2] * S), 4: (C.c_uint32 * S)(*[4] * S)}

    def scaled():
        chk(lib.ssw_locate_scaled_rgb8(ctx.handle, base.data_ptr(), W, H, ptrs, pls["scaled"], rg, S, sads["scaled"]), "ssw_locate_scaled_rgb8")

    def free(a_):
        name = "free%d" % a_
        return lambda: chk(lib.ssw_locate_free_rgb8(ctx.handle, base.data_ptr(), W, H, ptrs, pls[name], rg, slack[a_], S, sads[name]), "ssw_locate_free_rgb8")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    timed(scaled)                                   # warm-up, and the ladder's answers the per-size route starts from
    sizes = [[(pw, ph) for pw in range(p.pw - 2, p.pw + 3) for ph in range(p.ph - 2, p.ph + 3)] for p in list(pls["scaled"])[:B]]
    nb = sum(len(z) for z in sizes)
    per = len(sizes[0]) if sizes else 0
    bsad = (C.c_uint64 * max(B, 1))()

    def per_size():                                 # one call per (pw, ph): the B suspects at the j-th size around their own ladder answer
        out = []
        for j in range(per):
            bp = (L.Placement * B)(*[L.Placement(sw, sh, 3, 0, 0, sizes[i][j][0], sizes[i][j][1]) for i in range(B)])
            chk(lib.ssw_locate_rgb8(ctx.handle, base.data_ptr(), W, H, ptrs, bp, B, bsad), "ssw_locate_rgb8")
            out.append([(p.pw, p.ph, p.x, p.y, int(s)) for p, s in zip(bp, bsad)])
        return out

    routes = {"scaled": scaled, "free2": free(2), "free4": free(4), "per_size": per_size}
    for fn in routes.values():
        timed(fn)                                   # warm-up: workspace, cached tap tables
    times = {name: [] for name in routes}
    for _ in range(a.repeats):
        for name, fn in routes.items():
            times[name].append(timed(fn))
    truth = [(cw, ch) + xy for xy in where]
    exact = {name: int(sum((p.pw, p.ph, p.x, p.y) == t for p, t in zip(pls[name], truth))) for name in pls}
    best = [min((r[i] for r in per_size()), key=lambda v: (v[4] / (v[0] * v[1]), v[0], v[1], v[3], v[2])) for i in range(B)]
    exact["per_size"] = int(sum(b[:4] == t for b, t in zip(best, truth)))
    stages = {name: {"resize": [], "locate_coarse": [], "locate": []} for name in ("scaled", "free2", "free4")}
    ctx.enable_timing(True)
    for _ in range(a.repeats):
        for name in stages:
            ctx.reset_timing()
            routes[name]()
            t = ctx.timing()
            for st in stages[name]:
                stages[name][st].append(t[st]["ms"])
    ctx.enable_timing(False)
    med = lambda v: float(np.median(v))
    m = {name: med(v) for name, v in times.items()}
    res = {
        "gpu": torch.cuda.get_device_name(0), "frame": [W, H], "cut_out": [cw, ch], "suspect": [sw, sh], "widths": [wmin, wmax],
        "suspects": S, "repeats": a.repeats, "call_ms": times, "median_ms": m,
        "stage_cost_ms": {"a=2": m["free2"] - m["scaled"], "a=4": m["free4"] - m["scaled"]},
        "stage_cost_over_ladder": {"a=2": (m["free2"] - m["scaled"]) / m["scaled"], "a=4": (m["free4"] - m["scaled"]) / m["scaled"]},
        "stage_timers_median_ms": {name: {st: med(v) for st, v in by.items()} for name, by in stages.items()},
        "per_size_suspects": B, "per_size_calls": per, "per_size_entries": nb, "per_size_ms_per_suspect": m["per_size"] / max(B, 1),
        "per_size_over_stage_per_suspect_a2": (m["per_size"] / max(B, 1)) / max((m["free2"] - m["scaled"]) / S, 1e-9),
        "exact_of": {"scaled": [exact["scaled"], S], "free2": [exact["free2"], S], "free4": [exact["free4"], S], "per_size": [exact["per_size"], B]},
        "answers": {name: [[p.pw, p.ph, p.x, p.y] for p in pls[name]] for name in pls}, "truth": [list(t) for t in truth],
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
