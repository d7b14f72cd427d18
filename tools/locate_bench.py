"""Locating cut-outs (ssw_locate_rgb8) on one GPU: 128 cut-outs of 1920 x 1080, each from its own marked 4K copy at its own
(odd) position, device-resident.

Reported (device events around the call, median of 5 after one warm-up call; the call synchronises by contract):
  whole call       ms per call and per suspect
  coarse stage     ms per suspect from the stage timer SSW_STAGE_LOCATE_COARSE (median of 5 timed calls), its rate in byte
                   differences per second -- candidate positions x S_f pixels, what the definition asks for, not what the tiles
                   execute -- and that rate as a fraction of the VALU peak it is bound by: lanes per clock (256 CUs x 4 SIMDs x
                   32 lanes) x 4 bytes per v_sad_u8 x clock.  The clock the run held is not measured here: the fraction is
                   against the 2400 MHz maximum, so it is a lower bound of the fraction of what the chip offered.
  found            how many of the suspects were located at their true position

    python tools/locate_bench.py [--suspects 128] [--out profiles/locate_bench_4k.json]
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

LANES_PER_CLOCK = 256 * 4 * 32
MAX_CLOCK_HZ = 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--suspects", type=int, default=128)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_bench_4k.json"))
    a = ap.parse_args()
    W, H, S, k = 3840, 2160, a.suspects, a.k
    cw, ch = W // 2, H // 2
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
        cuts = []
        for s0 in range(0, S, 16):                   # copy s carries mark s; a 4K copy is 25 MB
            n = min(16, S - s0)
            copies = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
            chk(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), base.data_ptr(), W, H, marks[s0:s0 + n].data_ptr(), n, k,
                                               copies.data_ptr(), None))
            stream.synchronize()
            for i in range(n):
                x, y = where[s0 + i]
                cuts.append(copies[i, y:y + ch, x:x + cw].contiguous())
            del copies
    stream.synchronize()
    ptrs = (C.c_void_p * S)(*[c.data_ptr() for c in cuts])
    pl = (L.Placement * S)(*[L.Placement(cw, ch, 3, 0, 0, 0, 0) for _ in range(S)])
    sad = (C.c_uint64 * S)()

    def call():
        chk(lib.ssw_locate_rgb8(ctx.handle, base.data_ptr(), W, H, ptrs, pl, S, sad), "ssw_locate_rgb8")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    timed(call)                                      # warm-up: workspace
    whole = [timed(call) for _ in range(a.repeats)]
    found = sum((p.x, p.y) == xy for p, xy in zip(pl, where))
    mean_diff = float(np.mean([s / (cw * ch) for s in sad]))
    coarse, total, work = [], [], 0.0
    ctx.enable_timing(True)
    for _ in range(a.repeats):
        ctx.reset_timing()
        call()
        t = ctx.timing()
        coarse.append(t["locate_coarse"]["ms"])
        total.append(t["locate"]["ms"])
        work = t["locate_coarse"]["work"]
    ctx.enable_timing(False)
    c_ms, w_ms = float(np.median(coarse)), float(np.median(whole))
    rate = work / (c_ms * 1e-3)
    peak = LANES_PER_CLOCK * 4 * MAX_CLOCK_HZ
    res = {
        "gpu": torch.cuda.get_device_name(0), "frame": [W, H], "cut_out": [cw, ch], "suspects": S, "repeats": a.repeats,
        "whole_call_ms": whole, "whole_call_median_ms": w_ms, "whole_call_ms_per_suspect": w_ms / S,
        "coarse_stage_ms": coarse, "coarse_stage_median_ms": c_ms, "coarse_stage_ms_per_suspect": c_ms / S,
        "locate_stage_median_ms": float(np.median(total)),
        "coarse_byte_differences_per_call": work, "coarse_byte_differences_per_second": rate,
        "valu_peak_byte_differences_per_second_at_2400MHz": peak, "coarse_fraction_of_valu_peak_at_2400MHz": rate / peak,
        "clock_held": "not measured; the fraction is against the 2400 MHz maximum clock",
        "found_at_true_position": int(found), "mean_luma_difference_at_answer": mean_diff,
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
