"""Restoring trace against the composition available before it, on one GPU.

128 u8 4K suspects, each a 1/2-scale whole-frame resize of a ssw_fingerprint_embed_rgb8 copy, M = 1024 stored marks.  From
the same pinned host suspects:
  new          ssw_fingerprint_trace_restored_host_rgb8 (suspects stream as they are, restored per group on the device)
  composition  upload of the suspects, ssw_resize_rgb8 into a temporary [128][2160][3840][3], ssw_fingerprint_trace_rgb8
Device events around each, the two alternating (composition, new, composition) x 5: median of 5 each, and the composition's
two series against each other as its own run-to-run spread.  The restore kernels' GB/s come from the stage timer
(SSW_STAGE_RESIZE: algorithmic bytes / event time) of one extra, timed run.

    python tools/restore_bench.py [--suspects 128] [--marks 1024] [--out profiles/restore_bench_4k.json]
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
    ap.add_argument("--suspects", type=int, default=128)
    ap.add_argument("--marks", type=int, default=1024)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_bench_4k.json"))
    a = ap.parse_args()
    W, H, S, M, k = 3840, 2160, a.suspects, a.marks, a.k
    sw, sh = W // 2, H // 2
    ctx = wm.Context(0)
    lib = ctx._lib
    chk = L.check
    cfg = L.Config()
    lib.ssw_config_default(C.byref(cfg))
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    marks = torch.from_numpy(np.random.default_rng(1).standard_normal((M, k)).astype(np.float32)).to(dev)
    with torch.cuda.stream(stream):
        base_f = torch.empty((1, H, W, 3), dtype=torch.float32, device=dev)
        chk(lib.ssw_synth_frames(ctx.handle, 7, 0, 1, W, H, base_f.data_ptr()))
        base = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        chk(lib.ssw_convert_f32_to_rgb8(ctx.handle, base_f.data_ptr(), base_f.numel(), base.data_ptr()))
        del base_f
        # the suspects: copy s carries mark s; made in batches of 16 (a 4K copy is 25 MB), resized to 1/2 on the device
        small = torch.empty((S, sh, sw, 3), dtype=torch.uint8, device=dev)
        for s0 in range(0, S, 16):
            n = min(16, S - s0)
            copies = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
            chk(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), base.data_ptr(), W, H, marks[s0:s0 + n].data_ptr(), n, k,
                                               copies.data_ptr(), None))
            chk(lib.ssw_resize_rgb8(ctx.handle, copies.data_ptr(), n, W, H, sw, sh, small[s0:s0 + n].data_ptr()))
            del copies
    stream.synchronize()
    host_small = ctx.pinned_empty((S, sh, sw, 3), np.uint8)
    host_small[...] = small.cpu().numpy()
    host_base = ctx.pinned_empty((H, W, 3), np.uint8)
    host_base[...] = base.cpu().numpy()
    host_marks = marks.cpu().numpy()
    ptrs = (C.c_void_p * S)(*[host_small[s].ctypes.data for s in range(S)])
    pl = (L.Placement * S)(*[L.Placement(sw, sh, 3, 0, 0, W, H) for _ in range(S)])
    out = {n: np.empty(shape, dt) for n, shape, dt in (("extracted", (S, k), np.float32), ("sims", (S, M), np.float32), ("best", (S,), np.uint32),
                                                        ("best_sim", (S,), np.float32), ("n_exceed", (S,), np.uint32))}
    outs = [out[n].ctypes.data for n in ("extracted", "sims", "best", "best_sim", "n_exceed")]
    th = C.c_float(6.0)

    def new():
        chk(lib.ssw_fingerprint_trace_restored_host_rgb8(ctx.handle, C.byref(cfg), host_base.ctypes.data, W, H, ptrs, pl, S, k,
                                                         host_marks.ctypes.data, M, th, *outs), "restored trace")

    with torch.cuda.stream(stream):
        d_small = torch.empty((S, sh, sw, 3), dtype=torch.uint8, device=dev)
        d_full = torch.empty((S, H, W, 3), dtype=torch.uint8, device=dev)
        d_ext = torch.empty((S, k), dtype=torch.float32, device=dev)
        d_sims = torch.empty((S, M), dtype=torch.float32, device=dev)
        d_best = torch.empty((S,), dtype=torch.int32, device=dev)
        d_bs = torch.empty((S,), dtype=torch.float32, device=dev)
        d_ne = torch.empty((S,), dtype=torch.int32, device=dev)
    comp = {}

    def composition():
        chk(lib.ssw_copy_to_dev(ctx.handle, base.data_ptr(), host_base.ctypes.data, host_base.nbytes))
        chk(lib.ssw_copy_to_dev(ctx.handle, d_small.data_ptr(), host_small.ctypes.data, host_small.nbytes))
        chk(lib.ssw_resize_rgb8(ctx.handle, d_small.data_ptr(), S, sw, sh, W, H, d_full.data_ptr()))
        chk(lib.ssw_fingerprint_trace_rgb8(ctx.handle, C.byref(cfg), base.data_ptr(), d_full.data_ptr(), S, W, H, k, marks.data_ptr(), M, th,
                                           d_ext.data_ptr(), d_sims.data_ptr(), d_best.data_ptr(), d_bs.data_ptr(), d_ne.data_ptr()))
        for n, t in (("extracted", d_ext), ("sims", d_sims), ("best", d_best), ("best_sim", d_bs), ("n_exceed", d_ne)):
            comp[n] = t.cpu().numpy()                # the results come back to the host in both

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    for fn in (composition, new):                    # warm-up: workspaces, tap tables, bases
        timed(fn)
    t = {"composition_a": [], "new": [], "composition_b": []}
    for _ in range(a.repeats):
        t["composition_a"].append(timed(composition))
        t["new"].append(timed(new))
        t["composition_b"].append(timed(composition))
    equal = {n: bool(np.array_equal(out[n], comp[n].view(out[n].dtype), equal_nan=True)) for n in out}
    named = int((out["best"] == np.arange(S)).sum())
    ctx.reset_timing()
    ctx.enable_timing(True)
    new()
    ctx.synchronize()
    tm = ctx.timing()
    ctx.enable_timing(False)
    rz = tm["resize"]
    med = {n: float(np.median(v)) for n, v in t.items()}
    comp_med = 0.5 * (med["composition_a"] + med["composition_b"])
    spread = abs(med["composition_a"] - med["composition_b"])
    res = {
        "gpu": torch.cuda.get_device_name(0), "frame": [W, H], "suspect": [sw, sh], "suspects": S, "marks": M, "k": k, "repeats": a.repeats,
        "ms": t, "median_ms": med, "composition_spread_ms": spread, "speedup_new_vs_composition": comp_med / med["new"],
        "new_not_slower_than_composition_by_more_than_its_spread": bool(med["new"] <= max(med["composition_a"], med["composition_b"]) + spread),
        "outputs_equal_to_composition": equal, "suspects_named": named,
        "restore_stage": {"ms": rz["ms"], "timed_regions": rz["launches"], "algorithmic_bytes": rz["work"],
                          "gb_per_s": rz["work"] / (rz["ms"] * 1e-3) / 1e9 if rz["ms"] else None,
                          "bytes_per_restored_pixel": rz["work"] / (S * W * H) if S else None},
    }
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    assert res["new_not_slower_than_composition_by_more_than_its_spread"], med
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
