"""Base-reader pruning of ssw_batch_extract (csrc/base_prune.hip): the base frame's column pass runs on the
128-column tiles that can hold one of the first k keys.  Every case compares `extracted` and `similarity` byte for byte
with the same call under base_prune = 0 (the full transform), checks the counters, and frames 0 and last against the
oracle at the bars of tests/test_gpu_parity.py.

Shape: 384 x 256 (three column tiles: first, middle, last), k = 64, and 32 frames -- the planner takes the fused forward
transform only where both passes fill 448 block slots with 128-line tiles (dct_plan.hip: launch_is_small), which at this
size needs 28 frames or more with the eight classes of a pass merged into one launch (merge_max_lines raised); 8 frames
cannot take the fused path under any setting.  One case uses W = 256."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_util as G
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import check, tuning

pytestmark = pytest.mark.gpu

H, W, N, K = 256, 384, 32, 64
FUSED = dict(merge_max_lines=65536, efold_min=256, efold_inv_min=256, efold_cols_min=64)


def smooth(n, h, w, seed):
    """240 low-frequency cosines (horizontal frequencies below 24: all inside column tile 0, and far more than k = 64 of them
    strong) + noise of 1e-4."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w, 3), np.float32)
    for f in range(n):
        a = np.zeros((h, w))
        for _ in range(240):
            fx, fy = rng.integers(0, 24), rng.integers(0, 24)
            a += rng.uniform(0.2, 1.0) / (1 + fx + fy) * np.cos(np.pi * (2 * x + 1) * fx / (2 * w)) * np.cos(np.pi * (2 * y + 1) * fy / (2 * h))
        a = 0.5 + 0.35 * a / np.abs(a).max()
        for c in range(3):
            out[f, :, :, c] = a + 1e-4 * rng.standard_normal((h, w))
    return np.clip(out, 0.0, 1.0).astype(np.float32)


def noise(n, h, w, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, h, w, 3)).astype(np.float32)


def with_cosine(frames, col, amp=0.1):
    """+ one strong horizontal cosine of frequency `col` (and vertical frequency 3)."""
    n, h, w, _ = frames.shape
    y, x = np.mgrid[0:h, 0:w]
    c = amp * np.cos(np.pi * (2 * x + 1) * col / (2 * w)) * np.cos(np.pi * (2 * y + 1) * 3 / (2 * h))
    return np.clip(frames + c[None, :, :, None], 0.0, 1.0).astype(np.float32)


def marks_for(n, k, seed=5):
    return np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)


def run_pair(base, k, cfg=None, marks=None, derived=None):
    """(extracted, sims, counters) with base pruning on, and the same call with base_prune = 0."""
    n, h, w, _ = base.shape
    marks = marks_for(n, k) if marks is None else marks
    ctx = G.ctx()
    assert ctx.transform_plan(n, w, h)["fused_cols"], "the fused forward transform must be the path under test"
    if derived is None:
        with np.errstate(all="ignore"):
            derived = G.batch_embed(base, marks, cfg)["rgb"]
    ctx.reset_timing()
    on = G.batch_extract(base, derived, k, marks, cfg)
    st = ctx.prune_stats()
    with tuning(base_prune=0):
        ctx.reset_timing()
        off = G.batch_extract(base, derived, k, marks, cfg)
        st_off = ctx.prune_stats()
    assert st_off["base_tiles"] == 0, st_off
    assert on[0].tobytes() == off[0].tobytes(), "extracted marks differ from the full transform"
    assert on[1].tobytes() == off[1].tobytes(), "similarities differ from the full transform"
    return on, st, derived, marks


def routes(st, n, tiles_per_frame):
    """(tiles computed, frames extended) of one pass over the n base frames.  A chunk whose derived column set overflows the
    compact plane is redone with the full derived transform, base frame included: the counters then hold two passes."""
    passes = st["base_tiles"] // (n * tiles_per_frame)
    assert passes in (1, 2) and st["base_tiles"] == passes * n * tiles_per_frame, st
    assert st["base_tiles_computed"] % passes == 0 and st["base_frames_extended"] % passes == 0, st
    return st["base_tiles_computed"] // passes, st["base_frames_extended"] // passes


def check_oracle(base, derived, marks, on, cfg_kw=None):
    for f in (0, base.shape[0] - 1):
        ref_ext, ref_sim = O.extract_frame(base[f], derived[f], marks[f], **(cfg_kw or {}))
        assert G.ext_within_1e5(on[0][f], ref_ext), f
        assert abs(float(on[1][f]) - ref_sim) < 1e-4 * max(1.0, abs(ref_sim)), (f, on[1][f], ref_sim)


def check_bound(base, k=K, ordering=L.ORDER_ENERGY, coef=None):
    """boundkey(v) >= the largest key of column v of the library's own full plane (or of `coef`, a reference plane [n, h, w] of
    the caller's), on every frame."""
    n, h, w, _ = base.shape
    ctx = G.ctx()
    d = ctx.to_device(np.ascontiguousarray(base))
    out = ctx.alloc(n * w * 4)
    cfg = G.default_config(ordering=ordering)
    check(G.lib().ssw_debug_base_prune_bound(ctx.handle, C.byref(cfg), d.ptr, n, w, h, k, out.ptr), "ssw_debug_base_prune_bound")
    bound = out.to_host(np.float32, (n, w))
    d.free(); out.free()
    if coef is None:
        yplane = G.rgb_to_yiq(base, with_iq=False)[0]
        coef = G.dct2d(np.asarray(yplane, np.float32).reshape(n, h, w), L.DCT2, L.PRECISION_F64)
    coef = np.asarray(coef, np.float32).reshape(n, h, w)
    with np.errstate(all="ignore"):
        if ordering == L.ORDER_ENERGY:
            key = (coef * coef).astype(np.float32)
        else:
            s = np.full((h, w), np.float32(np.sqrt(np.float32(1 / (2 * w))) * np.sqrt(np.float32(1 / (2 * h)))), np.float32)
            key = ((s * coef).astype(np.float32) ** 2).astype(np.float32)       # the largest scale everywhere: an upper bound of the key
        worst = key.max(axis=1)
    finite = np.isfinite(worst) & np.isfinite(bound)
    assert np.all(bound[finite] >= worst[finite]), float((worst[finite] / np.maximum(bound[finite], 1e-30)).max())
    assert not np.any(np.isfinite(bound) & ~np.isfinite(worst)), "a finite bound over a non-finite column"
    return bound


@pytest.fixture(scope="module", autouse=True)
def fused_settings():
    with tuning(**FUSED), G.fresh_ctx():
        yield


@pytest.fixture(scope="module")
def smooth_frames():
    return smooth(N, H, W, 11)


def test_smooth_frames_skip_tiles(smooth_frames):
    on, st, derived, marks = run_pair(smooth_frames, K)
    assert routes(st, N, 3) == (N, 0), st
    check_oracle(smooth_frames, derived, marks, on)
    check_bound(smooth_frames)


def test_white_noise_skips_nothing():
    base = noise(N, H, W, 12)
    on, st, derived, marks = run_pair(base, K)
    assert routes(st, N, 3) == (3 * N, N), st
    check_oracle(base, derived, marks, on)
    check_bound(base)


def test_strong_cosine_in_the_last_tile_is_computed(smooth_frames):
    base = with_cosine(smooth_frames, 128 * 2 + 5)
    on, st, derived, marks = run_pair(base, K)
    assert routes(st, N, 3) == (2 * N, N), st
    check_oracle(base, derived, marks, on)
    check_bound(base)


def test_cosine_filling_one_column_is_the_equality_case():
    y, x = np.mgrid[0:H, 0:W]
    a = 0.5 + 0.4 * np.cos(np.pi * (2 * x + 1) * 200 / (2 * W))               # all of its energy in (u, v) = (0, 200)
    base = np.repeat(np.repeat(a[None, :, :, None], 3, axis=3), N, axis=0).astype(np.float32)
    run_pair(base, K)
    bound = check_bound(base)
    assert bound[0, 200] > bound[0, 300]


def test_constant_frames_tie_at_zero():
    base = np.full((N, H, W, 3), 0.5, np.float32)
    on, st, _, _ = run_pair(base, K)
    assert routes(st, N, 3) == (3 * N, N), st              # no positive k-th key: every tile is needed


def test_nan_and_inf_pixels(smooth_frames):
    base = smooth_frames.copy()
    base[1, 10, 300, 0] = np.nan
    base[2, 20, 20, 1] = np.inf
    derived = with_cosine(base, 7, 0.01)
    run_pair(base, K, derived=derived)


def expected_routes(base, k):
    """What the decide kernel must find, restated in numpy from the library's own full plane and its own bounds: per frame
    T = the lower edge of the 11-bit bin of the sortable key that holds the k-th largest key of tile 0 (index 0 excluded), and
    tile t > 0 is needed when one of its columns has bound >= T (all of them when T is not above 1e-30)."""
    n, h, w, _ = base.shape
    bound = check_bound(base, k)
    coef = G.dct2d(G.rgb_to_yiq(base, with_iq=False)[0].reshape(n, h, w), L.DCT2, L.PRECISION_F64)
    computed = extended = 0
    for f in range(n):
        keys = (coef[f, :, :128] * coef[f, :, :128]).astype(np.float32).reshape(-1)[1:]
        kth = np.partition(keys, keys.size - k)[keys.size - k]
        edge = (np.array([kth], np.float32).view(np.uint32) & np.uint32(0xFFE00000)).view(np.float32)[0]
        need = [edge <= 1e-30 or bool(np.any(bound[f, t * 128:(t + 1) * 128] >= edge)) for t in range(1, w // 128)]
        computed += 1 + sum(need)
        extended += any(need)
    return computed, extended


@pytest.mark.parametrize("k", [64, 2000, 16384])
def test_threshold_and_needed_tiles_against_numpy(smooth_frames, k):
    """The counters equal the numpy restatement at a short, a middle and the longest mark the in-LDS selection takes (16384;
    longer marks use the full sort and the full transform).  At 16384 the k-th key lies in the noise and tiles are needed that
    k = 64 skips.  The kernel's "fewer than k keys in tile 0" answer (every tile needed) cannot be reached through the library:
    the fused transform needs H >= 144 (dct_plan.hip: pair_kpad(H / 8) == dct_pair_fused_units(H)), so tile 0 holds at least
    128 * 144 - 1 = 18431 keys, more than the longest mark of this path."""
    base = with_cosine(smooth_frames, 128 + 9)
    base[::2] = smooth_frames[::2]
    on, st, _, _ = run_pair(base, k)
    assert routes(st, N, 3) == expected_routes(base, k), st


def test_unmerged_row_launches():
    """224 frames at the default merge_max_lines: the eight energy row launches run one by one (as in the 4K benchmark), not as
    the one merged launch the 32-frame cases take."""
    n = 224
    few = smooth(8, H, W, 17)
    few[1::2] = with_cosine(few[1::2], 128 * 2 + 5)
    base = np.ascontiguousarray(np.tile(few, (n // 8, 1, 1, 1)))
    with tuning(merge_max_lines=8192), G.fresh_ctx():
        on, st, derived, marks = run_pair(base, K)
        assert routes(st, n, 3) == (n // 2 + 2 * (n // 2), n // 2), st
    check_oracle(base, derived, marks, on)


def test_mixed_batch_takes_different_routes(smooth_frames):
    base = smooth_frames.copy()
    base[1::3] = noise(len(base[1::3]), H, W, 14)
    base[2::3] = with_cosine(base[2::3], 128 + 9)
    on, st, derived, marks = run_pair(base, K)
    n_a, n_b, n_c = len(base[0::3]), len(base[1::3]), len(base[2::3])
    assert routes(st, N, 3) == (n_a + 3 * n_b + 2 * n_c, n_b + n_c), st
    check_oracle(base, derived, marks, on)


@pytest.mark.parametrize("method", [L.OPTION1, L.OPTION2, L.OPTION3])
@pytest.mark.parametrize("ordering", [L.ORDER_ENERGY, L.ORDER_ENERGY_ORTHOGONAL, L.ORDER_LEGACY])
def test_orderings_and_methods(smooth_frames, ordering, method):
    cfg = G.default_config(ordering=ordering, method=method)
    for base, tiles in ((smooth_frames, N), (with_cosine(smooth_frames, 128 * 2 + 5), 2 * N)):
        on, st, _, _ = run_pair(base, K, cfg)
        if ordering == L.ORDER_LEGACY:
            assert st["base_tiles"] == 0, st               # signed keys: no bound, the full transform
        else:
            assert routes(st, N, 3)[0] == tiles, st
    if ordering != L.ORDER_LEGACY:
        check_bound(smooth_frames, ordering=ordering)


def test_two_chunks_on_two_lanes(smooth_frames):
    base = np.concatenate([smooth_frames, with_cosine(smooth_frames, 128 + 9)])
    ctx = G.ctx()
    ctx.set_chunk_frames(N)
    try:
        on, st, _, _ = run_pair(base, K)
        assert routes(st, 2 * N, 3) == (N + 2 * N, N), st
    finally:
        ctx.set_chunk_frames(0)


def test_mixed_redo_with_base_prune_equals_the_unchunked_call(smooth_frames):
    """The two-chunk input of test_pruned_path_falls_back_when_the_columns_do_not_fit with base pruning on: the 32 index lists
    of the white-noise chunk use far more than the compact plane's 64 columns (each list alone about 59 of 384), so that chunk
    is redone with the full transform, base frames included; the smooth chunk (all keys below column 24) fits.  Beside the
    byte equality with base_prune = 0 (run_pair): the counters of both prunings, and the same bits as one chunk of 64 frames."""
    base = np.concatenate([noise(N, H, W, 12), smooth_frames])
    ctx = G.ctx()
    ctx.set_chunk_frames(N)
    try:
        on, st, derived, marks = run_pair(base, K)
    finally:
        ctx.set_chunk_frames(0)
    assert st["pruned_chunks"] == 2 and st["redone_chunks"] == 1, st
    assert st["base_tiles"] == (2 + 1) * N * 3 and st["base_tiles_computed"] == 2 * 3 * N + N, st      # the noise chunk twice
    whole = G.batch_extract(base, derived, K, marks)
    assert on[0].tobytes() == whole[0].tobytes() and on[1].tobytes() == whole[1].tobytes()
    ctx.set_prune(False)
    try:
        full = G.batch_extract(base, derived, K, marks)
    finally:
        ctx.set_prune(True)
    assert on[0].tobytes() == full[0].tobytes() and on[1].tobytes() == full[1].tobytes()


def test_two_tiles_wide():
    base = with_cosine(smooth(48, H, 256, 15), 128 + 40)
    base[::2] = smooth(24, H, 256, 16)
    on, st, derived, marks = run_pair(base, K)
    assert routes(st, 48, 2) == (48 + 24, 24), st
    check_oracle(base, derived, marks, on)


_GRAPH_SCRIPT = r"""
import ctypes as C, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import spread_spectrum_watermarking_amd as wm
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import check, tuning
lib = L.load()
base_np = np.load(sys.argv[2]); n, h, w, _ = base_np.shape; k = 64
with tuning(merge_max_lines=65536, efold_min=256, efold_inv_min=256, efold_cols_min=64):
    ctx = wm.Context(0)
    assert ctx.transform_plan(n, w, h)["fused_cols"]
    dev = torch.device("cuda", 0)
    base = torch.from_numpy(base_np).to(dev)
    marks = torch.randn((n, k), device=dev); derived = torch.empty_like(base)
    ext = torch.zeros((n, k), device=dev); sims = torch.zeros((n,), device=dev)
    cfg = L.Config(L.ORDER_ENERGY, L.OPTION2, 0.1, L.PRECISION_F64)
    torch.cuda.synchronize()
    check(lib.ssw_batch_embed(ctx.handle, C.byref(cfg), base.data_ptr(), n, w, h, marks.data_ptr(), k, derived.data_ptr(), None, None), "embed")
    def step():
        check(lib.ssw_batch_extract(ctx.handle, C.byref(cfg), base.data_ptr(), derived.data_ptr(), n, w, h, k, ext.data_ptr(), marks.data_ptr(), sims.data_ptr()), "extract")
    step(); ctx.synchronize()                      # eager: workspaces sized, bases cached
    want = (ext.clone(), sims.clone())
    with tuning(base_prune=0):
        ext.zero_(); sims.zero_(); torch.cuda.synchronize()
        step(); ctx.synchronize()
        assert torch.equal(ext, want[0]) and torch.equal(sims, want[1]), "eager differs from base_prune = 0"
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ext.zero_(); sims.zero_(); torch.cuda.synchronize()
    ctx.reset_timing()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
        step()
    torch.cuda.synchronize()
    assert ctx.prune_stats()["base_tiles"] == 0, "a capture runs nothing"
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(ext, want[0]) and torch.equal(sims, want[1]), "replay differs from eager"
    st = ctx.prune_stats()
    # one pass (the captured call takes the full derived transform: no redo): half of the frames need the last tile
    assert (st["base_tiles"], st["base_tiles_computed"], st["base_frames_extended"]) == (3 * n, n + n // 2, n // 2), st
    print("graph-ok")
    ctx.set_stream(None); ctx.close()
"""


def test_captured_into_a_graph_and_replayed(tmp_path, smooth_frames):
    """ssw_batch_extract with base pruning captured into a HIP graph (the energy memset, both phase launches, the decide and
    zero-fill kernels and their device counters are nodes of the graph) and replayed once: byte-equal to the eager call and to
    base_prune = 0, counters of exactly one pass after the replay."""
    base = with_cosine(smooth_frames, 128 * 2 + 5)
    base[::2] = smooth_frames[::2]
    np.save(tmp_path / "base.npy", base)
    script = tmp_path / "graph_check.py"
    script.write_text(_GRAPH_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(script), root, str(tmp_path / "base.npy")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "graph-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
