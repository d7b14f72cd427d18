"""The selection of a pruned base reader (csrc/select.hip under a tile mask, csrc/base_prune.hip): skipped
column tiles of the base plane are NOT written any more -- they hold whatever the workspace held -- and the selection
reads the computed tiles only; phase 1 of the column pass runs on a grid of one line tile per frame.  Every case compares
`extracted` and `similarity` byte for byte with the same call under base_prune = 0 (the full transform).

Shape, tuning overrides and frame generators: those of tests/test_base_prune_gpu.py (384 x 256, 32 frames, k = 64: the
smallest shape on which the fused forward transform, and hence the pruning, runs at all); one case uses W = 256."""

import numpy as np
import pytest

import gpu_util as G
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import check, tuning
from test_base_prune_gpu import (FUSED, H, K, N, W, check_oracle, expected_routes, marks_for, noise, routes, run_pair,
                                 with_cosine)

pytestmark = pytest.mark.gpu


def smooth(n, h, w, seed):
    """The frames of test_base_prune_gpu.smooth (240 cosines of horizontal and vertical frequency below 24 + noise of 1e-4),
    summed as one 24 x 24 coefficient matrix between two cosine tables instead of 240 full-size planes."""
    rng = np.random.default_rng(seed)
    cy = np.cos(np.pi * (2 * np.arange(h)[:, None] + 1) * np.arange(24)[None, :] / (2 * h))
    cx = np.cos(np.pi * (2 * np.arange(w)[:, None] + 1) * np.arange(24)[None, :] / (2 * w))
    out = np.empty((n, h, w, 3), np.float32)
    for f in range(n):
        amp = np.zeros((24, 24))
        for _ in range(240):
            fx, fy = rng.integers(0, 24), rng.integers(0, 24)
            amp[fy, fx] += rng.uniform(0.2, 1.0) / (1 + fx + fy)
        a = cy @ amp @ cx.T
        a = 0.5 + 0.35 * a / np.abs(a).max()
        for c in range(3):
            out[f, :, :, c] = a + 1e-4 * rng.standard_normal((h, w))
    return np.clip(out, 0.0, 1.0).astype(np.float32)


def poison(n, h, w, seed):
    """White noise plus a strong cosine in every column tile behind tile 0: every tile is computed, and every tile of the
    workspace plane is left holding keys far above anything a smooth frame has."""
    base = noise(n, h, w, seed)
    for t in range(1, w // 128):
        base = with_cosine(base, 128 * t + 5)
    return base


@pytest.fixture(scope="module", autouse=True)
def fused_settings():
    with tuning(**FUSED), G.fresh_ctx():
        yield


@pytest.fixture(scope="module")
def smooth_frames():
    return smooth(N, H, W, 11)


def embedded(base, marks):
    with np.errstate(all="ignore"):
        return G.batch_embed(base, marks)["rgb"]


@pytest.mark.parametrize("w", [W, 256])
def test_stale_workspace_is_never_read(smooth_frames, w):
    """One context: 32 poison frames first (all tiles computed), then 32 smooth frames whose skipped tiles are that stale
    plane.  A mask ignored by the sample, the compaction, the finish or a reader of the plane changes the index list."""
    base = smooth_frames if w == W else smooth(N, H, w, 15)
    tpf = w // 128
    marks = marks_for(N, K)
    dirty = poison(N, H, w, 21)
    derived, derived_dirty = embedded(base, marks), embedded(dirty, marks)
    with G.fresh_ctx() as ctx:
        assert ctx.transform_plan(N, w, H)["fused_cols"]
        G.batch_extract(dirty, derived_dirty, K, marks)
        assert routes(ctx.prune_stats(), N, tpf) == (tpf * N, N)
        ctx.reset_timing()
        on = G.batch_extract(base, derived, K, marks)
        st, sel = ctx.prune_stats(), ctx.select_stats()
    assert routes(st, N, tpf) == (N, 0), st
    assert sel["exact_fallback_frames"] == 0, sel
    with tuning(base_prune=0), G.fresh_ctx():
        off = G.batch_extract(base, derived, K, marks)
    assert on[0].tobytes() == off[0].tobytes(), "extracted marks differ from the full transform on a fresh context"
    assert on[1].tobytes() == off[1].tobytes(), "similarities differ from the full transform on a fresh context"
    check_oracle(base, derived, marks, on)


def test_mixed_batch(smooth_frames):
    """Smooth, white-noise, constant and NaN-pixel frames and frames with a strong cosine in the last tile in one call; the
    tile counters against the numpy restatement of T and the needed tiles (a NaN pixel makes every energy of its frame NaN:
    every tile is needed)."""
    base = smooth_frames.copy()
    base[1::5] = noise(len(base[1::5]), H, W, 14)
    base[2::5] = 0.5
    base[3::5, 10, 300, 0] = np.nan
    base[4::5] = with_cosine(base[4::5], 128 * 2 + 5)
    derived = with_cosine(base, 7, 0.01)
    G.batch_extract(poison(N, H, W, 22), derived, K, marks_for(N, K))           # stale keys in every tile of the workspace
    on, st, _, _ = run_pair(base, K, derived=derived)
    # the restatement needs a batch that takes the fused transform (28 frames or more) and compares bounds with coefficients,
    # which means nothing on a plane of NaN or of rounding noise around zero: frames are independent, so the NaN and the
    # constant frames are replaced by white-noise frames, which the restatement itself finds to need every tile
    stand_in = base.copy()
    stand_in[2::5] = noise(len(base[2::5]), H, W, 15)
    stand_in[3::5] = noise(len(base[3::5]), H, W, 16)
    computed, extended = expected_routes(stand_in, K)
    assert routes(st, N, 3) == (computed, extended), st
    n_s, n_c = len(base[0::5]), len(base[4::5])
    assert (computed, extended) == (n_s + 2 * n_c + 3 * (N - n_s - n_c), N - n_s), (computed, extended)


def masked_select(coef, k, need=None, cand_cap=0, ordering=L.ORDER_ENERGY):
    ctx = G.ctx()
    n, h, w = coef.shape
    d = ctx.to_device(np.ascontiguousarray(coef, np.float32))
    nd = ctx.to_device(np.ascontiguousarray(need, np.uint32)) if need is not None else None
    idx = ctx.alloc(n * k * 4)
    check(G.lib().ssw_debug_select_masked(ctx.handle, d.ptr, n, w, h, ordering, k, nd.ptr if nd else None, cand_cap, idx.ptr),
          "ssw_debug_select_masked")
    out = idx.to_host(np.uint32, (n, k))
    for b in (d, nd, idx):
        if b:
            b.free()
    return out


@pytest.mark.parametrize("ordering", [L.ORDER_ENERGY, L.ORDER_ENERGY_ORTHOGONAL])
def test_exact_whole_plane_route_skips_masked_tiles(smooth_frames, ordering):
    """The finish kernel's exact select over the whole plane (forced: a candidate list shorter than k) under a mask, on planes
    whose skipped tiles hold huge keys and NaN: the indices of the unmasked selection on the zero-filled plane."""
    n = 4
    y = G.rgb_to_yiq(smooth_frames[:n], with_iq=False)[0]
    coef = G.dct2d(np.asarray(y, np.float32).reshape(n, H, W), L.DCT2, L.PRECISION_F64)
    need = np.array([[1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]], np.uint32)
    rng = np.random.default_rng(3)
    zero_filled, dirty = coef.copy(), coef.copy()
    for f in range(n):
        for t in range(3):
            if not need[f, t]:
                zero_filled[f, :, 128 * t:128 * (t + 1)] = 0.0
                junk = (1e6 * rng.standard_normal((H, 128))).astype(np.float32)
                junk[rng.integers(0, H, 50), rng.integers(0, 128, 50)] = np.nan
                dirty[f, :, 128 * t:128 * (t + 1)] = junk
    want = masked_select(zero_filled, K, ordering=ordering)
    ctx = G.ctx()
    ctx.reset_timing()
    assert np.array_equal(masked_select(dirty, K, need, ordering=ordering), want), "candidate route"
    assert ctx.select_stats()["exact_fallback_frames"] == 0
    assert np.array_equal(masked_select(dirty, K, need, cand_cap=K // 2, ordering=ordering), want), "exact whole-plane route"
    assert ctx.select_stats()["exact_fallback_frames"] == n
    # ... and an all-ones mask is no mask
    assert np.array_equal(masked_select(coef, K, np.ones((n, 3), np.uint32), ordering=ordering), masked_select(coef, K, ordering=ordering))


@pytest.mark.parametrize("jobs,n", [("none", 29), ("one", 29), ("all", 29), ("all", 32)])
def test_phase_grids(smooth_frames, jobs, n):
    """Phase 2 without a job, with exactly one job per frame (the last tile), and with every job (white noise: n x 2 line tiles
    x 8 classes x 3 pair tiles); 29 frames are not a multiple of the eight XCDs the block map deals tiles to."""
    base = {"none": smooth_frames[:n], "one": with_cosine(smooth_frames[:n], 128 * 2 + 5), "all": noise(n, H, W, 31)}[jobs]
    base = np.ascontiguousarray(base)
    on, st, derived, marks = run_pair(base, K)
    assert routes(st, n, 3) == {"none": (n, 0), "one": (2 * n, n), "all": (3 * n, n)}[jobs], st
    check_oracle(base, derived, marks, on)
