"""The low-precision tail bound of the base-reader pruning (csrc/base_energy.hip): rows of more than one
64-pair tile column per launch class run the exact energy launches on tile column 0 only, bound the other columns'
energies from f16 hi + lo products, and run the exact launches of those tile columns after the decision, gated per frame.

Every case compares `extracted` and `similarity` byte for byte with base_energy_lowp = 0 and with base_prune = 0, checks the
tile and tail-job counters, and frames 0 and last against the oracle at the bars of tests/test_gpu_parity.py.  Shapes: H = 256,
k = 64, the settings of tests/test_base_prune_gpu.py, and the smallest batch that takes the fused forward transform.
  W = 1152, tile48 = 0: 72 pairs per class = 64 + 8, a tail of 8 pairs, the narrowest tail tile (one 16-pair MFMA tile of the
            bound kernel, the one-pair-tile path of the gated row instance): nine column tiles, the head feeds tiles 0 .. 7,
            the tail tile column tiles 7 .. 8;
  W = 1152, tile48 = 1 (the default): the same 72 pairs as 48 + 24: the head feeds tiles 0 .. 5 (and one line of the last),
            the tail tile column tiles 5 .. 8;
  W = 2048: 128 pairs = 64 + 64: sixteen column tiles, the head feeds 0 .. 7, the tail tile column 7 .. 15.
A layout is (W, tile48); tile48 = 0 runs on a context of its own inside the tuning block.  A job is (frame, class, tail tile
column): a frame whose needed tile lies in the tail runs the eight classes' one tail tile column, eight jobs."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_util as G
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import tuning
from test_base_prune_gpu import FUSED, check_bound, check_oracle, marks_for, noise, routes, with_cosine
from tail_layout import tail_layout
from test_base_select_gpu import smooth

pytestmark = pytest.mark.gpu

H, K = 256, 64
NARROW, W48, WIDE = (1152, 0), (1152, 1), (2048, 1)
LAYOUTS = [NARROW, W48, WIDE]
FIRST_TAIL_TILE = {NARROW: 8, W48: 6, WIDE: 8}          # the first column tile that only the tail feeds
lay_id = lambda lay: f"{lay[0]}-tile48={lay[1]}"


@contextlib.contextmanager
def layout(lay):
    """The tiling of a layout: the default one on the module's context, tile48 = 0 on a fresh one."""
    if lay[1]:
        yield
    else:
        with tuning(tile48=0), G.fresh_ctx():
            yield


@pytest.fixture(scope="module", autouse=True)
def fused_settings():
    with tuning(**FUSED), G.fresh_ctx():
        yield


_frames = {}


def fused_batch(w):
    """The smallest batch whose forward transform is the fused one (run_three asserts it on the context it runs on)."""
    ctx = G.ctx()
    return next(i for i in range(1, 65) if ctx.transform_plan(i, w, H)["fused_cols"])


def frames_of(w):
    """(n, smooth frames) of that batch, computed once per width."""
    if w not in _frames:
        n = fused_batch(w)
        _frames[w] = (n, smooth(n, H, w, 31 + w))
    n, f = _frames[w]
    return n, f.copy()


def embedded(base, marks):
    with np.errstate(all="ignore"):
        return G.batch_embed(base, marks)["rgb"]


def run_three(base, cfg=None, derived=None):
    """The call with the tail bound on, with base_energy_lowp = 0 and with base_prune = 0: the same bytes.  Returns the first
    call's outputs and counters."""
    n, h, w, _ = base.shape
    marks = marks_for(n, K)
    ctx = G.ctx()
    assert ctx.transform_plan(n, w, h)["fused_cols"], "the fused forward transform must be the path under test"
    if derived is None:
        derived = embedded(base, marks) if cfg is None else G.batch_embed(base, marks, cfg)["rgb"]
    ctx.reset_timing()
    on = G.batch_extract(base, derived, K, marks, cfg)
    st = ctx.prune_stats()
    with tuning(base_energy_lowp=0):
        ctx.reset_timing()
        exact = G.batch_extract(base, derived, K, marks, cfg)
        st_exact = ctx.prune_stats()
    with tuning(base_prune=0):
        ctx.reset_timing()
        off = G.batch_extract(base, derived, K, marks, cfg)
        assert ctx.prune_stats()["base_tiles"] == 0
    assert st_exact["base_tail_jobs"] == 0, st_exact
    for other, what in ((exact, "base_energy_lowp = 0"), (off, "base_prune = 0")):
        assert on[0].tobytes() == other[0].tobytes(), f"extracted marks differ from {what}"
        assert on[1].tobytes() == other[1].tobytes(), f"similarities differ from {what}"
    return on, st, st_exact, derived, marks


def tail_jobs(st, n, tiles_per_frame):
    """Tail jobs of one pass over the n base frames (a chunk redone with the full derived transform runs its base frames
    again: the counters then hold two passes, as in test_base_prune_gpu.routes)."""
    passes = st["base_tiles"] // (n * tiles_per_frame)
    assert passes in (1, 2) and st["base_tail_jobs"] % passes == 0, st
    return st["base_tail_jobs"] // passes


def bounds_both_routes(base, lay, ordering=L.ORDER_ENERGY, head=None, coef=None):
    """check_bound under both routes (ssw_debug_base_prune_bound >= the largest key of each column); the head's columns carry
    the exact energies.  `head`: the columns fed by head pairs only (default: those of this module's three layouts).  With
    64-pair tiles (W = 2048, and W = 1152 under tile48 = 0) they are compared bit for bit: two waves add into a block's total
    and two blocks into a frame's, both commutative.  The 48-pair tiles of W = 1152 under the default tiling add four waves'
    parts in the order they arrive (LDS atomics), on either route: there the head is compared within what that reordering can
    move -- per route three additions of the four parts, the addition of the two blocks and the product with G, each 2^-24 of
    a positive sum: 2 * 5 * 2^-24 relative.  A frame of more than 256 (padded) lines has more than two 128-line blocks, whose
    totals arrive in any order too: blocks - 1 additions per route instead of the one, with either tile width (H = 256: the
    rules above, unchanged).  Tail bounds lie above the exact energies up to the reordering of the exact route's H = 256 terms
    (2 * 256 * 2^-24).  `coef`: the reference plane check_bound compares with, instead of the library's own."""
    assert base.shape[2] == lay[0]
    lowp = check_bound(base, K, ordering, coef)
    with tuning(base_energy_lowp=0):
        exact = check_bound(base, K, ordering, coef)
    if head is None:
        head = 128 * (FIRST_TAIL_TILE[lay] - 1)            # every column below is fed by head pairs only
    tw = tail_layout(*lay).tw
    blocks = (base.shape[1] // 16 + 7) // 8                # 128-line blocks per frame: the units padded to whole blocks
    additions = (3 if tw == 48 else 0) + (blocks - 1) + 1
    if tw == 64 and blocks <= 2:
        assert lowp[:, :head].tobytes() == exact[:, :head].tobytes(), "head bounds differ from the exact route"
    else:
        a, b = lowp[:, :head], exact[:, :head]
        assert np.array_equal(np.isfinite(a), np.isfinite(b))
        ok = np.isfinite(a)
        assert np.all(np.abs(a[ok] - b[ok]) <= np.float32(2 * additions * 2.0 ** -24) * np.abs(b[ok])), "head bounds differ from the exact route"
    fin = np.isfinite(exact) & np.isfinite(lowp)
    assert np.all(lowp[fin] >= exact[fin] * np.float32(1 - 2.0 ** -15)), "a tail bound below the exact energy's"
    assert not np.any(np.isfinite(lowp) & ~np.isfinite(exact)), "a finite bound where the exact energy is not"
    return lowp, exact


@pytest.fixture(params=LAYOUTS, ids=lay_id)
def lay(request):
    with layout(request.param):
        yield request.param


def only(*lays):
    return pytest.mark.parametrize("lay", lays, ids=lay_id, indirect=True)


def test_smooth_frames_run_no_tail_job(lay):
    w = lay[0]
    n, base = frames_of(w)
    on, st, st_exact, derived, marks = run_three(base)
    assert routes(st, n, w // 128) == (n, 0) and st["base_tail_jobs"] == 0, st
    assert routes(st_exact, n, w // 128) == (n, 0), st_exact
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay)


# (under tile48 = 0 the first tail tile of W = 1152 is its last tile)
@pytest.mark.parametrize("lay, where", [(NARROW, "last tile"), (W48, "last tile"), (W48, "first tail tile"), (WIDE, "last tile"),
                                        (WIDE, "first tail tile")], ids=lambda v: lay_id(v) if isinstance(v, tuple) else v, indirect=["lay"])
def test_cosine_in_a_tail_tile_runs_the_tail_of_its_frames_only(lay, where):
    w = lay[0]
    n, base = frames_of(w)
    tile = w // 128 - 1 if where == "last tile" else FIRST_TAIL_TILE[lay]
    base[1::2] = with_cosine(base[1::2], 128 * tile + 37)
    hit = len(base[1::2])
    on, st, st_exact, derived, marks = run_three(base)
    assert routes(st, n, w // 128) == (n + hit, hit), st
    assert routes(st_exact, n, w // 128) == (n + hit, hit), st_exact
    assert st["base_tail_jobs"] == 8 * hit, st
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay)


def test_one_frame_in_the_middle(lay):
    """The line tiles of the frames around it must not run (or must not matter): one frame's jobs, the same bytes."""
    w = lay[0]
    n, base = frames_of(w)
    mid = n // 2
    base[mid:mid + 1] = with_cosine(base[mid:mid + 1], w - 20)
    on, st, _, derived, marks = run_three(base)
    assert routes(st, n, w // 128) == (n + 1, 1) and st["base_tail_jobs"] == 8, st
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay)


def test_white_noise_runs_every_tail_job(lay):
    w = lay[0]
    n, _ = frames_of(w)
    base = noise(n, H, w, 12)
    on, st, _, derived, marks = run_three(base)
    assert routes(st, n, w // 128) == (n * (w // 128), n) and tail_jobs(st, n, w // 128) == 8 * n, st
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay)


def test_tiny_frames(lay):
    """Frames scaled by 1e-6: the absolute terms of the bound (halves flushed in f16) weigh more; the bytes are the same."""
    w = lay[0]
    n, base = frames_of(w)
    base = (base * np.float32(1e-6)).astype(np.float32)
    base[1::2] = (with_cosine(base[1::2] * np.float32(1e6), w - 20) * np.float32(1e-6)).astype(np.float32)
    on, st, _, derived, marks = run_three(base)
    assert tail_jobs(st, n, w // 128) >= 8 * len(base[1::2]), st
    bounds_both_routes(base, lay)


def test_frames_beyond_the_f16_range_need_everything(lay):
    """Frames scaled by 3e4: the sixteen-fold sums of class R1+ R1- pass 65504, their bounds are Inf / NaN in every tail tile."""
    w = lay[0]
    n, base = frames_of(w)
    base = (base * np.float32(3e4)).astype(np.float32)
    on, st, st_exact, derived, marks = run_three(base)
    assert tail_jobs(st, n, w // 128) == 8 * n, st
    assert routes(st, n, w // 128)[1] == n, st
    lowp, exact = bounds_both_routes(base, lay)
    assert not np.isfinite(lowp[:, 128 * FIRST_TAIL_TILE[lay]:]).all()


def test_constant_frames_and_nan_and_inf_pixels(lay):
    w = lay[0]
    n, base = frames_of(w)
    base[0] = 0.5
    base[1, 10, 300, 0] = np.nan
    base[2, 20, 20, 1] = np.inf
    derived = with_cosine(base, 7, 0.01)
    on, st, _, _, _ = run_three(base, derived=derived)
    assert tail_jobs(st, n, w // 128) == 8 * 3, st         # no positive k-th key | NaN energies: every tile of those frames
    const = np.full((n, H, w, 3), 0.5, np.float32)
    on, st, _, _, _ = run_three(const)
    assert tail_jobs(st, n, w // 128) == 8 * n, st
    bounds_both_routes(const, lay)


@only(WIDE)
def test_energy_orthogonal(lay):
    w = lay[0]
    n, base = frames_of(w)
    base[::2] = with_cosine(base[::2], w - 20)
    cfg = G.default_config(ordering=L.ORDER_ENERGY_ORTHOGONAL)
    on, st, _, _, _ = run_three(base, cfg)
    assert st["base_tail_jobs"] == 8 * len(base[::2]), st
    bounds_both_routes(base, lay, L.ORDER_ENERGY_ORTHOGONAL)


@only(NARROW, W48)
def test_three_chunks_on_two_lanes(lay):
    w = lay[0]
    n, base = frames_of(w)
    base = np.concatenate([base, with_cosine(base, w - 20), base])
    ctx = G.ctx()
    ctx.set_chunk_frames(n)
    try:
        on, st, _, _, _ = run_three(base)
        assert routes(st, 3 * n, w // 128) == (3 * n + n, n) and st["base_tail_jobs"] == 8 * n, st
        bounds_both_routes(base, lay)
    finally:
        ctx.set_chunk_frames(0)


def test_unmerged_launches():
    """The default merge_max_lines, as in the 4K benchmark: eight head launches, eight gated tail launches."""
    w, n = W48[0], 112
    few = smooth(8, H, w, 17)
    few[1::2] = with_cosine(few[1::2], w - 20)
    base = np.ascontiguousarray(np.tile(few, (n // 8, 1, 1, 1)))
    with tuning(merge_max_lines=8192), G.fresh_ctx():
        on, st, _, derived, marks = run_three(base)
        assert routes(st, n, w // 128) == (n + n // 2, n // 2) and st["base_tail_jobs"] == 8 * (n // 2), st
        bounds_both_routes(base, W48)
    check_oracle(base, derived, marks, on)


def test_sums_of_more_than_256_terms_keep_the_exact_launches():
    """W = 4224: the row classes sum 264 terms, more than the tail bound takes ("Why W <= 4096": its accumulation
    term grows with the sum length).  White noise needs every tile: the route with the bound would run every tail job; the
    eight full energy launches run none, and base_energy_lowp changes neither a byte nor a counter."""
    w = 4224
    n = fused_batch(w)
    base = noise(n, H, w, 3)
    on, st, st_exact, _, _ = run_three(base)
    assert routes(st, n, w // 128) == (n * (w // 128), n) and st["base_tail_jobs"] == 0, st
    assert st == st_exact


def test_stale_column_operands_are_never_read():
    """One context: a batch of NaN frames first, then smooth frames with a cosine in the last tile of every other frame.  The
    NaN batch needs every tile and leaves NaN in every column-operand plane, in the coefficient plane and in the energies,
    and a set flag in every entry of the need buffer: the second call's tail launches run for its own frames' flags only
    (the job counter) and write what phase 2 reads."""
    w = WIDE[0]
    n, base = frames_of(w)
    base[1::2] = with_cosine(base[1::2], w - 20)
    marks = marks_for(n, K)
    derived = embedded(base, marks)
    dirty = np.full(base.shape, np.nan, np.float32)
    with G.fresh_ctx() as ctx:
        G.batch_extract(dirty, dirty, K, marks)
        assert ctx.prune_stats()["base_tail_jobs"] >= 8 * n            # (twice that where the chunk is redone with the full derived transform)
        ctx.reset_timing()
        on = G.batch_extract(base, derived, K, marks)
        st = ctx.prune_stats()
        G.batch_extract(dirty, dirty, K, marks)
        bounds_both_routes(base, WIDE)
    assert st["base_tail_jobs"] == 8 * len(base[1::2]), st
    with tuning(base_prune=0), G.fresh_ctx():
        off = G.batch_extract(base, derived, K, marks)
    assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
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
    with tuning(base_energy_lowp=0):
        ext.zero_(); sims.zero_(); torch.cuda.synchronize()
        step(); ctx.synchronize()
        assert torch.equal(ext, want[0]) and torch.equal(sims, want[1]), "eager differs from base_energy_lowp = 0"
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
    assert (st["base_tiles_computed"], st["base_frames_extended"], st["base_tail_jobs"]) == (n + n // 2, n // 2, 8 * (n // 2)), st
    print("graph-ok")
    ctx.set_stream(None); ctx.close()
"""


def test_captured_into_a_graph_and_replayed(tmp_path):
    """ssw_batch_extract with the tail bound captured into a HIP graph (the bound kernel, the head launches, the decide kernel
    and the gated tail launches are nodes; no host wait, no redo) and replayed once: byte-equal to the eager call and to
    base_energy_lowp = 0, counters of exactly one pass."""
    w = W48[0]
    n, base = frames_of(w)
    n -= n % 2
    base = base[:n]
    assert G.ctx().transform_plan(n, w, H)["fused_cols"]
    base[1::2] = with_cosine(base[1::2], w - 20)
    np.save(tmp_path / "base.npy", base)
    script = tmp_path / "graph_check.py"
    script.write_text(_GRAPH_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, str(script), root, str(tmp_path / "base.npy")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "graph-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
