"""The tail bound of the base reader and its gated row launches (csrc/base_energy.hip, the SUB == 5 block of
dct_pair_f64_kernel.hpp) at the layouts tests/test_base_energy_gpu.py does not reach: more than one tail tile
column per class, a full block of the bound kernel (11 MFMA pair tiles) and a second chunk, eight k-steps, and frames whose
last 128-line tile is mostly padding.  H = 256 (272 for the padded units), k = 64, the smallest batch that takes the fused
forward transform.

    W     tile48  pairs  tile columns        tail  MFMA tiles x chunks  Kp   column tiles  seam tiles
    2176  1       136    48 + 48 + 40        88    6 (last half) x 1    136  17            5, 11
    2176  0       136    64 + 64 + 8         72    5 x 1                136  17            7, 15
    3840  1       240    64 + 64 + 64 + 48   176   11 x 1               240  30            7, 15, 23
    4096  1       256    64 x 4              192   11 + 1: 2 chunks     256  32            7, 15, 23

tests/tail_layout.py restates the layout and tests/test_tail_layout_cpu.py binds it to pair_class_args on the host; every
expected counter here comes from it.  A job is (frame, class, tail tile column).  Away from a seam a needed column tile runs
the eight classes of its one tile column.  A seam tile -- the last column tile that tile column tn - 1 feeds -- also holds
the second output of the first pair of tile column tn in every class of E's shape (e2off = 1).  The level-2 row pass has FIVE
such classes (R2 rotated, AS2 BD2, AS+ BD-, both rotations of O), not the one a reading of "class E" suggests: a needed seam
tile costs 8 [tn >= 2] + 5 jobs per frame, which is what the seam sweep asserts.

Every equality is byte equality with base_energy_lowp = 0 and with base_prune = 0 (run_three); the only bars are those of
check_oracle and bounds_both_routes.  Each counter test prints the measured base_tail_jobs beside the expected ones."""
import numpy as np
import pytest

import gpu_util as G
import tail_layout as T
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import tuning
from test_base_energy_gpu import bounds_both_routes, embedded, fused_batch, lay_id, layout, run_three, tail_jobs
from test_base_prune_gpu import FUSED, check_oracle, marks_for, noise, routes, with_cosine

pytestmark = pytest.mark.gpu

H, HPAD, K = 256, 272, 64
A48, A64, UHD, MAXW = (2176, 1), (2176, 0), (3840, 1), (4096, 1)
LAYOUTS = [A48, A64, UHD, MAXW]


@pytest.fixture(scope="module", autouse=True)
def fused_settings():
    with tuning(**FUSED), G.fresh_ctx():
        yield


@pytest.fixture(params=LAYOUTS, ids=lay_id)
def lay(request):
    with layout(request.param):
        yield request.param


def only(*lays):
    return pytest.mark.parametrize("lay", lays, ids=lay_id, indirect=True)


_frames = {}


def batch_of(w, h):
    """The smallest batch whose forward transform is the fused one (run_three asserts it where it runs)."""
    if h == H:
        return fused_batch(w)
    ctx = G.ctx()
    return next(i for i in range(1, 65) if ctx.transform_plan(i, w, h)["fused_cols"])


def frames_of(w, h=H, n=None):
    """(n, smooth frames), computed once per shape."""
    n = n or batch_of(w, h)
    if (w, h, n) not in _frames:
        _frames[(w, h, n)] = T.smooth_like(n, h, w, 31 + w + h)
    return n, _frames[(w, h, n)].copy()


def at(tile):
    return 128 * tile + 37


def check_counters(what, lay, st, st_exact, needs):
    """needs[f]: the column tiles beyond tile 0 that frame f must need.  Tiles computed, frames extended and tail jobs, all from
    tests/tail_layout.py."""
    t = T.tail_layout(*lay)
    n = len(needs)
    want = (n + sum(len(set(s)) for s in needs), sum(1 for s in needs if s))
    jobs = sum(len(T.jobs(t, s)) for s in needs)
    got = tail_jobs(st, n, t.column_tiles)
    print(f"JOBS {lay_id(lay)} {what}: {n} frames, base_tail_jobs measured {got}, expected {jobs}; tiles computed / frames extended "
          f"measured {routes(st, n, t.column_tiles)}, expected {want}")
    assert routes(st, n, t.column_tiles) == want, st
    assert routes(st_exact, n, t.column_tiles) == want, st_exact
    assert got == jobs, st


def tile_cases():
    """(layout, tail tile column, tile): the first and the last column tile that only that tile column feeds."""
    out = []
    for lay in LAYOUTS:
        t = T.tail_layout(*lay)
        for tn in range(1, len(t.tile_cols)):
            own = T.own_tiles(t, tn)
            out += [pytest.param(lay, tn, tile, id=f"{lay_id(lay)}-tn{tn}-tile{tile}") for tile in sorted({own[0], own[-1]})]
    return out


# ---- 2. a needed tile in every tail tile column, and two at once

@pytest.mark.parametrize("lay, tn, tile", tile_cases(), indirect=["lay"])
def test_cosine_in_one_tail_tile_column_runs_that_tile_column_only(lay, tn, tile):
    w = lay[0]
    n, base = frames_of(w)
    base[1::2] = with_cosine(base[1::2], at(tile))
    on, st, st_exact, derived, marks = run_three(base)
    needs = [[tile] if f % 2 else [] for f in range(n)]
    assert T.jobs(T.tail_layout(*lay), [tile]) == [(c, tn) for c in range(8)]
    check_counters(f"cosine in tile {tile} (tile column {tn})", lay, st, st_exact, needs)
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay, head=T.head_width(T.tail_layout(*lay)))


def test_two_cosines_in_one_frame_first_and_last_tail_tile_column(lay):
    w, t = lay[0], T.tail_layout(*lay)
    n, base = frames_of(w)
    first, last = T.own_tiles(t, 1)[0], T.own_tiles(t, len(t.tile_cols) - 1)[-1]
    base[1::2] = with_cosine(with_cosine(base[1::2], at(first)), at(last))
    on, st, st_exact, derived, marks = run_three(base)
    needs = [[first, last] if f % 2 else [] for f in range(n)]
    assert len(T.jobs(t, [first, last])) == 16
    check_counters(f"cosines in tiles {first} and {last}", lay, st, st_exact, needs)
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay, head=T.head_width(t))


def test_frames_of_one_batch_need_different_tile_columns(lay):
    """Frame i needs tile column 1 + i mod (tile columns - 1)."""
    w, t = lay[0], T.tail_layout(*lay)
    n, base = frames_of(w)
    needs = []
    for f in range(n):
        own = T.own_tiles(t, 1 + f % (len(t.tile_cols) - 1))
        needs.append([own[len(own) // 2]])
        base[f:f + 1] = with_cosine(base[f:f + 1], at(needs[-1][0]))
    on, st, st_exact, derived, marks = run_three(base)
    check_counters("a tile column per frame", lay, st, st_exact, needs)
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay, head=T.head_width(t))


# ---- 3. the seams, column by column

def cosine_sweep(frame, cols, amp=0.1):
    """with_cosine(frame, col, amp) for every col of `cols`, one frame each (the same arithmetic, one pass)."""
    h, w, _ = frame.shape
    x, y = np.arange(w)[None, :], np.arange(h)
    cx = amp * np.cos(np.pi * (2 * x + 1) * np.asarray(cols)[:, None] / (2 * w))
    c = cx[:, None, :] * np.cos(np.pi * (2 * y + 1) * 3 / (2 * h))[None, :, None]
    out = np.empty((len(cols), h, w, 3), np.float32)
    for ch in range(3):
        out[..., ch] = np.clip(frame[None, :, :, ch] + c, 0.0, 1.0)
    return out


def seam_cases():
    return [pytest.param(lay, tn, seam, first, id=f"{lay_id(lay)}-seam{seam}-from{first}")
            for lay in (A48, UHD) for tn, seam in enumerate(T.seam_tiles(T.tail_layout(*lay)), 1) for first in range(0, 128, 32)]


@pytest.mark.parametrize("lay, tn, seam, first", seam_cases(), indirect=["lay"])
def test_every_frequency_of_a_seam_tile(lay, tn, seam, first):
    """One smooth frame with a cosine at each of the seam tile's 128 frequencies, 32 frames per call (and case), four calls per
    seam tile.  The flags are per tile:
    whichever frequency raised it, the tile column below (when it is a tail one) and the one entry of the E-shaped classes of
    tile column tn must run; a gate that misses that entry leaves a column-operand line stale and the bytes differ."""
    w, t = lay[0], T.tail_layout(*lay)
    _, one = frames_of(w, H, 1)
    per_frame = 8 * (tn >= 2) + sum(T.E_SHAPED)
    assert len(T.jobs(t, [seam])) == per_frame
    assert cosine_sweep(one[0], [128 * seam + first]).tobytes() == with_cosine(one, 128 * seam + first).tobytes()
    base = cosine_sweep(one[0], 128 * seam + first + np.arange(32))
    on, st, st_exact, _, _ = run_three(base, derived=with_cosine(base, 7, 0.01))
    check_counters(f"seam tile {seam}, frequencies {first} .. {first + 31}", lay, st, st_exact, [[seam]] * 32)


# ---- 4. the bound kernel at full width

@only(UHD, MAXW)
def test_white_noise_every_tail_column_bounded_and_none_left_at_zero(lay):
    w, t = lay[0], T.tail_layout(*lay)
    n = batch_of(w, H)
    base = noise(n, H, w, 12)
    on, st, st_exact, derived, marks = run_three(base)
    check_counters("white noise", lay, st, st_exact, [list(range(1, t.column_tiles))] * n)
    check_oracle(base, derived, marks, on)
    lowp, exact = bounds_both_routes(base, lay, head=T.head_width(t))
    assert np.all(exact > 0), "white noise has energy in every column"
    assert np.all(lowp > 0), "a tail column without a bound: a chunk or a pair tile added nothing"


@only(UHD, MAXW)
def test_smooth_and_cosine_frames_bounds_at_full_width(lay):
    w, t = lay[0], T.tail_layout(*lay)
    n, base = frames_of(w)
    for f in range(n):
        base[f:f + 1] = with_cosine(base[f:f + 1], 128 * (1 + (f * 5) % (t.column_tiles - 1)) + 11 * f)
    assert G.ctx().transform_plan(n, w, H)["fused_cols"]
    bounds_both_routes(base, lay, head=T.head_width(t))


def row_patterns(w):
    """The row patterns of tests/test_base_energy_cpu.py::lines(), W samples long."""
    rng = np.random.default_rng(7)
    i = np.arange(w)
    return {"alternating": np.where(i % 2 == 0, 1.0, -1.0), "spike": np.where(i == 17, 1.0, 0.0),
            "1e-7": 1e-7 * rng.choice([-1.0, 1.0], w), "6e4": 6e4 * rng.choice([-1.0, 1.0], w),
            "dc dwarfs detail": 1000.0 + 1e-3 * rng.standard_normal(w), "noise": rng.standard_normal(w)}


def rows_frame(p):
    return np.ascontiguousarray(np.broadcast_to(p.astype(np.float32)[None, :, None], (H, p.size, 3)))


def oracle_plane(frames):
    """The oracle's coefficient planes [n, h, w], every coefficient moved toward zero by the oracle's own error: check_bound asks
    bound >= key without a bar, and where the true coefficient is exactly 0 (the even frequencies of alternating +-1 rows) the
    library's exact launches give energy 0 and bound 0, while the oracle's f64 FFT leaves its rounding noise (3e-11 beside
    coefficients of 8e5).  An FFT of N points has a normwise error of at most log2(N) eps ||X||_2, so no coefficient of the
    2-D transform is off by more than (log2(2 W) + log2(2 H)) 2^-53 ||plane||_2; four times that (the twiddles before and
    after the FFT that make it a DCT) is taken off every |coefficient|.  At these frames that is 1e-8 or less beside
    coefficients of 1e5 and more: the keys that decide anything keep 13 digits."""
    out = []
    for fr in frames:
        c = O.dct2d(O.rgb_to_yiq(fr)[0]).astype(np.float64)
        h, w = c.shape
        delta = 4.0 * (np.log2(2 * w) + np.log2(2 * h)) * 2.0 ** -53 * np.sqrt((c * c).sum())
        out.append(np.sign(c) * np.maximum(np.abs(c) - delta, 0.0))
    return np.stack(out).astype(np.float32)


@only(UHD, MAXW)
def test_adversarial_rows_on_the_device(lay):
    """Each pattern as the rows of one frame (three equal channels, nothing clipped), the batch filled up with smooth frames.
    The bounds are checked against the oracle's plane of these frames (oracle_plane), not the library's."""
    w, t = lay[0], T.tail_layout(*lay)
    n, base = frames_of(w)
    pats = row_patterns(w)
    assert len(pats) <= n
    for f, p in enumerate(pats.values()):
        base[f] = rows_frame(p)
    with np.errstate(all="ignore"):
        coef = oracle_plane(base)
    lowp, exact = bounds_both_routes(base, lay, head=T.head_width(t), coef=coef)
    f6 = list(pats).index("6e4")
    for tile in range(t.tw // 8, t.column_tiles):
        assert not np.isfinite(lowp[f6, 128 * tile:128 * (tile + 1)]).all(), f"tile {tile} of the 6e4 frame has finite bounds only"
    run_three(base)


@only(UHD, MAXW)
def test_rows_beyond_the_f16_range_need_everything(lay):
    """A batch of 6e4 * +-1 rows: sums of sixteen pass 65504, the bounds are Inf / NaN, every tail job of every frame runs."""
    w, t = lay[0], T.tail_layout(*lay)
    n = batch_of(w, H)
    rng = np.random.default_rng(9)
    base = np.stack([rows_frame(6e4 * rng.choice([-1.0, 1.0], w)) for _ in range(n)])
    on, st, st_exact, _, _ = run_three(base)
    check_counters("6e4 rows", lay, st, st_exact, [list(range(1, t.column_tiles))] * n)


@only(UHD)
def test_energy_orthogonal_at_full_width(lay):
    w, t = lay[0], T.tail_layout(*lay)
    n, base = frames_of(w)
    tile = T.own_tiles(t, 2)[0]
    base[::2] = with_cosine(base[::2], at(tile))
    cfg = G.default_config(ordering=L.ORDER_ENERGY_ORTHOGONAL)
    on, st, st_exact, _, _ = run_three(base, cfg)
    check_counters("energy-orthogonal", lay, st, st_exact, [[] if f % 2 else [tile] for f in range(n)])
    bounds_both_routes(base, lay, L.ORDER_ENERGY_ORTHOGONAL, head=T.head_width(t))


# ---- 5. padded units: H = 272 is 17 units padded to 24, the third 128-line tile of a frame holds one valid unit

@only(A48, UHD)
def test_padded_units_smooth_frames_run_no_tail_job(lay):
    w, t = lay[0], T.tail_layout(*lay)
    n, base = frames_of(w, HPAD)
    on, st, st_exact, derived, marks = run_three(base)
    check_counters("H = 272, smooth", lay, st, st_exact, [[]] * n)
    assert st["base_tail_jobs"] == 0, st
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay, head=T.head_width(t))


@only(A48, UHD)
def test_padded_units_cosine_in_the_last_tile(lay):
    w, t = lay[0], T.tail_layout(*lay)
    n, base = frames_of(w, HPAD)
    last = t.column_tiles - 1
    base[1::2] = with_cosine(base[1::2], at(last))
    on, st, st_exact, derived, marks = run_three(base)
    check_counters("H = 272, cosine in the last tile", lay, st, st_exact, [[last] if f % 2 else [] for f in range(n)])
    check_oracle(base, derived, marks, on)
    bounds_both_routes(base, lay, head=T.head_width(t))


@only(A48, UHD)
def test_padded_units_white_noise(lay):
    w, t = lay[0], T.tail_layout(*lay)
    n = batch_of(w, HPAD)
    base = noise(n, HPAD, w, 13)
    on, st, st_exact, derived, marks = run_three(base)
    check_counters("H = 272, white noise", lay, st, st_exact, [list(range(1, t.column_tiles))] * n)
    check_oracle(base, derived, marks, on)
    lowp, _ = bounds_both_routes(base, lay, head=T.head_width(t))
    assert np.all(lowp > 0)


@only(A48, UHD)
def test_padded_units_stale_column_operands_are_never_read(lay):
    """test_base_energy_gpu.test_stale_column_operands_are_never_read at H = 272: the NaN batch dirties every plane, padding
    lines included; the second call runs the jobs of its own flags only and reads nothing of the first."""
    w, t = lay[0], T.tail_layout(*lay)
    n, base = frames_of(w, HPAD)
    last = t.column_tiles - 1
    base[1::2] = with_cosine(base[1::2], at(last))
    marks = marks_for(n, K)
    derived = embedded(base, marks)
    dirty = np.full(base.shape, np.nan, np.float32)
    with G.fresh_ctx() as ctx:
        assert ctx.transform_plan(n, w, HPAD)["fused_cols"]
        G.batch_extract(dirty, dirty, K, marks)
        assert ctx.prune_stats()["base_tail_jobs"] >= 8 * (len(t.tile_cols) - 1) * n
        ctx.reset_timing()
        on = G.batch_extract(base, derived, K, marks)
        st = ctx.prune_stats()
        G.batch_extract(dirty, dirty, K, marks)
        bounds_both_routes(base, lay, head=T.head_width(t))
    want = sum(len(T.jobs(t, [last])) for _ in base[1::2])
    print(f"JOBS {lay_id(lay)} H = 272, after a NaN batch: base_tail_jobs measured {st['base_tail_jobs']}, expected {want}")
    assert st["base_tail_jobs"] == want, st
    with tuning(base_prune=0), G.fresh_ctx():
        off = G.batch_extract(base, derived, K, marks)
    assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
    check_oracle(base, derived, marks, on)


# ---- 6. stale operands between tile columns, and unmerged launches

def test_stale_operands_of_another_tile_column_are_never_read():
    """One context at 3840: call 1 makes every frame need a tile of tile column 3, call 2 (the same shapes) every other frame a
    tile of tile column 1 only.  Phase 2 of call 2 must read what call 2's gated launches wrote: 8 jobs per such frame, the
    bytes of base_prune = 0 on a fresh context."""
    w, t = UHD[0], T.tail_layout(*UHD)
    n, smooth = frames_of(w)
    t3, t1 = T.own_tiles(t, 3)[1], T.own_tiles(t, 1)[1]
    first = with_cosine(smooth, at(t3))
    base = smooth.copy()
    base[1::2] = with_cosine(base[1::2], at(t1))
    marks = marks_for(n, K)
    derived = embedded(base, marks)
    with G.fresh_ctx() as ctx:
        assert ctx.transform_plan(n, w, H)["fused_cols"]
        G.batch_extract(first, with_cosine(first, 7, 0.01), K, marks)
        st1 = ctx.prune_stats()
        assert tail_jobs(st1, n, t.column_tiles) == 8 * n and T.jobs(t, [t3]) == [(c, 3) for c in range(8)], st1
        ctx.reset_timing()
        on = G.batch_extract(base, derived, K, marks)
        st = ctx.prune_stats()
    want = len(T.jobs(t, [t1])) * len(base[1::2])
    print(f"JOBS {lay_id(UHD)} tile column 1 after tile column 3: base_tail_jobs measured {st['base_tail_jobs']}, expected {want}")
    assert T.jobs(t, [t1]) == [(c, 1) for c in range(8)] and st["base_tail_jobs"] == want, st
    assert routes(st, n, t.column_tiles) == (n + len(base[1::2]), len(base[1::2])), st
    with tuning(base_prune=0), G.fresh_ctx():
        off = G.batch_extract(base, derived, K, marks)
    assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
    check_oracle(base, derived, marks, on)


def test_unmerged_launches_over_three_tail_tile_columns():
    """merge_max_lines = 8192, the benchmark's launch mode, at 3840: eight head launches and eight gated tail launches, each over
    three tile columns.  The planner fuses such launches from 56 frames on (448 blocks of one class: 2 line tiles per frame x 4
    tile columns), so the batch is eight frames tiled seven times -- more than the 32 frames of the other cases."""
    w, t = UHD[0], T.tail_layout(*UHD)
    t2, t3 = T.own_tiles(t, 2)[2], T.own_tiles(t, 3)[2]
    _, few = frames_of(w, H, 8)
    few[0::4] = with_cosine(few[0::4], at(t2))
    few[2::4] = with_cosine(few[2::4], at(t3))
    with tuning(merge_max_lines=8192), G.fresh_ctx() as ctx:
        n = next(i for i in range(8, 129, 8) if ctx.transform_plan(i, w, H)["fused_cols"] and i * H > 8192)
        assert n == 56
        base = np.ascontiguousarray(np.tile(few, (n // 8, 1, 1, 1)))
        needs = [[t2] if f % 4 == 0 else [t3] if f % 4 == 2 else [] for f in range(n)]
        on, st, st_exact, derived, marks = run_three(base)
        check_counters("unmerged launches", UHD, st, st_exact, needs)
        bounds_both_routes(base, UHD, head=T.head_width(t))
    check_oracle(base, derived, marks, on)
