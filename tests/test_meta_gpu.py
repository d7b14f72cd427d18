"""Three properties the library documents or relies on, on every kernel family (tests/meta_cases.py: shapes D, P, L2, F, T):

1. exact scaling -- a frame multiplied by 2^e has every coefficient multiplied by 2^e bit for bit, the same index list, the
   same extracted mark (Options 2, 3; scaled under Option 1) and the same similarity, whatever its neighbours in the batch
   are scaled by;
2. isolation -- a frame, mark or suspect poisoned with NaN, +-Inf, 3e38 or (8 / 16 bit) a flat frame changes no byte of any
   other frame's output, in either precision;
3. history -- a context that has processed such frames answers later clean calls, on the same and on narrower shapes,
   byte for byte like a fresh context.

Every expected value is exact: the same call on the clean batch, the unscaled call times 2^e, or a fresh context.  The clean
batches themselves are held to the oracle on frame 0 with the project's bars, so that "equal to the clean call" is not a
comparison of the library with itself only; tests/test_meta_cpu.py pins the oracle's side of every property.  Every test
asserts the plan flags of its shape.  Poisoned outputs are looked at only through np.isnan.  Everything goes through the C ABI."""
import contextlib

import numpy as np
import pytest

import gpu_util as G
import meta_cases as M
import spread_spectrum_watermarking_amd as wm
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd.api import tuning
from test_base_prune_gpu import FUSED
from test_config_matrix_gpu import LEVEL2, _derived_row_launches
from test_trace_gpu import NONE, trace

pytestmark = pytest.mark.gpu
marks_of = M.marks_of

F32, F64 = L.PRECISION_F32, L.PRECISION_F64
E, EO, LG = L.ORDER_ENERGY, L.ORDER_ENERGY_ORTHOGONAL, L.ORDER_LEGACY
O1, O2, O3 = L.OPTION1, L.OPTION2, L.OPTION3
ORDERINGS = (E, EO, LG)
DCT_TYPES = (L.DCT2, L.DCT2_ORTHOGONAL, L.DCT3)
TUNINGS = {None: {}, "LEVEL2": LEVEL2, "FUSED": FUSED}
# A NaN pixel gives an all-NaN coefficient plane, in the oracle and here.  (A +-Inf pixel does in the oracle, whose FFT
# multiplies it by twiddles of both signs; the basis GEMMs leave +-Inf where a column's basis entries keep one sign.  What a
# poisoned frame itself yields beyond the NaN case is not pinned.)
NAN_KINDS = ("nan_last", "all_nan")
PRUNED = ("P", "L2", "F")          # shapes whose batch extract takes the pruned derived transform
# every poison kind on P and L2, kinds (a) and (e) on every shape
FRAME_CASES = [(s, k) for s in ("P", "L2") for k in M.FRAME_POISONS] + [(s, k) for s in ("D", "F", "T") for k in ("nan_last", "all_3e38")]
_id = lambda v: {F32: "f32", F64: "f64"}.get(v, str(v)) if isinstance(v, int) else str(v)


@contextlib.contextmanager
def shape_ctx(name, chunk=None):
    """A fresh context under the shape's tuning, its chunk size set, its plan asserted."""
    s = M.SHAPES[name]
    with tuning(**TUNINGS[s["tuning"]]), G.fresh_ctx() as ctx, np.errstate(all="ignore"):
        ctx.set_chunk_frames(s["chunk"] if chunk is None else chunk)
        for n in {s["chunk"], s["n"] % s["chunk"]}:          # the full chunks and the ragged one
            plan = ctx.transform_plan(n, s["w"], s["h"])
            assert {f: plan[f] for f in s["plan"]} == s["plan"], (name, n, plan)
        yield ctx, s


def frames_of(name):
    return M.frames_of(name, O.synth_frame)


def cfg_of(precision=F64, ordering=E, method=O2):
    return G.default_config(precision, ordering, method)


def pipelines(rgb, marks, cfg, derived=None):
    """ssw_batch_embed (marked frames, coefficient planes, index lists) and ssw_batch_extract of `derived` (default: the
    marked frames of this call) against `rgb`."""
    e = G.batch_embed(rgb, marks, cfg, want_coef=True, want_idx=True)
    ext, sims = G.batch_extract(rgb, e["rgb"] if derived is None else derived, marks.shape[1], marks, cfg)
    return {"marked": e["rgb"], "coef": e["coef"], "idx": e["idx"], "ext": ext, "sims": sims}


def assert_isolated(clean, got, j, what):
    for key in clean:
        diff = M.others_same(clean[key], got[key], j)
        assert diff == [], f"{what}: poison in frame {j} changed `{key}` of frames {diff}"


def stats(ctx):
    return {**ctx.select_stats(), **ctx.prune_stats()}


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


_CLEAN = {}


def clean_ref(name, precision):
    """The clean batch of a shape and what the batch pipelines give on it: computed once per shape and precision on a fresh
    context of its own under the shape's tuning and chunking -- whichever test asks first, and whatever that test set on its
    own context -- and never changed.  Canonical precision: frame 0 against the oracle with the project's bars."""
    if (name, precision) not in _CLEAN:
        with shape_ctx(name) as (ctx, s):
            _CLEAN[(name, precision)] = _clean_ref(name, precision, ctx, s)
    return _CLEAN[(name, precision)]


def _clean_ref(name, precision, ctx, s):
    frames, marks = frames_of(name), marks_of(name)
    before = stats(ctx)
    out = pipelines(frames, marks, cfg_of(precision))
    d = delta(stats(ctx), before)
    if precision == F64:
        assert (d["pruned_chunks"] > 0 and d["redone_chunks"] == 0) if name in PRUNED else d["pruned_chunks"] == 0, (name, d)
        if name == "F":         # the two-phase base prune ran, skipped tiles, and extended some frames
            assert d["base_tiles"] == 3 * s["n"] and s["n"] < d["base_tiles_computed"] < d["base_tiles"] and d["base_frames_extended"] > 0, d
    assert all(np.all(np.isfinite(v)) for v in out.values())
    if precision == F64:
        ref_coef = O.dct2d(O.rgb_to_yiq(frames[0])[0])
        assert np.abs(out["coef"][0].astype(np.float64) - ref_coef).max() <= 2e-7 * np.abs(ref_coef.reshape(-1)[1:]).max()
        assert np.array_equal(out["idx"][0], O.indices(ref_coef, O.ORDER_ENERGY, s["k"]).astype(np.uint32))
        G.assert_f32_bars(out["marked"][0], O.embed_frame(frames[0], marks[0]), identical=0.999, what=name)
        o_ext, o_sim = O.extract_frame(frames[0], out["marked"][0], marks[0])
        assert G.ext_within_1e5(out["ext"][0], o_ext), name
        assert abs(float(out["sims"][0]) - o_sim) < 1e-4 * max(1.0, abs(o_sim)), (name, out["sims"][0], o_sim)
    return dict(frames=frames, marks=marks, out=out)


# ---- group 1: exact scaling -------------------------------------------------------------------------------------------------
def plane_calls(rgb, k, precision=F64):
    """ssw_rgb_to_yiq, ssw_dct2d of the Y plane (three types), ssw_topk_indices of the DCT-II plane (three orderings)."""
    y, i, q = G.rgb_to_yiq(rgb)
    out = {"y": y, "i": i, "q": q}
    for t in DCT_TYPES:
        out[f"dct{t}"] = G.dct2d(y, t, precision)
    for o in ORDERINGS:
        out[f"idx{o}"] = G.topk(out[f"dct{L.DCT2}"], k, o)
    return out


def assert_scaled(unscaled, got, exps, what, scale=True):
    for i, e in enumerate(exps):
        want = unscaled[i] * M.pow2(e) if scale else unscaled[i]
        assert M.same_bits(got[i], want), f"{what}: frame {i} (2^{e}) is not {'2^e times ' if scale else ''}the unscaled call's"


@pytest.mark.parametrize("name", list(M.SHAPES))
def test_scaling_by_powers_of_two_is_exact(name):
    with shape_ctx(name) as (ctx, s):
        ref = clean_ref(name, F64)
        frames, marks, k = ref["frames"], ref["marks"], s["k"]
        exps = M.cycle_exps(s["n"])
        big = M.scaled(frames, exps)
        a, b = plane_calls(frames, k), plane_calls(big, k)
        for key in a:
            assert_scaled(a[key], b[key], exps, key, scale=not key.startswith("idx"))
        before = stats(ctx)
        e = G.batch_embed(big, marks, cfg_of(), want_coef=True, want_idx=True)
        assert_scaled(ref["out"]["coef"], e["coef"], exps, "ssw_batch_embed coef")
        assert_scaled(ref["out"]["idx"], e["idx"], exps, "ssw_batch_embed idx", scale=False)
        for ordering, method in ((E, O2), (EO, O1), (LG, O3)):
            for kk in (k, M.K_GATHERED) if name == "L2" else (k,):
                cfg, m = cfg_of(F64, ordering, method), marks_of(name, kk)
                derived = G.batch_embed(frames, m, cfg)["rgb"]
                ext, sims = G.batch_extract(frames, derived, kk, m, cfg)
                mid = stats(ctx)
                ext_s, sims_s = G.batch_extract(big, M.scaled(derived, exps), kk, m, cfg)
                # the counters may differ between the scales (recorded); the results may not
                print(f"{name} ordering {ordering} method {method} k {kk}: unscaled {delta(mid, before)} scaled {delta(stats(ctx), mid)}")
                before = stats(ctx)
                assert np.all(np.isfinite(sims)), (ordering, method)
                assert_scaled(ext, ext_s, exps, f"extracted, method {method}, k {kk}", scale=method == O1)
                assert_scaled(sims, sims_s, exps, f"similarity, method {method}, k {kk}", scale=False)


@pytest.mark.parametrize("k, fused", [(M.SHAPES["L2"]["k"], True), (M.K_GATHERED, False)], ids=["fused-derived", "gathered-launches"])
def test_l2_reaches_both_pruned_row_passes(k, fused):
    """The route of shape L2 (see test_config_matrix_gpu.test_landscape_level2): the derived frame's row pass in one kernel at
    k = 600, as gathered launches at k = 1056."""
    with shape_ctx("L2") as (ctx, s):
        full, _ = _derived_row_launches(ctx, s["h"], s["w"], s["chunk"], k, cfg_of(), False)
        pruned, st = _derived_row_launches(ctx, s["h"], s["w"], s["chunk"], k, cfg_of(), True)
        assert st["pruned_chunks"] == 1 and st["redone_chunks"] == 0, st
        assert (2 * pruned == full) if fused else (2 * pruned > full), (pruned, full)


# ---- group 2: isolation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, kind", FRAME_CASES)
def test_plane_calls_isolate_a_poisoned_frame(name, kind):
    with shape_ctx(name) as (ctx, s):
        frames = clean_ref(name, F64)["frames"]
        for precision in (F64, F32):
            clean = plane_calls(frames, s["k"], precision)
            for j in s["poison_at"]:
                got = plane_calls(M.poison_batch(frames, j, kind), s["k"], precision)
                assert_isolated(clean, got, j, f"{_id(precision)} plane calls, {kind}")
                if kind in NAN_KINDS:
                    for t in DCT_TYPES:
                        assert np.all(np.isnan(got[f"dct{t}"][j])), (t, j)


@pytest.mark.parametrize("precision", [F64, F32], ids=_id)
@pytest.mark.parametrize("name, kind", FRAME_CASES)
def test_batch_pipelines_isolate_a_poisoned_frame(name, kind, precision):
    """ssw_batch_embed on a batch with one poisoned frame; ssw_batch_extract with a poisoned base frame, and with a poisoned
    derived frame."""
    with shape_ctx(name) as (ctx, s):
        ref = clean_ref(name, precision)
        frames, marks, clean, cfg = ref["frames"], ref["marks"], ref["out"], cfg_of(precision)
        for j in s["poison_at"]:
            got = pipelines(M.poison_batch(frames, j, kind), marks, cfg, derived=clean["marked"])
            assert_isolated(clean, got, j, f"poisoned base frame, {kind}")
            if kind in NAN_KINDS:
                assert np.all(np.isnan(got["coef"][j])), j
            ext, sims = G.batch_extract(frames, M.poison_batch(clean["marked"], j, kind), s["k"], marks, cfg)
            assert_isolated({"ext": clean["ext"], "sims": clean["sims"]}, {"ext": ext, "sims": sims}, j, f"poisoned derived frame, {kind}")


def _integer_entry_points(frames, marks, cfg, bits):
    embed, extract, to_int = ((G.batch_embed_rgb8, G.batch_extract_rgb8, O.f32_to_u8) if bits == 8 else
                              (G.batch_embed_rgb16, G.batch_extract_rgb16, O.f32_to_u16))
    return embed, extract, to_int(frames), to_int


@pytest.mark.parametrize("precision", [F64, F32], ids=_id)
@pytest.mark.parametrize("name", ["P", "L2", "D"])
def test_integer_pipelines_isolate_flat_frames_and_poisoned_marks(name, precision):
    """ssw_batch_embed / _extract and their _rgb8 / _rgb16 forms: flat frames (AC coefficients zero, Option 2 extraction 0 / 0)
    as base and as derived frame, and NaN, +-Inf and 3e38 entries in one frame's mark."""
    with shape_ctx(name) as (ctx, s):
        ref = clean_ref(name, precision)
        frames, marks, cfg, k, at = ref["frames"], ref["marks"], cfg_of(precision), s["k"], s["poison_at"]
        for bits in (8, 16):
            embed, extract, fr, to_int = _integer_entry_points(frames, marks, cfg, bits)
            marked = embed(fr, marks, cfg)
            derived = marked if bits == 8 else to_int(marked)
            ext, sims = extract(fr, derived, k, marks, cfg)
            clean = {"marked": marked, "ext": ext, "sims": sims}
            if precision == F64 and bits == 8:
                G.assert_u8_bars(marked[0], O.f32_to_u8(O.embed_frame(O.u8_to_f32(fr[0]), marks[0])), "frame 0 against the oracle")
            elif precision == F64:
                G.assert_f32_bars(marked[0], O.embed_frame(O.u16_to_f32(fr[0]), marks[0]), identical=0.999, what="frame 0 against the oracle")
            for n_case, (dtype, value) in enumerate(c for c in M.FLAT_FRAMES if np.dtype(c[0]).itemsize * 8 == bits):
                for j in at if n_case == 0 else at[1:2]:
                    bad = M.flat_batch(fr, j, value)
                    e, x = extract(bad, M.flat_batch(derived, j, value), k, marks, cfg)
                    got = {"marked": embed(bad, marks, cfg), "ext": e, "sims": x}
                    assert_isolated(clean, got, j, f"flat {bits}-bit frame of {value}")
                    if value == 0:
                        assert np.isnan(x[j]) and np.all(np.isnan(e[j])), "0 / 0: the oracle's answer for an all-zero frame"
            for n_case, kind in enumerate(M.MARK_POISONS):
                j = at[n_case % len(at)]
                bad = M.poison_marks(marks, j, kind)
                e, x = extract(fr, derived, k, bad, cfg)
                assert M.same_bits(e, ext), "the marks are not an input of the extraction"
                assert_isolated(clean, {"marked": embed(fr, bad, cfg), "ext": e, "sims": x}, j, f"{kind} in a mark, {bits} bit")
        for n_case, kind in enumerate(M.MARK_POISONS):          # the f32 entry points
            j = at[(n_case + 1) % len(at)]
            got = pipelines(frames, M.poison_marks(marks, j, kind), cfg, derived=ref["out"]["marked"])
            assert_isolated(ref["out"], got, j, f"{kind} in a mark, f32 frames")


@pytest.mark.parametrize("name", ["P", "L2"])
def test_similarity_calls_isolate_a_poisoned_row(name):
    """ssw_similarity_batch, and ssw_similarity_matrix: a poisoned extraction changes its row only, a poisoned stored mark its
    column only."""
    with shape_ctx(name) as (ctx, s):
        ref = clean_ref(name, F64)
        ext, marks = ref["out"]["ext"], ref["marks"]
        sims, matrix = G.similarity_batch(ext, marks), G.similarity_matrix(ext, marks)
        assert sims[0] == np.float32(O.similarity(ext[0], marks[0])) and np.all(np.isfinite(sims)) and np.all(np.isfinite(matrix))
        assert abs(float(matrix[0, 1]) - O.similarity(ext[0], marks[1])) <= 1e-4 * max(1.0, abs(O.similarity(ext[0], marks[1])))
        for kind in M.MARK_POISONS:
            for j in s["poison_at"]:
                bad_e, bad_m = M.poison_marks(ext, j, kind), M.poison_marks(marks, j, kind)
                for got in (G.similarity_batch(bad_e, marks), G.similarity_batch(ext, bad_m)):
                    assert M.others_same(sims, got, j) == [], (kind, j)
                assert M.others_same(matrix, G.similarity_matrix(bad_e, marks), j) == [], (kind, j, "rows")
                assert M.others_same(matrix.T.copy(), G.similarity_matrix(ext, bad_m).T.copy(), j) == [], (kind, j, "columns")


@pytest.mark.parametrize("precision", [F64, F32], ids=_id)
@pytest.mark.parametrize("name", ["P", "L2"])
def test_fingerprint_and_trace_isolate_a_poisoned_copy(name, precision):
    """ssw_fingerprint_embed with a poisoned mark for copy j; ssw_fingerprint_trace with a poisoned suspect j: its row of the
    matrix is NaN, it names no mark and exceeds nothing, and every other row is unchanged."""
    with shape_ctx(name) as (ctx, s):
        ref, cfg = clean_ref(name, precision), cfg_of(precision)
        base, marks, n = ref["frames"][0], ref["marks"], s["n"]
        copies = G.fingerprint(base, marks)
        if precision == F32:        # ssw_fingerprint_embed is canonical-precision only (include/ssw.h): the f32 trace reads the f64 copies
            with pytest.raises(wm.SswError) as err:
                G.fingerprint(base, marks, cfg)
            assert err.value.status == L.SSW_ERR_UNSUPPORTED
        else:
            G.assert_f32_bars(copies[0], O.embed_frame(base, marks[0]), identical=0.999, what="copy 0 against the oracle")
            for n_case, kind in enumerate(M.MARK_POISONS):
                j = s["poison_at"][n_case % 3]
                assert M.others_same(copies, G.fingerprint(base, M.poison_marks(marks, j, kind)), j) == [], (kind, j)
        clean = trace(base, copies, marks, cfg=cfg)
        assert list(clean["best"]) == list(range(n)) and np.all(clean["n_exceed"] == 1), clean
        if precision == F64:
            assert G.ext_within_1e5(clean["extracted"][0], O.extract_frame(base, copies[0], marks[0])[0])
        for n_case, kind in enumerate(M.FRAME_POISONS):
            for j in s["poison_at"] if n_case < 2 else s["poison_at"][n_case % 3:][:1]:
                got = trace(base, M.poison_batch(copies, j, kind), marks, cfg=cfg)
                assert_isolated(clean, got, j, f"poisoned suspect, {kind}")
                if kind in NAN_KINDS:
                    assert np.all(np.isnan(got["sims"][j])) and np.isnan(got["best_sim"][j]), (kind, j)
                    assert got["best"][j] == NONE and got["n_exceed"][j] == 0, (kind, j, got["best"][j], got["n_exceed"][j])


@pytest.mark.parametrize("precision", [F64, F32], ids=_id)
@pytest.mark.parametrize("name", ["P", "L2"])
def test_streaming_calls_isolate_across_group_boundaries(name, precision, monkeypatch):
    """mark_many / extract_many in groups of four frames (SSW_STREAM_GROUP): flat frames and poisoned marks in the first group,
    at the end of a group and in the ragged last one."""
    monkeypatch.setenv("SSW_STREAM_GROUP", "4")
    with shape_ctx(name, chunk=0) as (ctx, s):
        ref = clean_ref(name, precision)
        frames, marks, k = list(O.f32_to_u8(ref["frames"])), ref["marks"], s["k"]
        cw, cr = wm.WriteConfig(precision=precision), wm.ReadConfig(precision=precision)
        mark_many = lambda f, m: np.stack(wm.mark_many(f, m, cw, ctx=ctx))
        extract_many = lambda f, d, m: wm.extract_many(f, list(d), k, m, cr, ctx=ctx)
        marked = mark_many(frames, marks)
        ext, sims = extract_many(frames, marked, marks)
        assert M.same_bits(marked, G.batch_embed_rgb8(np.stack(frames), marks, cfg_of(precision))), "the streaming call is the batch call"
        if precision == F64:
            G.assert_u8_bars(marked[0], O.f32_to_u8(O.embed_frame(O.u8_to_f32(frames[0]), marks[0])), "frame 0 against the oracle")
        clean = {"marked": marked, "ext": ext, "sims": sims}
        for n_case, j in enumerate(s["poison_at"]):
            value = (0, 255)[n_case % 2]
            bad = [np.full_like(f, value) if i == j else f for i, f in enumerate(frames)]
            bad_marked = [np.full_like(f, value) if i == j else f for i, f in enumerate(marked)]
            e, x = extract_many(bad, bad_marked, marks)
            assert_isolated(clean, {"marked": mark_many(bad, marks), "ext": e, "sims": x}, j, f"flat frame of {value}")
            kind = M.MARK_POISONS[n_case]
            bad_m = M.poison_marks(marks, j, kind)
            e, x = extract_many(frames, marked, bad_m)
            assert_isolated(clean, {"marked": mark_many(frames, bad_m), "ext": e, "sims": x}, j, f"{kind} in a mark")


# ---- group 3: history -------------------------------------------------------------------------------------------------------
def _dirty_calls(name, k):
    """The poisoned batch pipelines of group 2 on one context: flat frames, every mark poison, every frame poison.  The last
    call is an f32 one with a frame of NaN in every chunk, as base and as derived frame, so that both lanes' operand planes,
    compact planes and handle planes are left holding NaN where those frames' lines lay."""
    s = M.SHAPES[name]
    frames, at = frames_of(name), s["poison_at"]
    marks = marks_of(name, k)
    marked = G.batch_embed(frames, marks)["rgb"]
    fr8 = M.flat_batch(O.f32_to_u8(frames), at[1], 0)
    G.batch_extract_rgb8(fr8, G.batch_embed_rgb8(fr8, marks), k, marks)
    for n_case, kind in enumerate(M.FRAME_POISONS):
        j = at[n_case % 3]
        bad_m = M.poison_marks(marks, at[(n_case + 1) % 3], M.MARK_POISONS[n_case % 4])
        pipelines(M.poison_batch(frames, j, kind), bad_m, cfg_of(), derived=M.poison_batch(marked, at[(n_case + 2) % 3], kind))
    bad, bad_d = frames, marked
    for j in sorted({*at, s["chunk"] + 1, 1}):               # first, second and ragged chunk
        bad, bad_d = M.poison_batch(bad, j, "all_nan"), M.poison_batch(bad_d, j, "all_nan")
    out = pipelines(bad, marks, cfg_of(), derived=bad_d)
    assert np.all(np.isnan(out["coef"][at[1]])) and np.all(np.isfinite(out["coef"][2]))


def _clean_calls(w, h, n, k, batch=True):
    """Clean batch pipelines on n frames of w x h (unless `batch` is off), then the single-image handles (Writer.mark_rgb8,
    Reader.extract, planes from the context's pool) on one."""
    out, ctx = {}, G.ctx()
    if batch:
        frames = np.stack([O.synth_frame(21, i, w, h) for i in range(n)])
        marks = np.random.default_rng(w + k).standard_normal((n, k)).astype(np.float32)
        out = pipelines(frames, marks, cfg_of())
    f8 = O.f32_to_u8(O.synth_frame(22, 0, w, h))
    mark = np.random.default_rng(k).standard_normal(k).astype(np.float32)
    wr = wm.Writer(f8, ctx=ctx)
    out["writer coef"] = wr.coefficient_image()
    out["mark_rgb8"] = wr.mark_rgb8([mark])
    out["reader extract"] = wm.Reader.base(f8, ctx=ctx).extract(wm.Reader.derived(out["mark_rgb8"], ctx), k)
    return out


@pytest.mark.parametrize("follow", ["same", "D", "narrow", "narrow-handles", "semi", "semi-handles"])
@pytest.mark.parametrize("name, k", [("P", M.K_GATHERED), ("L2", M.K_GATHERED), ("F", M.SHAPES["F"]["k"])])
def test_a_context_that_saw_poison_answers_like_a_fresh_one(name, k, follow):
    """Poisoned batches on the tuning's own shape (P by default, L2 under LEVEL2, F under FUSED); directly after them, on that
    context, ONE clean follow-up -- the same shape, D, the 432 x 272 shape of meta_cases.NARROW, the semi-deep 432 x 264 of
    NARROW_SEMI (narrower operand planes in the same workspaces, whose zero padding lies where the poisoned calls left NaN),
    or only the handles on one of those two -- so that no clean call has rewritten the workspaces in between: byte for byte
    what a fresh context gives."""
    s, d = M.SHAPES[name], M.SHAPES["D"]
    nw = M.NARROW_SEMI if follow.startswith("semi") else M.NARROW
    w, h, kk, plan = {"same": (s["w"], s["h"], k, s["plan"]), "D": (d["w"], d["h"], d["k"], d["plan"])}.get(
        follow, (nw["w"], nw["h"], nw["k"], nw["plan"][s["tuning"]]))
    results = []
    for dirty in (True, False):
        with shape_ctx(name) as (ctx, _):
            for n in {s["chunk"], s["n"] % s["chunk"]}:
                got_plan = ctx.transform_plan(n, w, h)
                assert {f: got_plan[f] for f in plan} == plan, (follow, n, got_plan)
            if follow not in ("same", "D"):
                # the pads these follow-ups are there for lie along k: the row pre-pass leaves w/4 = 108 terms in rows of 112
                # doubles; the staged column pre-pass runs, deep (272 rows: 34 units in rows of 40) or semi-deep (264 rows:
                # the M plane's 66 terms in rows of 72, which only its zero fill writes)
                assert (w // 4) % 8 != 0 and M.kpad(w // 2) > w // 4
                assert h >= tuning.get("deep_min_cols") and M.kpad(h // 4) > h // 8
                if follow.startswith("semi"):
                    assert h % 16 == 8 and not plan["cols_deep"] and M.kpad(h // 2) > h // 4
                else:
                    assert h % 16 == 0 and plan["cols_deep"]
            if dirty:
                _dirty_calls(name, k)
            results.append(_clean_calls(w, h, s["n"], kk, batch=not follow.endswith("handles")))
    got, want = results
    for key in want:
        assert np.all(np.isfinite(want[key])), key
        assert M.same_bits(got[key], want[key]), f"`{key}` after poisoned calls differs from a fresh context's"
