"""Tracing on the GPU: ssw_fingerprint_trace(_rgb8), its host and handle forms and the CLI's `trace` -- one original, S
suspect frames, M stored marks -> extracted marks, similarity matrix, and per suspect the mark it carries (or none).

Against the CPU oracle (Reader::base + Reader::derived + extract + Tester::similarity per suspect and mark) with the project's
bars -- extracted marks within 1e-5 (gpu_util.ext_within_1e5), similarities within 1e-4 relative -- and bit for bit against
the existing entry points: ssw_batch_extract(_rgb8) on a replicated base, ssw_similarity_matrix, ssw_similarity_batch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_util as G
import spread_spectrum_watermarking_amd as wm
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
E, EO, LG = L.ORDER_ENERGY, L.ORDER_ENERGY_ORTHOGONAL, L.ORDER_LEGACY
O1, O2, O3 = L.OPTION1, L.OPTION2, L.OPTION3
THRESHOLD = 6.0


def marks_for(n, k, seed):
    return np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)


def cat_u8():
    return np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))["cat"]


def trace(base, suspects, marks, k=None, threshold=THRESHOLD, cfg=None, want=("sims", "best", "best_sim", "n_exceed")):
    """ssw_fingerprint_trace(_rgb8) on device buffers: base [h, w, 3], suspects [S, h, w, 3] (both f32 or both u8),
    marks [M, k] or None -> dict of extracted / sims / best / best_sim / n_exceed (those in `want`)."""
    ctx, lib = G.ctx(), G.lib()
    u8 = base.dtype == np.uint8
    b, s = np.ascontiguousarray(base), np.ascontiguousarray(suspects)
    assert s.dtype == b.dtype and s.shape[1:] == b.shape
    h, w = b.shape[:2]
    n = s.shape[0]
    m = np.ascontiguousarray(marks, dtype=np.float32) if marks is not None else None
    n_marks = m.shape[0] if m is not None else 0
    k = m.shape[1] if m is not None else k
    c = cfg or G.default_config()
    db, ds = ctx.to_device(b), ctx.to_device(s) if n else ctx.alloc(16)
    dm = ctx.to_device(m) if m is not None and m.size else (ctx.alloc(16) if m is not None else None)
    shapes = {"sims": ((n, n_marks), np.float32), "best": ((n,), np.uint32), "best_sim": ((n,), np.float32), "n_exceed": ((n,), np.uint32)}
    ext = ctx.alloc(max(n * k, 1) * 4)
    outs = {name: ctx.alloc(max(int(np.prod(shapes[name][0])), 1) * 4) for name in want} if m is not None else {}
    ptr = lambda name: outs[name].ptr if name in outs else None
    fn = lib.ssw_fingerprint_trace_rgb8 if u8 else lib.ssw_fingerprint_trace
    G.check(fn(ctx.handle, C.byref(c), db.ptr, ds.ptr, n, w, h, k, dm.ptr if dm else None, n_marks, C.c_float(threshold), ext.ptr,
               ptr("sims"), ptr("best"), ptr("best_sim"), ptr("n_exceed")), "ssw_fingerprint_trace")
    res = {"extracted": ext.to_host(np.float32, (n, k))}
    for name, buf in outs.items():
        res[name] = buf.to_host(shapes[name][1], shapes[name][0])
    for x in [db, ds, dm, ext, *outs.values()]:
        if x:
            x.free()
    return res


def batch_extract_any(base, suspects, k, cfg=None):
    """ssw_batch_extract(_rgb8) with the base replicated once per suspect (the parent commit's way to ask)."""
    rep = np.repeat(base[None], suspects.shape[0], 0)
    if base.dtype == np.uint8:
        return G.batch_extract_rgb8(rep, suspects, k, np.zeros((suspects.shape[0], k), np.float32), cfg)[0]
    return G.batch_extract(rep, suspects, k, cfg=cfg)[0]


def ref_best(sims):
    """The contract's winner per row: the largest non-NaN entry, the lowest index on ties; NONE without one."""
    out = np.full(sims.shape[0], NONE, np.uint32)
    for s, row in enumerate(sims):
        ok = ~np.isnan(row)
        if ok.any():
            out[s] = np.flatnonzero(ok & (row == row[ok].max()))[0]
    return out


def ref_exceed(sims, threshold=THRESHOLD):
    with np.errstate(invalid="ignore"):
        return (sims > np.float32(threshold)).sum(1).astype(np.uint32)


def assert_consistent(res, marks, base, suspects, cfg=None, threshold=THRESHOLD):
    """Case 2 of the contract: every output bit for bit what the existing entry points give on the same data."""
    k = marks.shape[1]
    assert np.array_equal(res["extracted"], batch_extract_any(base, suspects, k, cfg)), "extracted vs ssw_batch_extract"
    assert np.array_equal(res["sims"], G.similarity_matrix(res["extracted"], marks), equal_nan=True), "sims vs ssw_similarity_matrix"
    assert np.array_equal(res["best"], ref_best(res["sims"]))
    assert np.array_equal(res["n_exceed"], ref_exceed(res["sims"], threshold))
    won = res["best"] != NONE
    assert np.all(np.isnan(res["best_sim"][~won]))
    if won.any():
        exact = G.similarity_batch(res["extracted"][won], marks[res["best"][won]])
        assert np.array_equal(res["best_sim"][won], exact), "best_sim vs ssw_similarity_batch"


def scenario(rgb_f32, marks, cfg_kw=None, u8=True):
    """The issue's six suspects from one original: oracle copies 0-3, the unmarked original, the average of copies 0 and 1.
    u8: 8-bit frames (copies through into_rgb8, the average rounded); else the f32 frames as Writer::mark returns them (synthetic
    frames: tests/test_fingerprint_gpu.py does the same -- their marks do not survive 8 bits at these sizes)."""
    kw = cfg_kw or {}
    copies = [O.embed_frame(rgb_f32, marks[i], **kw) for i in range(4)]
    if not u8:
        return rgb_f32, np.stack(copies + [rgb_f32, ((copies[0].astype(np.float64) + copies[1]) / 2).astype(np.float32)])
    copies = [O.f32_to_u8(c) for c in copies]
    base = O.f32_to_u8(rgb_f32)
    avg = ((copies[0].astype(np.uint16) + copies[1].astype(np.uint16) + 1) // 2).astype(np.uint8)
    return base, np.stack(copies + [base, avg])


def as_f32(frames):
    return O.u8_to_f32(frames) if frames.dtype == np.uint8 else frames


def oracle_matrix(base_f32, suspects_f32, marks, ordering=E, method=O2, alpha=0.1):
    """(extracted [S][k], sims [S][M]) of the reference flow, one forward transform per frame."""
    k = marks.shape[1]
    bc = G.oracle_forward(base_f32)[0]
    idx = O.indices(bc, ordering, k)
    ext = np.stack([O.extract(bc, G.oracle_forward(s)[0], idx, k, method, alpha) for s in suspects_f32])
    with np.errstate(invalid="ignore"):
        sims = np.array([[O.similarity(e, m) for m in marks] for e in ext], np.float32)
    return ext, sims


def assert_scenario(res, ext_o, sims_o, ext_ok=None):
    """Expectations of case 1 against the oracle's matrix (which must itself be clear of the threshold)."""
    finite = sims_o[~np.isnan(sims_o)]
    assert np.all(np.abs(finite - THRESHOLD) > 1e-3 * THRESHOLD), "oracle similarity too close to the threshold for an exact count"
    assert np.all(np.isnan(sims_o[4])), "the unmarked original extracts zeros: 0 / sqrt(0)"
    assert list(res["best"][:5]) == [0, 1, 2, 3, NONE] and res["best"][5] in (0, 1), res["best"]
    assert list(res["n_exceed"]) == [1, 1, 1, 1, 0, 2], (res["n_exceed"], sims_o)
    assert np.isnan(res["best_sim"][4]) and np.all(np.isnan(res["sims"][4]))
    assert (ext_ok or G.ext_within_1e5)(res["extracted"], ext_o)
    ok = ~np.isnan(sims_o)
    assert np.array_equal(np.isnan(res["sims"]), ~ok)
    assert np.all(np.abs(res["sims"][ok] - sims_o[ok]) <= 1e-4 * np.maximum(1.0, np.abs(sims_o[ok])))
    for s in (0, 1, 2, 3, 5):
        ref = sims_o[s][res["best"][s]]
        assert abs(res["best_sim"][s] - ref) <= 1e-4 * max(1.0, abs(ref)), (s, res["best_sim"][s], ref)


# 1 + 2. the cat scenario (640 x 444: the dense path), 8-bit, k = 1000, six marks ---------------------------------------
def test_cat_scenario_against_oracle_and_existing_entry_points():
    marks = marks_for(6, 1000, 11)
    base, sus = scenario(O.u8_to_f32(cat_u8()), marks)
    res = trace(base, sus, marks)
    ext_o, sims_o = oracle_matrix(O.u8_to_f32(base), O.u8_to_f32(sus), marks)
    d = np.diag(sims_o[:4, :4])
    print("oracle diagonal", d, "row 5", sims_o[5], "device best_sim", res["best_sim"], flush=True)
    assert_scenario(res, ext_o, sims_o)
    assert_consistent(res, marks, base, sus)
    # the f32 form on the frames the 8-bit ones decode to: the same reference flow
    res32 = trace(O.u8_to_f32(base), O.u8_to_f32(sus), marks)
    assert_scenario(res32, ext_o, sims_o)
    assert_consistent(res32, marks, O.u8_to_f32(base), O.u8_to_f32(sus))


# 3. other strategies, every ordering x method --------------------------------------------------------------------------
SHAPES = [(320, 180), (180, 320), (333, 197)]
CONFIGS = [(o, m) for o in (E, EO, LG) for m in (O1, O2, O3)]


def option3_ext_ok(ext, ref):
    """Option3 extracts ln(derived / base) / alpha: device logf against libm.  tests/test_config_matrix_gpu.py holds such
    extracted marks to max |d| <= 1e-4; the same bar here."""
    return bool(np.abs(np.asarray(ext, np.float64) - np.asarray(ref, np.float64)).max() <= 1e-4)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("conf", CONFIGS, ids=lambda c: f"o{c[0]}-m{c[1]}")
def test_small_shapes_every_configuration(shape, conf):
    w, h = shape
    ordering, method = conf
    marks = marks_for(6, 300, w * 7 + h + ordering * 3 + method)
    kw = dict(ordering=ordering, method=method, alpha=0.1)
    base, sus = scenario(O.synth_frame(3, w + h, w, h), marks, kw, u8=False)
    cfg = G.default_config(L.PRECISION_F64, ordering, method, 0.1)
    res = trace(base, sus, marks, cfg=cfg)
    assert_consistent(res, marks, base, sus, cfg)
    ext_o, sims_o = oracle_matrix(base, sus, marks, ordering, method, 0.1)
    assert_scenario(res, ext_o, sims_o, option3_ext_ok if method == O3 else None)


def test_level2_and_fused_derived_kernels_on_a_small_frame():
    """Thresholds lowered like tools/level2_check.py, and merge_max_lines so that six suspects' lines take the fused derived
    kernel: the pruned path with the shared plan against the oracle and the per-pair entry points."""
    w, h, k = 1024, 144, 200
    marks = marks_for(6, k, 21)
    base, sus = scenario(O.synth_frame(21, 0, w, h), marks, u8=False)
    ext_o, sims_o = oracle_matrix(base, sus, marks)
    with wm.tuning(efold_min=256, efold_inv_min=256, efold_cols_min=64, merge_max_lines=256), G.fresh_ctx() as ctx:
        ctx.reset_timing()
        res = trace(base, sus, marks)
        st = ctx.prune_stats()
        assert st["pruned_chunks"] == 1 and st["redone_chunks"] == 0, st
        assert_scenario(res, ext_o, sims_o)
        assert_consistent(res, marks, base, sus)
        with wm.tuning(derived_fused=0):                      # pre-pass + gathered launches
            res2 = trace(base, sus, marks)
        for name in res:
            assert np.array_equal(res[name], res2[name], equal_nan=True), name


# 4. 4K, f32 and u8, 12 suspects from ssw_fingerprint_embed, 64 stored marks -------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_4k_twelve_suspects(u8):
    w, h, k, n, n_marks = 3840, 2160, 1000, 12, 64
    rgb = O.synth_frame(7, 0, w, h)
    base = O.f32_to_u8(rgb) if u8 else rgb
    marks = marks_for(n_marks, k, 31)
    sus = G.fingerprint(base, marks[:n])
    ctx = G.ctx()
    ctx.reset_timing()
    res = trace(base, sus, marks)
    st = ctx.prune_stats()
    assert st["pruned_chunks"] == 1 and st["redone_chunks"] == 0, st
    assert list(res["best"]) == list(range(n)), res["best"]
    assert np.all(res["best_sim"] > THRESHOLD) and np.all(res["n_exceed"] == 1), (res["best_sim"], res["n_exceed"])
    ctx.reset_timing()
    assert_consistent(res, marks, base, sus)          # (runs ssw_batch_extract on 12 replicated pairs)
    ctx.reset_timing()
    batch_extract_any(base, sus[:1], k)
    assert ctx.prune_stats()["columns_needed"] == st["columns_needed"], "one list: the column set of a single pair"
    ctx.set_chunk_frames(5)                            # three chunks on two lanes
    try:
        ctx.reset_timing()
        res5 = trace(base, sus, marks)
        st5 = ctx.prune_stats()
    finally:
        ctx.set_chunk_frames(0)
    assert st5["pruned_chunks"] == 3 and st5["redone_chunks"] == 0 and st5["columns_needed"] == st["columns_needed"], st5
    for name in res:
        assert np.array_equal(res[name], res5[name]), name


def test_columns_that_do_not_fit_redo_every_chunk():
    """The trace's redo branch (the shape of test_pruned_path_falls_back_when_the_columns_do_not_fit): k = 200 gives a compact
    plane of 128 columns, 128 * 4 <= 1040, so pruning is attempted; the first 200 indices of this white-noise original touch
    184 distinct columns (counted on the CPU with the oracle: O.indices of its plane, index % 1040), so the one list of the call
    overflows by construction, the one flag is set, and all three chunks are redone with the full transform."""
    w, h, k = 1040, 144, 200
    base = np.random.default_rng(51).random((h, w, 3)).astype(np.float32)
    marks = marks_for(5, k, 43)
    sus = G.fingerprint(base, marks)
    ctx = G.ctx()
    ctx.set_chunk_frames(2)                            # three chunks on two lanes
    try:
        ctx.reset_timing()
        res = trace(base, sus, marks)
        st = ctx.prune_stats()
        ctx.set_prune(False)
        try:
            full = trace(base, sus, marks)
        finally:
            ctx.set_prune(True)
    finally:
        ctx.set_chunk_frames(0)
    assert st["pruned_chunks"] == 3 and st["redone_chunks"] == 3, st
    for name in res:
        assert np.array_equal(res[name], full[name], equal_nan=True), name


def test_last_chunk_takes_the_other_row_route():
    """The tuning of test_level2_and_fused_derived_kernels_on_a_small_frame with six suspects in chunks of five: the first
    chunk's 720 lines (> merge_max_lines = 256) take the fused derived kernel, the last chunk's 144 lines the merged subset
    launch, so the call's tables must hold the gathered bases in both orders."""
    w, h, k = 1024, 144, 200
    marks = marks_for(6, k, 21)
    base, sus = scenario(O.synth_frame(21, 0, w, h), marks, u8=False)
    with wm.tuning(efold_min=256, efold_inv_min=256, efold_cols_min=64, merge_max_lines=256), G.fresh_ctx() as ctx:
        whole = trace(base, sus, marks)
        ctx.set_chunk_frames(5)
        ctx.reset_timing()
        res = trace(base, sus, marks)
        st = ctx.prune_stats()
    assert st["pruned_chunks"] == 2 and st["redone_chunks"] == 0, st
    for name in whole:
        assert np.array_equal(res[name], whole[name], equal_nan=True), name


# 5. independence -------------------------------------------------------------------------------------------------------
def test_rows_independent_of_company_and_position():
    w, h, k = 768, 256, 200
    marks = marks_for(9, k, 41)
    base = O.synth_frame(41, 0, w, h)
    sus = np.concatenate([G.fingerprint(base, marks[:7]), base[None]])
    a = trace(base, sus, marks)
    assert list(a["best"]) == [0, 1, 2, 3, 4, 5, 6, NONE]
    perm = np.roll(np.arange(8), 3)
    p = trace(base, sus[perm], marks)
    for name in a:
        assert np.array_equal(p[name], a[name][perm], equal_nan=True), name
    for sub in ([0], [7], [2, 5], [6, 1, 7]):
        r = trace(base, sus[sub], marks)
        for name in a:
            assert np.array_equal(r[name], a[name][sub], equal_nan=True), (name, sub)


# 6. prune off ----------------------------------------------------------------------------------------------------------
def test_prune_off_gives_the_same_bits():
    w, h, k = 768, 256, 200
    marks = marks_for(5, k, 51)
    base = O.synth_frame(51, 0, w, h)
    sus = np.concatenate([G.fingerprint(base, marks[:4]), base[None]])
    ctx = G.ctx()
    ctx.reset_timing()
    on = trace(base, sus, marks)
    assert ctx.prune_stats()["pruned_chunks"] == 1
    ctx.set_prune(False)
    try:
        ctx.reset_timing()
        off = trace(base, sus, marks)
        assert ctx.prune_stats()["pruned_chunks"] == 0
        ctx.set_chunk_frames(2)
        off2 = trace(base, sus, marks)
    finally:
        ctx.set_prune(True)
        ctx.set_chunk_frames(0)
    for name in on:
        assert np.array_equal(on[name], off[name], equal_nan=True), name
        assert np.array_equal(on[name], off2[name], equal_nan=True), name
    assert_consistent(on, marks, base, sus)


# 7. tie rule and NaN rule of the finish kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_marks,dups", [(1, (0,)), (63, (5, 62)), (65, (10, 64)), (1000, (64, 999))])
def test_ties_take_the_lower_index_and_nan_never_wins(n_marks, dups):
    w, h, k = 256, 144, 100
    rgb = O.synth_frame(61, 0, w, h)
    own = marks_for(2, k, 61)
    marks = marks_for(n_marks, k, 62 + n_marks)
    for j in dups:
        marks[j] = own[0]
    base = rgb
    sus = np.concatenate([G.fingerprint(base, own), base[None]])         # copy of mark 0 (stored), of mark 1 (not stored), the original
    res = trace(base, sus, marks)
    assert np.array_equal(res["best"], ref_best(res["sims"])) and np.array_equal(res["n_exceed"], ref_exceed(res["sims"]))
    assert res["best"][0] == min(dups), (res["best"], dups)
    assert res["n_exceed"][0] >= len(dups) and np.all(res["sims"][0][list(dups)] > THRESHOLD)
    assert res["sims"][0][dups[0]] == res["sims"][0][dups[-1]]
    assert res["best"][2] == NONE and np.isnan(res["best_sim"][2]) and res["n_exceed"][2] == 0
    assert np.all(np.isnan(res["sims"][2]))
    assert_consistent(res, marks, base, sus)
    # a threshold below everything counts every non-NaN entry, none of the NaN row
    low = trace(base, sus, marks, threshold=-1e30, want=("n_exceed",))
    assert list(low["n_exceed"]) == [n_marks, n_marks, 0]


# 8. host and handle forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_and_handle_forms_equal_the_device_form(pinned, monkeypatch):
    monkeypatch.setenv("SSW_STREAM_GROUP", "2")           # five suspects: three streaming groups
    w, h, k = 768, 256, 200
    marks = marks_for(6, k, 71)
    base = O.f32_to_u8(O.synth_frame(71, 0, w, h))
    sus = np.concatenate([G.fingerprint(base, marks[:4]), base[None]])
    dev = trace(base, sus, marks)
    ctx = G.ctx()
    if pinned:
        bufs = []
        for s in sus:
            p = ctx.pinned_empty(s.shape, np.uint8)
            p[...] = s
            bufs.append(p)
    else:
        bufs = [s.copy() for s in sus]
    host = wm.trace_many(base, bufs, list(marks), ctx=ctx)
    reader = wm.Reader.base(base, ctx=ctx)
    handle = reader.trace(bufs, list(marks))
    for r in (host, handle):
        for name in dev:
            assert np.array_equal(getattr(r, name), dev[name], equal_nan=True), name
    for s in range(5):
        assert host.matches(s) == list(np.flatnonzero(dev["sims"][s] > np.float32(THRESHOLD)))
    assert dev["best"][4] == NONE          # (8-bit synthetic copies: which mark survives is the device form's business, tested above)
    # the reader is untouched: extract() afterwards equals row 1, indices() the oracle's
    assert np.array_equal(reader.extract(wm.Reader.derived(sus[1], ctx), k), dev["extracted"][1])
    only = reader.trace(bufs[:2], None, k=k)              # extraction only
    assert np.array_equal(only.extracted, dev["extracted"][:2])
    with pytest.raises(wm.SswError) as e:
        wm.Reader(base, False, wm.ReadConfig(), ctx).trace(bufs, list(marks))
    assert e.value.status == L.SSW_ERR_NOT_BASE


# 9. statuses ----------------------------------------------------------------------------------------------------------------
def test_error_statuses():
    lib, ctx = G.lib(), G.ctx()
    w, h, k = 64, 48, 50
    rgb = O.synth_frame(81, 0, w, h)
    marks = marks_for(3, k, 81)
    d, ds, dm = ctx.to_device(rgb), ctx.to_device(np.stack([rgb, rgb])), ctx.to_device(marks)
    ext, sims, best, bs, ne = (ctx.alloc(2 * max(k, 3) * 4) for _ in range(5))
    cfg = G.default_config()
    th = C.c_float(6.0)
    call = lambda c, b, s, n, kk, m, nm, e, *o: lib.ssw_fingerprint_trace(ctx.handle, C.byref(c) if c else None, b, s, n, w, h, kk, m, nm, th, e, *o)
    full = (sims.ptr, best.ptr, bs.ptr, ne.ptr)
    none = (None, None, None, None)
    assert call(cfg, d.ptr, ds.ptr, 2, k, dm.ptr, 3, ext.ptr, *full) == L.SSW_OK
    assert call(cfg, d.ptr, ds.ptr, 2, w * h, dm.ptr, 3, ext.ptr, *full) == L.SSW_ERR_K_TOO_LARGE
    assert call(cfg, d.ptr, ds.ptr, 0, k, dm.ptr, 3, ext.ptr, *full) == L.SSW_OK
    assert call(cfg, d.ptr, ds.ptr, 2, k, None, 0, ext.ptr, *none) == L.SSW_OK                       # extraction only
    assert call(cfg, d.ptr, ds.ptr, 2, k, None, 3, ext.ptr, *none) == L.SSW_ERR_BAD_ARG
    for i in range(4):
        o = [None] * 4
        o[i] = full[i]
        assert call(cfg, d.ptr, ds.ptr, 2, k, None, 0, ext.ptr, *o) == L.SSW_ERR_BAD_ARG
    assert call(cfg, d.ptr, ds.ptr, 2, k, dm.ptr, 3, ext.ptr, *none) == L.SSW_OK                     # every similarity output optional
    for bad in (L.Config(L.ORDER_CUSTOM, O2, 0.1, L.PRECISION_F64), L.Config(E, L.METHOD_CUSTOM, 0.1, L.PRECISION_F64)):
        assert call(bad, d.ptr, ds.ptr, 2, k, dm.ptr, 3, ext.ptr, *full) == L.SSW_ERR_UNSUPPORTED
    assert call(None, d.ptr, ds.ptr, 2, k, dm.ptr, 3, ext.ptr, *full) == L.SSW_ERR_BAD_ARG
    assert call(cfg, None, ds.ptr, 2, k, dm.ptr, 3, ext.ptr, *full) == L.SSW_ERR_BAD_ARG
    assert call(cfg, d.ptr, None, 2, k, dm.ptr, 3, ext.ptr, *full) == L.SSW_ERR_BAD_ARG
    assert call(cfg, d.ptr, ds.ptr, 2, k, dm.ptr, 3, None, *full) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_fingerprint_trace(ctx.handle, C.byref(cfg), d.ptr, ds.ptr, 2, 0, h, k, dm.ptr, 3, th, ext.ptr, *full) == L.SSW_ERR_BAD_DIMS
    # n_marks == 0 with a marks pointer, and k == 0: no winner anywhere
    for kk, nm in ((k, 0), (0, 3)):
        assert call(cfg, d.ptr, ds.ptr, 2, kk, dm.ptr, nm, ext.ptr, *full) == L.SSW_OK
        assert list(best.to_host(np.uint32, (2,))) == [NONE, NONE]
        assert np.all(np.isnan(bs.to_host(np.float32, (2,)))) and list(ne.to_host(np.uint32, (2,))) == [0, 0]
    for b in (d, ds, dm, ext, sims, best, bs, ne):
        b.free()
    # SSW_PRECISION_F32 takes the dense path and answers
    f32 = G.default_config(L.PRECISION_F32)
    sus = np.concatenate([G.fingerprint(rgb, marks[:2]), rgb[None]])
    r = trace(rgb, sus, marks, cfg=f32)
    assert list(r["best"]) == [0, 1, NONE] and np.array_equal(r["extracted"], batch_extract_any(rgb, sus, k, f32))
    with pytest.raises(ValueError):
        wm.trace_many(O.f32_to_u8(rgb), list(O.f32_to_u8(sus)), [marks[0], marks[1][:40]], ctx=ctx)


# 10. the CLI: fingerprint, then trace over every copy and the original ---------------------------------------------------
def test_cli_fingerprint_then_trace_names_every_copy(tmp_path):
    import shutil
    src = tmp_path / "cat.jpg"
    shutil.copy(os.path.join(GOLDEN, "porcelain_cat_grey_background.jpg"), src)
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "spread_spectrum_watermarking_amd.cli", *a], cwd=str(tmp_path), env=env,
                                    capture_output=True, text=True, check=True, timeout=600).stdout
    run("fingerprint", str(src), "--copies", "4", "-d", "buyer")
    files = [str(tmp_path / f"cat_fp{i}.png") for i in range(4)] + [str(src)]
    out = run("trace", str(src), "--suspects", *files, "--marks", str(tmp_path / "cat_fp.json"))
    records = out.split("-\n")[1:]
    assert len(records) == 5, out
    for i in range(4):
        assert f'Suspect: "{files[i]}"' in records[i] and "Matches: true" in records[i], out
        assert f'Description: "buyer #{i}"' in records[i] and "Also:" not in records[i], out
        sim = float(records[i].split("Similarity: ")[1].split()[0])
        assert sim > 6.0
    assert f'Suspect: "{files[4]}"' in records[4] and "Matches: false" in records[4] and "Description" not in records[4], out
