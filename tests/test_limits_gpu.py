"""The kernels outside the box the benchmark sizes draw: frames of 2^27 pixels and more (the inverse's RGB epilogue leaves its
buffer-resource round), rows longer than 32768 (no deep inverse row pass), strips 16 or 24 lines tall and their transposes,
batches of more than 65535 frames in one pass (frame counts in a grid dimension) and fingerprinting past one group of 64
copies.  Everything goes through the C ABI and is checked against the CPU oracle with the project's own bars
(tests/gpu_util.py): marked f32 frames max |d| <= 2e-7 and >= 0.999 bit-identical against the oracle (the 4K bar), >= 0.9999
against another GPU path; 8-bit frames <= 1 LSB and >= 99.99 % equal; extracted marks per element within 1e-5 * max(1, |ref|);
index lists identical; coefficient planes the bars of tools/fuzz_dct.py.  Every case prints what it measured (`-s`)."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import gpu_util as G
import spread_spectrum_watermarking_amd as wm
from conftest import ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_batch  # noqa: E402
import fuzz_dct  # noqa: E402

pytestmark = pytest.mark.gpu

ORACLE_4K_IDENTICAL = 0.999          # marked frames against the oracle at 4K and above (tests/test_fingerprint_gpu.py)


def report(what, **vals):
    print(f"\nlimits {what}: " + " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in vals.items()))


# A. huge single frames ---------------------------------------------------------------------------------------------------
K_HUGE = 1000
# (h, w, forward plan, inverse plan): 2^27 pixels exactly -- the RGB epilogue of the inverse stores through put_quad; 16 rows
# fewer -- its buffer-resource round at the largest offsets (off * 12 just below 0x60000000); rows of 65536 -- beyond the deep
# inverse row pass (len <= 32768): PairTwo rows, then level-2 columns on a natural-order plane
HUGE = [(8192, 16384, 127, 63), (8176, 16384, 127, 63), (1024, 65536, 127, 21)]


def huge_mark(h, w):
    return np.random.default_rng(h + w).standard_normal((1, K_HUGE)).astype(np.float32)


@pytest.mark.parametrize("h, w, fwd, inv", HUGE, ids=[f"{w}x{h}" for h, w, _, _ in HUGE])
def test_huge_frame_plans(h, w, fwd, inv):
    """Each huge case reaches the branch it is here for; a planner change has to update this deliberately."""
    assert G.plan_flags(1, w, h, L.DCT2) == fwd
    assert G.plan_flags(1, w, h, L.DCT3) == inv


@pytest.fixture(scope="module", params=HUGE, ids=[f"{w}x{h}" for h, w, _, _ in HUGE])
def huge(request):
    """One huge frame (ssw_synth_frames: bit-identical to oracle.synth_frame, which takes seconds per frame at this size), its
    ssw_batch_embed result and the oracle's flow on it: forward plane, index list, marked frame and the marked frame's forward
    plane (what extraction reads) -- each computed once.  Module scope with parameters: one case alive at a time."""
    h, w, _, _ = request.param
    rgb = G.synth(h, 0, 1, w, h)[0]
    mark = huge_mark(h, w)
    res = G.batch_embed(rgb[None], mark, want_idx=True)
    marked, idx = res["rgb"][0], res["idx"][0]
    del res
    with ThreadPoolExecutor(1) as pool:                 # the oracle's C calls release the GIL: the derived plane alongside
        derived = pool.submit(lambda: G.oracle_forward(marked)[0])
        coef, i, q = G.oracle_forward(rgb)
        o_idx = O.indices(coef, k=K_HUGE)
        o_marked = G.oracle_marked(coef, i, q, o_idx, mark[0])
        del i, q
        d_coef = derived.result()
    yield {"h": h, "w": w, "rgb": rgb, "mark": mark, "marked": marked, "idx": idx, "coef": coef, "o_idx": o_idx,
           "o_marked": o_marked, "d_coef": d_coef}


def test_huge_frame_embed_matches_the_oracle(huge):
    assert np.array_equal(huge["idx"], huge["o_idx"].astype(np.uint32))
    err, same = G.f32_stats(huge["marked"], huge["o_marked"])
    report(f"{huge['w']}x{huge['h']} embed vs oracle", max_err=err, identical=same)
    G.assert_f32_bars(huge["marked"], huge["o_marked"], ORACLE_4K_IDENTICAL, "batch vs oracle")


def test_huge_frame_writer_handle_equals_the_batch_call(huge):
    got = wm.Writer(huge["rgb"], wm.WriteConfig(), G.ctx()).mark([huge["mark"][0]])
    assert np.array_equal(got, huge["marked"])


def test_huge_frame_extract_matches_the_oracle(huge):
    """ssw_batch_extract with the pruned derived transform (the default) against the oracle, and against the full transform
    (set_prune(False)) bit for bit."""
    ctx = G.ctx()
    rgb, marked, mark = huge["rgb"][None], huge["marked"][None], huge["mark"]
    pruned0 = ctx.prune_stats()["pruned_chunks"]
    ext, sims = G.batch_extract(rgb, marked, K_HUGE, mark)
    pruned = ctx.prune_stats()["pruned_chunks"] - pruned0
    ctx.set_prune(False)
    try:
        ext_full, sims_full = G.batch_extract(rgb, marked, K_HUGE, mark)
    finally:
        ctx.set_prune(True)
    assert np.array_equal(ext, ext_full) and np.array_equal(sims, sims_full)
    o_ext, o_sim = G.oracle_extracted(huge["coef"], huge["d_coef"], huge["o_idx"], mark[0])
    report(f"{huge['w']}x{huge['h']} extract vs oracle", max_err=float(np.abs(ext[0] - o_ext).max()),
           identical=float(np.mean(ext[0] == o_ext)), sim_err=abs(float(sims[0]) - o_sim), pruned_chunks=pruned)
    assert G.ext_within_1e5(ext[0], o_ext)
    assert abs(float(sims[0]) - o_sim) < 1e-4 * max(1.0, abs(o_sim))


def test_huge_frame_fingerprint_equals_the_batch_call(huge):
    rgb, mark = huge["rgb"], huge["mark"]
    other = np.random.default_rng(7).standard_normal((1, K_HUGE)).astype(np.float32)
    copies = G.fingerprint(rgb, np.concatenate([mark, other]))
    batch = G.batch_embed(rgb[None], other)["rgb"][0]
    (err0, same0), (err1, same1) = G.f32_stats(copies[0], huge["marked"]), G.f32_stats(copies[1], batch)
    report(f"{huge['w']}x{huge['h']} fingerprint vs batch", max_err=max(err0, err1), identical=min(same0, same1))
    G.assert_f32_bars(copies[0], huge["marked"], what="copy 0 vs batch")
    G.assert_f32_bars(copies[1], batch, what="copy 1 vs batch")


def test_huge_frame_8bit_entry_points_match_the_oracle():
    """ssw_batch_embed_rgb8 / ssw_batch_extract_rgb8 on the 8-bit form of the 2^27-pixel frame (the slow RGB epilogue, 8-bit
    stores) against the oracle's flow on u8_to_f32 of it."""
    h, w = HUGE[0][:2]
    frame8 = O.f32_to_u8(G.synth(h, 0, 1, w, h)[0])
    mark = huge_mark(h, w)
    wm8 = G.batch_embed_rgb8(frame8[None], mark)[0]
    ext, sims = G.batch_extract_rgb8(frame8[None], wm8[None], K_HUGE, mark)
    with ThreadPoolExecutor(1) as pool:
        derived = pool.submit(lambda: G.oracle_forward(O.u8_to_f32(wm8))[0])
        coef, i, q = G.oracle_forward(O.u8_to_f32(frame8))
        idx = O.indices(coef, k=K_HUGE)
        o_wm8 = O.f32_to_u8(G.oracle_marked(coef, i, q, idx, mark[0]))
        del i, q
        d_coef = derived.result()
    d = np.abs(wm8.astype(np.int16) - o_wm8)
    o_ext, o_sim = G.oracle_extracted(coef, d_coef, idx, mark[0])
    report(f"{w}x{h} 8-bit vs oracle", max_lsb=int(d.max()), equal=float(np.mean(d == 0)),
           ext_err=float(np.abs(ext[0] - o_ext).max()), ext_identical=float(np.mean(ext[0] == o_ext)))
    G.assert_u8_bars(wm8, o_wm8, "8-bit embed vs oracle")
    assert G.ext_within_1e5(ext[0], o_ext)
    assert abs(float(sims[0]) - o_sim) < 1e-4 * max(1.0, abs(o_sim))


# B. strips ---------------------------------------------------------------------------------------------------------------
# (h, w, forward plan, inverse plan): level-2 rows over a handful of lines, then pair columns 16 or 24 long; the transposes
# run columns first
STRIPS = [(16, 8192, 11, 11), (24, 4096, 11, 11), (16, 32768, 11, 11),
          (8192, 16, 21, 21), (4096, 24, 21, 21), (32768, 16, 21, 21)]
STRIP_IDS = [f"{h}x{w}" for h, w, _, _ in STRIPS]


@pytest.mark.parametrize("h, w, fwd, inv", STRIPS, ids=STRIP_IDS)
def test_strip_plans(h, w, fwd, inv):
    for n in (1, 2, 3):
        assert G.plan_flags(n, w, h, L.DCT2) == fwd and G.plan_flags(n, w, h, L.DCT3) == inv, n


@pytest.mark.parametrize("cfg", [None, (L.ORDER_LEGACY, L.OPTION3, 0.1)], ids=["default", "legacy-o3"])
@pytest.mark.parametrize("h, w, fwd, inv", STRIPS, ids=STRIP_IDS)
def test_strips_through_the_batch_pipelines(h, w, fwd, inv, cfg):
    """tools/fuzz_batch.py: 3 frames, k = 200, pruned + two lanes against full + one lane bit for bit, frame 0 against the
    oracle.  On a fresh context: the first call of a shape makes its basis tables on the context's stream while the chains are
    built, and the second lane's RGB pre-pass has to wait for them (csrc/ssw_pipeline.hip run_pipeline_impl; before, rows of
    16384 and more read the rotation tables before they were written and every coefficient of the first pass was wrong)."""
    with G.fresh_ctx():
        r = fuzz_batch.check(h, w, 3, 200, h + w, h * w, cfg)
    report(f"{h}x{w} batch {'default' if cfg is None else 'legacy-o3'}", marked_err=r["marked_err"], ext_err=r["ext_err"],
           sim_err=r["sim_err"], pruned_chunks=r["pruned_chunks"])
    assert r["same"], "pruned + two lanes differs from full transforms + one lane"
    assert fuzz_batch.passes(r), r


@pytest.mark.parametrize("kind", ["fwd", "ortho", "inv"])
@pytest.mark.parametrize("h, w, fwd, inv", STRIPS, ids=STRIP_IDS)
def test_strips_through_ssw_dct2d(h, w, fwd, inv, kind):
    same, err = fuzz_dct.check(h, w, 3, h * 31 + w, kind)
    report(f"{h}x{w} dct2d {kind}", identical=same, err_over_ac=err)
    assert same >= fuzz_dct.BAR_IDENTICAL and err <= fuzz_dct.BAR_ERR, (same, err)


# C. batches past 65535 frames --------------------------------------------------------------------------------------------
N_MANY, K_MANY, CHUNK = 70000, 20, 4096
SAMPLE = [0, 65534, 65535, 65536, 69999]
TINY = [(16, 16), (8, 8)]            # (h, w): the pair path (plan 1) and the dense kernels


def in_calls_of(fn, n, step=CHUNK):
    """fn(f0, n_f) over [0, n) in separate calls of `step` frames, concatenated."""
    return np.concatenate([fn(f0, min(step, n - f0)) for f0 in range(0, n, step)])


def flows(rgb, marks, db):
    res = G.batch_embed(rgb, marks, want_idx=True)
    ext, sims = G.batch_extract(rgb, res["rgb"], marks.shape[1], marks)
    return res["rgb"], res["idx"], ext, sims, G.similarity_matrix(ext, db)


@pytest.mark.parametrize("h, w", TINY, ids=[f"{h}x{w}" for h, w in TINY])
def test_more_than_65535_frames_through_the_batch_flows(h, w):
    """70000 frames in one pass (select / embed / extract launches carry the frame in a grid dimension) against the same frames
    in passes of 4096 (set_chunk_frames), bit for bit; five frames around 65535 against the oracle."""
    ctx = G.ctx()
    assert G.plan_flags(N_MANY, w, h) == (1 if h == 16 else 0)
    assert ctx.pass_frames(N_MANY, w, h) == N_MANY
    seed = 11 + h
    rgb = G.synth(seed, 0, N_MANY, w, h)
    assert np.array_equal(rgb, in_calls_of(lambda f0, n: G.synth(seed, f0, n, w, h), N_MANY))
    for f in SAMPLE:
        assert np.array_equal(rgb[f], O.synth_frame(seed, f, w, h)), f
    marks = np.random.default_rng(seed).standard_normal((N_MANY, K_MANY)).astype(np.float32)
    db = marks[SAMPLE]
    a = flows(rgb, marks, db)
    ctx.set_chunk_frames(CHUNK)
    try:
        assert ctx.pass_frames(N_MANY, w, h) == CHUNK
        b = flows(rgb, marks, db)
    finally:
        ctx.set_chunk_frames(0)
    for name, x, y in zip(("marked", "indices", "extracted", "similarities", "similarity matrix"), a, b):
        assert np.array_equal(x, y), f"{name}: one pass of {N_MANY} frames differs from passes of {CHUNK}"
    marked, idx, ext, sims, smat = a
    got, ref, ext_err, sim_err = [], [], 0.0, 0.0
    for j, f in enumerate(SAMPLE):
        o_marked = O.embed_frame(rgb[f], marks[f])
        o_ext, o_sim = O.extract_frame(rgb[f], marked[f], marks[f])
        assert np.array_equal(idx[f], O.indices(G.oracle_forward(rgb[f])[0], k=K_MANY).astype(np.uint32)), f
        assert G.ext_within_1e5(ext[f], o_ext), f
        assert abs(float(sims[f]) - o_sim) < 1e-4 * max(1.0, abs(o_sim)), f
        row = np.array([O.similarity(ext[f], m) for m in db], np.float32)
        assert np.abs(smat[f] - row).max() <= 1e-4 * max(1.0, np.abs(row).max()), f
        got.append(marked[f]); ref.append(o_marked)
        ext_err, sim_err = max(ext_err, float(np.abs(ext[f] - o_ext).max())), max(sim_err, abs(float(sims[f]) - o_sim))
    err, same = G.f32_stats(np.stack(got), np.stack(ref))
    report(f"{N_MANY} x {h}x{w} flows vs oracle", max_err=err, identical=same, ext_err=ext_err, sim_err=sim_err)
    G.assert_f32_bars(np.stack(got), np.stack(ref), ORACLE_4K_IDENTICAL, "sampled frames vs oracle")


def dct_bars(got, ref):
    """tools/fuzz_dct.py's measures on a stack of planes: (identical fraction, max error / AC max)."""
    return float(np.mean(got == ref)), float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref[:, 1:, 1:]).max(), 1.0))


@pytest.mark.parametrize("h, w", TINY, ids=[f"{h}x{w}" for h, w in TINY])
def test_more_than_65535_planes_through_ssw_dct2d_and_ssw_topk_indices(h, w):
    x = np.random.default_rng(h).random((N_MANY, h, w)).astype(np.float32)
    for kind in (L.DCT2, L.DCT3):
        src = G.dct2d(x, L.DCT2, L.PRECISION_F64) if kind == L.DCT3 else x
        got = G.dct2d(src, kind, L.PRECISION_F64)
        assert np.array_equal(got, in_calls_of(lambda f0, n: G.dct2d(src[f0:f0 + n], kind, L.PRECISION_F64), N_MANY)), kind
        same, err = dct_bars(got[SAMPLE], np.stack([O.dct2d(src[f], kind) for f in SAMPLE]))
        report(f"{N_MANY} x {h}x{w} dct2d type {kind} vs oracle", identical=same, err_over_ac=err)
        assert same >= fuzz_dct.BAR_IDENTICAL and err <= fuzz_dct.BAR_ERR, (kind, same, err)
    coef = G.dct2d(x, L.DCT2, L.PRECISION_F64)
    idx = G.topk(coef, K_MANY)
    assert np.array_equal(idx, in_calls_of(lambda f0, n: G.topk(coef[f0:f0 + n], K_MANY), N_MANY))
    for f in SAMPLE:
        assert np.array_equal(idx[f], O.indices(coef[f], k=K_MANY).astype(np.uint32)), f


def test_more_than_65535_frames_through_the_two_pass_resize():
    """20 x 12 -> 13 x 9: output rows of 39 bytes send every batch to the two-pass fallback (the fused kernel takes neither
    unaligned rows nor more than 65535 frames), whose vertical pass has the frame in gridDim.z."""
    frames = np.random.default_rng(3).integers(0, 256, (N_MANY, 12, 20, 3), dtype=np.uint8)
    got = G.resize_rgb8(frames, 13, 9)
    assert np.array_equal(got, in_calls_of(lambda f0, n: G.resize_rgb8(frames[f0:f0 + n], 13, 9), N_MANY))
    for f in SAMPLE:
        assert np.array_equal(got[f], O.resize_rgb8(frames[f], 13, 9)), f


# D. fingerprinting past one group of 64 copies -----------------------------------------------------------------------------
FP_W, FP_H, FP_K = 320, 180, 500


@pytest.fixture(scope="module")
def fp_case():
    rgb = O.synth_frame(13, 0, FP_W, FP_H)
    marks = np.random.default_rng(13).standard_normal((130, FP_K)).astype(np.float32)
    alone = np.stack([G.fingerprint(rgb, marks[i:i + 1])[0] for i in range(130)])
    return rgb, marks, alone


@pytest.mark.parametrize("n", [65, 130])
def test_fingerprint_past_one_group(fp_case, n):
    """Copies in groups of 64 (csrc/fingerprint.hip): every copy of a later group equals its mark fingerprinted alone bit for
    bit, and the last copies meet the f32 bars against the oracle."""
    rgb, marks, alone = fp_case
    copies = G.fingerprint(rgb, marks[:n])
    for i in range(n):
        assert np.array_equal(copies[i], alone[i]), i
    for i in sorted({64, n - 1}):
        ref = O.embed_frame(rgb, marks[i])
        err, same = G.f32_stats(copies[i], ref)
        report(f"fingerprint {n} copies, copy {i} vs oracle", max_err=err, identical=same)
        G.assert_f32_bars(copies[i], ref, what=f"copy {i} vs oracle")
