"""The oracle's side of tests/test_meta_gpu.py, without a GPU: the reference must itself have every property the library is
held to -- exact covariance under scaling by powers of two on every shape of tests/meta_cases.py, what a non-finite pixel
yields -- and the generators must put their poison where they say."""
import numpy as np
import pytest

import meta_cases as M
from oracle import oracle as O

ORDERINGS = {O.ORDER_ENERGY: "Energy", O.ORDER_ENERGY_ORTHOGONAL: "EnergyOrthogonal", O.ORDER_LEGACY: "Legacy"}
METHODS = {O.OPTION1: "Option1", O.OPTION2: "Option2", O.OPTION3: "Option3"}
# every method under Energy, and the two other pairs of the GPU file's diagonal
CONFIGS = [(O.ORDER_ENERGY, m) for m in METHODS] + [(O.ORDER_ENERGY_ORTHOGONAL, O.OPTION1), (O.ORDER_LEGACY, O.OPTION3)]
DCT_TYPES = {O.DCT2: "DCT2", O.DCT2_ORTHOGONAL: "DCT2Orthogonal", O.DCT3: "DCT3"}


def frames_of(name, n=None):
    return M.frames_of(name, O.synth_frame, n)


marks_of = M.marks_of


@pytest.fixture(scope="module", params=list(M.SHAPES))
def case(request):
    """One frame of a shape with everything the oracle computes from it, unscaled."""
    name = request.param
    rgb = frames_of(name, 2)[1]
    k = M.SHAPES[name]["k"]
    mark = marks_of(name, n=2)[1]
    y, i, q = O.rgb_to_yiq(rgb)
    return dict(name=name, rgb=rgb, k=k, mark=mark, yiq=(y, i, q), coef={t: O.dct2d(y, t) for t in DCT_TYPES},
                marked={(o, m): O.embed_frame(rgb, mark, ordering=o, method=m) for o, m in CONFIGS})


# ---- generators -------------------------------------------------------------------------------------------------------------
def test_scaled_is_an_exact_power_of_two():
    a = np.random.default_rng(1).uniform(0, 1, (5, 4, 6, 3)).astype(np.float32)
    s = M.scaled(a, M.cycle_exps(5))
    assert M.cycle_exps(5) == [0, -40, 12, -12, 40]
    for i, e in enumerate(M.cycle_exps(5)):
        mant, ex = np.frexp(a[i])
        mant_s, ex_s = np.frexp(s[i])
        assert np.array_equal(mant, mant_s) and np.array_equal(ex_s[mant != 0], ex[mant != 0] + e)
    assert M.same_bits(M.scaled(s, [-e for e in M.cycle_exps(5)]), a)


@pytest.mark.parametrize("kind", M.FRAME_POISONS)
def test_frame_poison_sits_where_claimed(kind):
    a = np.random.default_rng(2).uniform(0, 1, (7, 10, 3)).astype(np.float32)
    p = M.poison(a, kind)
    sites = M.poison_sites(a.shape, kind)
    assert M.same_bits(p[~sites], a[~sites]) and sites.sum() == (a.size if kind.startswith("all") else 1)
    want = {"nan_last": np.isnan, "all_nan": np.isnan, "inf_first": np.isposinf, "ninf_middle": np.isneginf,
            "all_3e38": lambda v: v == M.BIG}[kind]
    assert np.all(want(p[sites]))
    assert {"nan_last": sites[6, 9, 2], "inf_first": sites[0, 0, 0], "ninf_middle": sites[3, 5, 1]}.get(kind, True)
    batch = np.stack([a, a, a])
    pb = M.poison_batch(batch, 1, kind)
    assert M.others_same(batch, pb, 1) == [] and M.others_same(batch, pb, 0) == [1]
    assert np.isinf(M.BIG + M.BIG) and np.isfinite(M.BIG)


@pytest.mark.parametrize("kind", M.MARK_POISONS)
def test_mark_poison_sits_where_claimed(kind):
    m = np.random.default_rng(3).standard_normal((4, 31)).astype(np.float32)
    p = M.poison_marks(m, 2, kind)
    assert M.others_same(m, p, 2) == []
    changed = np.flatnonzero(p[2].view(np.uint32) != m[2].view(np.uint32))
    assert tuple(changed) == M.mark_sites(31) == (0, 15, 30)
    assert not np.any(np.abs(p[2][changed]) < 1e38)


def test_predicates():
    a = np.array([1.0, np.nan, -0.0], np.float32)
    assert M.same_bits(a, a.copy()) and not M.same_bits(a, np.array([1.0, np.nan, 0.0], np.float32))
    b = a.copy()
    b.view(np.uint32)[1] |= 1                                  # another NaN payload
    assert not M.same_bits(a, b) and M.same_nan_mask(a, b) and not M.same_nan_mask(a, np.array([1.0, 2.0, -0.0], np.float32))


@pytest.mark.parametrize("dtype, value", M.FLAT_FRAMES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_flat_frames_have_no_ac_energy(dtype, value):
    """The AC coefficients of a flat frame are exactly zero in the oracle for the all-zero frame; for a flat frame of another
    level most are, and the rest is the round-off of its f64 FFT (below 1e-9 of the DC coefficient: 2^-52 times a few hundred
    terms).  Option 2 extraction of such a frame from itself is 0 / 0 = NaN wherever the coefficient is zero, and the
    similarity NaN: non-finite values from legal integer input."""
    s = M.SHAPES["D"]
    f = M.flat(s["h"], s["w"], dtype, value)
    rgb = O.u8_to_f32(f) if dtype == np.uint8 else O.u16_to_f32(f)
    coef = O.dct2d(O.rgb_to_yiq(rgb)[0]).reshape(-1)
    assert np.abs(coef[1:]).max() <= 1e-9 * abs(coef[0]) and np.mean(coef[1:] == 0) > 0.5
    if value == 0:
        assert np.all(coef == 0)
    mark = marks_of("D")[0]
    with np.errstate(all="ignore"):
        ext, sim = O.extract_frame(rgb, rgb, mark)
    assert np.isnan(ext).any() and np.isnan(sim)
    if value == 0:
        assert np.all(np.isnan(ext))


# ---- exact scaling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", M.EXPONENTS)
def test_planes_scale_exactly(case, e):
    s = M.pow2(e)
    rgb = case["rgb"] * s
    for got, want in zip(O.rgb_to_yiq(rgb), case["yiq"]):
        assert M.same_bits(got, want * s)
    for t, name in DCT_TYPES.items():
        assert M.same_bits(O.dct2d(case["yiq"][0] * s, t), case["coef"][t] * s), name


@pytest.mark.parametrize("e", M.EXPONENTS)
def test_index_lists_do_not_move(case, e):
    coef = case["coef"][O.DCT2]
    ks = [case["k"]] + ([M.K_GATHERED] if case["name"] == "L2" else [])
    for o, name in ORDERINGS.items():
        for k in ks:
            assert np.array_equal(O.indices(coef * M.pow2(e), o, k), O.indices(coef, o, k)), (name, k)


def test_index_lists_move_where_the_keys_overflow(case):
    """At 2^60 the largest energy keys are +inf and tie: the guard of the choice of exponents."""
    coef = case["coef"][O.DCT2]
    with np.errstate(over="ignore"):
        big = coef * M.pow2(M.OVERFLOW_EXPONENT)
        assert np.isinf(big.astype(np.float32) * big.astype(np.float32)).sum() >= 2
    assert not np.array_equal(O.indices(big, O.ORDER_ENERGY, case["k"]), O.indices(coef, O.ORDER_ENERGY, case["k"]))


@pytest.mark.parametrize("e", M.EXPONENTS)
def test_extraction_scales_exactly(case, e):
    """Base and marked frame scaled alike: the extracted mark is unchanged under Options 2 and 3 and scaled under Option 1;
    the similarity (e . m / sqrt(e . e): the scale cancels, and sqrt(2^2e) is exact) is unchanged under all three."""
    s = M.pow2(e)
    for o, m in CONFIGS:
        name = (ORDERINGS[o], METHODS[m])
        ext, sim = O.extract_frame(case["rgb"], case["marked"][(o, m)], case["mark"], ordering=o, method=m)
        ext_s, sim_s = O.extract_frame(case["rgb"] * s, case["marked"][(o, m)] * s, case["mark"], ordering=o, method=m)
        assert M.same_bits(ext_s, ext * s if m == O.OPTION1 else ext), name
        assert np.float32(sim_s).tobytes() == np.float32(sim).tobytes() and np.isfinite(sim), (name, sim, sim_s)


# ---- non-finite pixels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", M.FRAME_POISONS)
def test_a_non_finite_pixel_gives_an_all_nan_plane(case, kind):
    """One NaN, +Inf or -Inf pixel or a frame of NaN: the oracle's luma plane is non-finite there and nowhere else, and every
    coefficient of the transformed plane is NaN (the value meets every sum of both passes; Inf - Inf, or Inf beside basis
    entries of both signs).  A frame of 3e38 is recorded, not fixed: its luma plane is finite (the weights sum to 1), the sums
    of the row pass round to Inf in f32, the DC coefficient is not finite, and the AC coefficients are whatever the
    cancellation leaves."""
    rgb = M.poison(case["rgb"], kind)
    with np.errstate(all="ignore"):
        y = O.rgb_to_yiq(rgb)[0]
        coef = O.dct2d(y)
    sites = M.poison_sites(rgb.shape, kind).any(axis=2)
    if kind == "all_3e38":
        assert np.all(np.isfinite(y)) and not np.isfinite(coef[0, 0])
        return
    assert kind in M.ALL_NAN_PLANE
    assert not np.any(np.isfinite(y[sites])) and np.all(np.isfinite(y[~sites]))
    assert np.all(np.isnan(coef)), (kind, int(np.isnan(coef).sum()), coef.size)
