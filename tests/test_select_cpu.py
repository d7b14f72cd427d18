"""The planes of tests/select_cases.py without a GPU: the numpy restatement of the ordering equals the oracle's list on every
case (the full list and every prefix the GPU test asks for), and every generator still produces what it was built for --
a case that stops reaching its branch of csrc/select.hip fails here, not silently on the device."""
import numpy as np
import pytest

import select_cases as SC
from oracle import oracle as O

NAMES = SC.ORDERING_NAMES
SELECT_KS = [k for k in SC.KS if k <= SC.MAX_K]


def assert_orders_agree(plane, ordering, ks, what):
    full = O.indices(plane, ordering)
    mine = SC.order(plane, ordering)
    assert np.array_equal(mine, full), (what, "full list")
    for k in ks:
        assert np.array_equal(O.indices(plane, ordering, k=k), full[:k]), (what, k)
    return full


def digits(plane, ordering):
    return SC.sortable(SC.keys(plane, ordering))[1:] >> np.uint32(21)


def check_one_digit(planes, ordering):
    for f, p in enumerate(planes):
        assert np.unique(digits(p, ordering)).size == 1
        distinct = np.unique(np.abs(p.reshape(-1)[1:])).size          # (t / s rounds a few scaled values onto each other)
        assert distinct == p.size - 1 if ordering == SC.ENERGY else distinct > 0.999 * p.size, "values are distinct"
        for k in SELECT_KS:
            assert SC.candidate_count(p, ordering, f, k)[1] == p.size - 1, "everything is a candidate"


def check_ties(planes, ordering):
    for p in planes:
        assert np.count_nonzero(np.abs(p.reshape(-1)[1:]) == SC.TIE_DOMINANT) == (7 * (p.size - 1)) // 10
        for k in SELECT_KS:
            assert SC.tie_group_size(p, ordering, k) > SC.n_pow2(k), k
        assert SC.tie_group_size(p, ordering, 4096) > SC.MAX_K


def check_spikes(planes, ordering, k):
    for p, count in zip(planes, (k - 1, k, k + 1)):
        body = p.reshape(-1)[1:]
        big = body[body != 0]
        assert big.size == count and np.unique(np.abs(big)).size == count and np.all(np.abs(big) >= 1024)
        zero = body[body == 0]
        assert 0 < np.count_nonzero(np.signbit(zero)) < zero.size, "+0.0 and -0.0"


def check_signed(planes, ordering):
    flat = planes.reshape(len(planes), -1)[:, 1:]
    assert np.all(flat[0] < 0)
    few = flat[-2]
    assert np.count_nonzero(few > 0) == SC.SIGNED_POSITIVES < max(SELECT_KS) and np.count_nonzero(few < 0) == few.size - SC.SIGNED_POSITIVES
    if len(planes) == 4:
        assert abs(np.count_nonzero(flat[1] < 0) - flat[1].size / 2) < 0.01 * flat[1].size
    zeros = flat[-1]
    assert np.all(zeros == 0) and 0 < np.count_nonzero(np.signbit(zeros)) < zeros.size
    if ordering == SC.LEGACY:
        # the negative keys rank smallest magnitude first; +0 ranks before -0, each in index order
        order = SC.order(planes[0], ordering)
        scaled = SC.keys(planes[0], ordering)[order.astype(np.int64)]
        assert np.all(np.diff(scaled) <= 0)
        plus, minus = np.nonzero(~np.signbit(zeros))[0] + 1, np.nonzero(np.signbit(zeros))[0] + 1
        assert np.array_equal(SC.order(planes[-1], ordering), np.concatenate([plus, minus]))
    else:
        assert np.array_equal(SC.order(planes[-1], ordering), np.arange(1, zeros.size + 1))


def check_subnormal(planes, ordering):
    tiny = np.finfo(np.float32).tiny
    counts = []
    for p in planes:
        key = np.abs(SC.keys(p, ordering)[1:])
        counts.append(np.count_nonzero((key > 0) & (key < tiny)))
    assert max(counts) > 20000, counts                          # more than any k: rank k is a subnormal key
    if ordering == SC.ENERGY:
        v = planes[0].reshape(-1)[1:]
        assert np.count_nonzero((v != 0) & (SC.keys(planes[0], ordering)[1:] == 0)) > 1000, "squares that underflow to zero"
        assert np.count_nonzero(v == 0) > 1000, "true zeros"


def check_overflow(planes, ordering):
    for p in planes:
        v, key = p.reshape(-1), SC.keys(p, ordering)
        assert np.count_nonzero(v == SC.FLT_MAX) > 100 and np.count_nonzero(np.isinf(v)) > 100
        assert np.count_nonzero(np.isfinite(key[1:])) > 20000, "finite keys beside them"
        big = (np.abs(v[1:]) >= 1.9e19) & np.isfinite(v[1:])
        assert np.unique(np.abs(v[1:][big])).size >= np.count_nonzero(big) - np.count_nonzero(np.abs(v) == SC.FLT_MAX)
        top = np.nonzero(key[1:] == np.inf)[0] + 1
        if ordering == SC.ENERGY:
            assert top.size == np.count_nonzero(np.abs(v[1:]) >= 1.9e19) > SC.MAX_K, "|v| >= 1.9e19 squares to +inf"
        assert top.size > 100
        assert np.array_equal(SC.order(p, ordering, top.size), top), "+inf keys tie: index order"


def check_nan(planes, ordering):
    for f, p in enumerate(planes):
        v = p.reshape(-1)
        nan = np.nonzero(np.isnan(v))[0]
        assert np.all(v[nan].view(np.uint32) == 0x7FC00000)
        assert nan.size == (int(SC.NAN_MANY_FRACTION * (p.size - 1)) if f == 1 else SC.NAN_FEW)
        assert np.all(SC.keys(p, ordering)[nan].view(np.uint32) == 0x7FC00000), "the host's products keep the default NaN"
        assert np.array_equal(SC.order(p, ordering, nan.size), nan), "NaN keys rank first, in index order"
        if f == 1:
            for k in SELECT_KS:
                if nan.size > 3.3 * k:             # (the smaller shape holds fewer than 3 x 16384 NaNs)
                    assert SC.candidate_count(p, ordering, f, k)[0] == 0x7FE, "the threshold digit is the NaN digit"
    assert SC.candidate_count(planes[1], ordering, 1, 1000)[0] == 0x7FE


def check_heavy_tail(planes, ordering):
    for k in SELECT_KS:
        assert SC.predicted_fallbacks(planes, ordering, k, SC.capacity(k)) == 0, k
    body = np.abs(planes[0].reshape(-1)[1:])
    assert body.size - np.unique(body).size >= 200, "exact duplicates"


CHECKS = {"one_digit": check_one_digit, "ties": check_ties, "signed": check_signed, "subnormal": check_subnormal,
          "overflow": check_overflow, "nan": check_nan, "heavy_tail": check_heavy_tail}


@pytest.mark.parametrize("ordering", SC.ORDERINGS, ids=NAMES.get)
@pytest.mark.parametrize("name", SC.DISTRIBUTIONS)
def test_key_distributions(name, ordering):
    for ks, planes in SC.distribution(name, ordering):
        for f, p in enumerate(planes):
            assert_orders_agree(p, ordering, ks, (name, p.shape, f))
        if name == "spikes":
            check_spikes(planes, ordering, ks[0])
        else:
            CHECKS[name](planes, ordering)


def test_restated_keys_are_the_oracles():
    """The f32 key of every ordering, bit for bit (sign included), on values of every class the planes use."""
    import ctypes as C
    h, w = 5, 7
    v = np.array([0.0, -0.0, 1.5, -1.5, 3e-23, -1e-40, 2e19, -SC.FLT_MAX, np.inf, -np.inf, 1e-3], np.float32)
    plane = np.resize(v, h * w).reshape(h, w)
    for ordering in SC.ORDERINGS:
        want = [O.lib().sswo_order_key(ordering, w, h, i, C.c_float(plane.reshape(-1)[i])) for i in range(h * w)]
        got = SC.sortable(SC.keys(plane, ordering)).astype(np.int64) - (1 << 31)
        assert np.array_equal(got, np.array(want, np.int64)), ordering


@pytest.mark.parametrize("ordering", SC.ORDERINGS, ids=NAMES.get)
def test_boundary_planes_have_the_predicted_candidate_count(ordering):
    for w, h, k, fallbacks in SC.BOUNDARY_DEFAULT:
        p = SC.one_digit((h, w), ordering)[0]
        assert_orders_agree(p, ordering, (k,), (w, h))
        assert np.unique(digits(p, ordering)).size == 1
        n = SC.candidate_count(p, ordering, 0, k)[1]
        assert n == w * h - 1 and n == SC.capacity(k) + fallbacks
        assert SC.predicted_fallbacks(p[None], ordering, k, SC.capacity(k)) == fallbacks
    for k in (1000, 5000):
        for cap, length, fallbacks, what in SC.boundary_capped(k):
            planes = SC.one_digit((1, length), ordering, 2)
            for f, p in enumerate(planes):
                assert_orders_agree(p, ordering, (k,), (cap, length))
                assert SC.candidate_count(p, ordering, f, k)[1] == length - 1, what
            assert SC.predicted_fallbacks(planes, ordering, k, cap) == 2 * fallbacks, what


@pytest.mark.parametrize("ordering", [SC.ENERGY, SC.LEGACY], ids=NAMES.get)
@pytest.mark.parametrize("k", SC.WRONG_KS)
@pytest.mark.parametrize("kind", ["blind", "dazzled"])
def test_wrong_sampler_planes_mislead_one_frame_only(kind, k, ordering):
    planes = SC.wrong_sampler(kind, k)
    cap = SC.capacity(k)
    counts = [SC.candidate_count(p, ordering, f, k)[1] for f, p in enumerate(planes)]
    assert k <= counts[0] <= cap and k <= counts[2] <= cap, counts
    assert counts[1] > cap if kind == "blind" else counts[1] < k, counts
    # the same plane under a neighbour's frame number is sampled elsewhere and selects normally
    if kind == "dazzled":
        assert SC.candidate_count(planes[1], ordering, 0, k)[1] >= k
    for f, p in enumerate(planes):
        assert np.array_equal(SC.order(p, ordering, k), O.indices(p, ordering, k=k)), f


def test_state_calls_fall_back_as_declared():
    for k, planes, fallbacks in SC.state_calls():
        for ordering in (SC.ENERGY, SC.LEGACY):
            assert SC.predicted_fallbacks(planes, ordering, k, SC.capacity(k)) == fallbacks, (k, ordering)
        for p in planes:
            assert np.array_equal(SC.order(p, SC.ENERGY, k), O.indices(p, SC.ENERGY, k=k))


def test_sampler_restatement_basics():
    """One quad per group, inside its group, moving with the frame number; m and the strides of select.hip."""
    for stride in (64, 128, 256):
        n = 196608
        q0, q1 = SC.quad_positions(n, 0, stride), SC.quad_positions(n, 1, stride)
        assert q0.size == n // (4 * stride) and np.all(q0 % 4 == 0)
        assert np.array_equal(q0 // (4 * stride), np.arange(q0.size))
        assert np.count_nonzero(q0 != q1) > q0.size // 2
    assert [SC.sample_stride(k) for k in (4095, 4096, 8191, 8192)] == [64, 128, 128, 256]
    assert SC.capacity(1000) == 65536 and SC.capacity(5000) == 80000
