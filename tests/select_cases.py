"""Adversarial coefficient planes for the top-k selection (csrc/select.hip, csrc/sort_full.hip), with a numpy restatement
of the ordering and of the threshold sampler.  No fixtures: tests/test_select_cpu.py pins the restatements against the
oracle and every generator's precondition without a GPU, tests/test_select_gpu.py runs the same planes on the device.

Planes are [n, h, w] float32; a "shape" is (h, w).  The DC coefficient of every generated plane is 3e38: it is never
selected (algorithm.rs:204), and a selection that forgets to skip it ranks it first."""
from functools import lru_cache

import numpy as np

ENERGY, ENERGY_ORTHOGONAL, LEGACY = 0, 1, 2
ORDERINGS = (ENERGY, ENERGY_ORTHOGONAL, LEGACY)
ORDERING_NAMES = {ENERGY: "energy", ENERGY_ORTHOGONAL: "ortho", LEGACY: "legacy"}

MAX_K = 16384                      # longer lists: sort_full.hip (no sampler, no candidate list, not counted in the stats)
KS = (1, 63, 64, 65, 1000, 1024, 1025, 4095, 4096, 8191, 8192, 16384, 16385, 20000)
DIGIT_BITS, NBINS = 11, 2048
SHAPE_A = (256, 320)               # 81 920 elements, 16-byte aligned frames: more than the default capacity of 65 536
SHAPE_B = (211, 301)               # 63 511 elements: odd, so every frame takes the scalar loads and frames 1, 2 start misaligned
SHAPE_C = (384, 512)               # the wrong-sampler planes
DC = np.float32(3e38)
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]       # the default quiet NaN, sign clear
FLT_MAX = np.finfo(np.float32).max
M32 = np.uint64(0xFFFFFFFF)


# ---- the ordering, as the header comment of select.hip states it -----------------------------------------------------------
def ortho_scales(w, h):
    """s[first_row][first_column] of algorithm.rs:245-265 in f32: 1.0 times the row factor, times the column factor."""
    f = np.float32
    s_k0_w, s_k0_h = np.sqrt(f(1) / (f(4) * f(w))), np.sqrt(f(1) / (f(4) * f(h)))
    s_w, s_h = np.sqrt(f(1) / (f(2) * f(w))), np.sqrt(f(1) / (f(2) * f(h)))
    s = np.empty((2, 2), np.float32)
    for fr in (0, 1):
        for fc in (0, 1):
            sc = f(1) * (s_k0_w if fr else s_w)
            s[fr, fc] = sc * (s_k0_h if fc else s_h)
    return s


def scale_plane(h, w):
    """The ortho scaling of every index of an h x w plane, flat."""
    idx = np.arange(h * w)
    return ortho_scales(w, h)[(idx < w).astype(int), (idx % w == 0).astype(int)]


def keys(plane, ordering):
    """key_f32 of every coefficient (flat, DC included) exactly as algorithm.rs:214-266 forms it."""
    h, w = plane.shape
    v = np.ascontiguousarray(plane, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        if ordering == ENERGY:
            return v * v
        scaled = scale_plane(h, w) * v
        return scaled * scaled if ordering == ENERGY_ORTHOGONAL else scaled


def sortable(key):
    """f32::total_cmp order as an unsigned integer (larger == Greater)."""
    b = np.ascontiguousarray(key, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def order(plane, ordering, k=None):
    """The first k indices of obtain_indices_by_function: composite (sortable(key) << 32) | ~index, DC skipped, descending."""
    with np.errstate(all="ignore"):
        kb = sortable(keys(plane, ordering)).astype(np.uint64)
        idx = np.arange(kb.size, dtype=np.uint32)
        comp = (kb << np.uint64(32)) | (~idx).astype(np.uint64)
        out = (np.argsort(comp[1:], kind="stable")[::-1] + 1).astype(np.uint64)       # composite keys are unique
    return out if k is None else out[:k]


def tie_group_size(plane, ordering, k):
    """Members of the group of equal keys that holds rank k."""
    kb = np.sort(sortable(keys(plane, ordering))[1:])[::-1]
    return int(np.count_nonzero(kb == kb[k - 1]))


def n_pow2(k):
    n = 2
    while n < k:
        n <<= 1
    return n


# ---- the sampler: select_sample_kernel and find_threshold_digit of select.hip, restated --------------------------------------
def mix32(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def sample_stride(k):
    return 256 if k >= 8192 else 128 if k >= 4096 else 64


def capacity(k):
    return max(65536, 16 * k)


def quad_positions(plane_len, f, stride):
    """j0(g, f, stride) of every group g: the first element of the one quad in `stride` that frame number f samples."""
    group = 4 * stride
    g = np.arange((plane_len + group - 1) // group, dtype=np.uint64)
    j0 = g * np.uint64(group) + np.uint64(4) * (mix32(g * np.uint64(0x9E3779B1) + np.uint64(f)) & np.uint64(group // 4 - 1))
    return j0[j0 < plane_len].astype(np.int64)


def sampled_elements(plane_len, f, stride):
    """Indices that enter the sample histogram: the elements of the quads, clipped to the plane, without the DC."""
    j = (quad_positions(plane_len, f, stride)[:, None] + np.arange(4)[None, :]).reshape(-1)
    return j[(j < plane_len) & (j != 0)]


def threshold_digit(kb, f, k):
    """The digit whose upper tail of the 2048-bin sample histogram first holds m = max(32, ceil(3k / stride)) samples; 0 (keep
    everything) when the whole sample is smaller."""
    stride = sample_stride(k)
    hist = np.bincount(kb[sampled_elements(kb.size, f, stride)] >> np.uint32(32 - DIGIT_BITS), minlength=NBINS)
    m = max(32, (3 * k + stride - 1) // stride)
    tail = np.cumsum(hist[::-1])
    hit = np.nonzero(tail >= m)[0]
    return NBINS - 1 - int(hit[0]) if hit.size else 0


def candidate_count(plane, ordering, f, k):
    """(threshold digit, candidates appended by select_compact_kernel) of frame number f of a call."""
    with np.errstate(all="ignore"):
        key = keys(plane, ordering)
        kb = sortable(key)
        thr = threshold_digit(kb, f, k)
        if ordering == ENERGY:                 # the float-compare shortcut: !(key < lower edge of the digit), NaN edge included
            bits = np.array([(thr << (32 - DIGIT_BITS)) & 0x7FFFFFFF], np.uint32)
            edge = bits.view(np.float32)[0] if thr > (1 << (DIGIT_BITS - 1)) else np.float32(0)
            cand = ~(key < edge)
        else:
            cand = (kb >> np.uint32(32 - DIGIT_BITS)) >= thr
    cand[0] = False
    return thr, int(np.count_nonzero(cand))


def predicted_fallbacks(planes, ordering, k, cap):
    """Frames of one call whose candidate count falls outside k <= n <= cap (exact_fallback_frames grows by this)."""
    if k > MAX_K:
        return 0
    return sum(not (k <= candidate_count(p, ordering, f, k)[1] <= cap) for f, p in enumerate(planes))


# ---- generators -------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def _distinct_unit(rng, n):
    """n distinct f32 in [1 + 1000 ulp, 1.118): their squares stay below 1.25, inside the digit of 1.0."""
    i = rng.permutation(985_000)[:n].astype(np.uint32) + np.uint32(1000)
    return (np.uint32(0x3F800000) + i).view(np.float32)


def _signs(rng, n):
    return np.where(rng.random(n) < 0.5, np.float32(-1), np.float32(1)).astype(np.float32)


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)


def _finish(flat_frames, shape):
    out = np.ascontiguousarray(flat_frames, np.float32).reshape((-1,) + shape)
    out[:, 0, 0] = DC
    return out


def one_digit(shape, ordering, n_frames=1, seed=1):
    """Every non-DC key inside the digit of 1.0 (keys in [1, 1.25)), all values distinct: everything is a candidate and the
    select resolves rank k on mantissa bits.  Energy: |v| in [1, 1.118), random signs; the orthogonal orderings: the scaled
    value there (Legacy: positive, a negative key sits in another digit)."""
    h, w = shape
    rng = _rng(11, seed, h, w, ordering)
    t = _distinct_unit(rng, n_frames * h * w).reshape(n_frames, h * w)
    v = t if ordering == ENERGY else (t / scale_plane(h, w)[None, :]).astype(np.float32)
    if ordering != LEGACY:
        v = v * _signs(rng, v.size).reshape(v.shape)
    return _finish(v, shape)


TIE_TOP, TIE_DOMINANT = np.float32(12), np.float32(8)
TIE_REST = np.array([6, 4, 3, 2, 1.5, 1, 0.75, 0.5], np.float32)


def ties(shape, n_frames=1, seed=2):
    """Ten magnitudes with random signs: 700 elements of the largest, 70 % of the plane at the second largest, the rest
    shared by eight smaller ones.  Rank k <= 16384 sits in a tie group larger than any sort buffer."""
    h, w = shape
    n = h * w - 1
    rng = _rng(12, seed, h, w)
    n_dom = (7 * n) // 10
    body = np.concatenate([np.full(700, TIE_TOP), np.full(n_dom, TIE_DOMINANT), np.resize(TIE_REST, n - 700 - n_dom)])
    frames = []
    for _ in range(n_frames):
        frames.append(np.concatenate([[DC], rng.permutation(body) * _signs(rng, n)]))
    return _finish(np.stack(frames), shape)


def spikes(shape, k, ordering, seed=3):
    """Three frames with exactly k - 1, k and k + 1 large distinct values; everything else is +0.0 or -0.0."""
    h, w = shape
    n = h * w - 1
    rng = _rng(13, seed, h, w, k, ordering)
    frames = []
    for count in (k - 1, k, k + 1):
        body = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        big = _distinct_unit(rng, count) * np.exp2(rng.integers(10, 40, count)).astype(np.float32)
        if ordering != LEGACY:
            big = big * _signs(rng, count)
        body[rng.permutation(n)[:count]] = big
        frames.append(np.concatenate([[DC], body]))
    return _finish(np.stack(frames), shape)


SIGNED_POSITIVES = 5000


def signed(shape, seed=4):
    """Legacy's signed keys: an all-negative frame, a half-negative frame, a frame with 5000 positive values and the rest
    negative (a list longer than 5000 descends into the negative keys, smallest magnitude first), and a frame of only
    +0.0 and -0.0 (+0 ranks before -0; the energy orderings tie them all)."""
    h, w = shape
    n = h * w - 1
    rng = _rng(14, seed, h, w)
    mag = lambda: _log_uniform(rng, 1e-3, 1e3, n)
    few = -mag()
    few[rng.permutation(n)[:SIGNED_POSITIVES]] *= np.float32(-1)
    zeros = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    frames = [-mag(), mag() * _signs(rng, n), few, zeros]
    return _finish(np.stack([np.concatenate([[DC], b]) for b in frames]), shape)


def subnormal(shape, seed=5):
    """Keys that are subnormal.  Frame 0: 60 % |v| log-uniform in [4e-23, 1e-19] (v * v is subnormal and not zero), 20 % |v|
    in [1e-30, 1e-24] (v * v underflows to zero), 20 % true zeros.  Frame 1: half the plane |v| in [1e-43, 1e-38], subnormal
    before it is scaled (Legacy's key s * v stays subnormal), half as in frame 0.  Frame 2: frame 0 with the first class in
    [2.5e-20, 5e-17], where the square of the scaled value s * v (s about 2e-3) is subnormal and not zero."""
    h, w = shape
    n = h * w - 1
    rng = _rng(15, seed, h, w)

    def mixed(lo=4e-23, hi=1e-19):
        u = rng.random(n)
        body = _log_uniform(rng, lo, hi, n)
        body = np.where(u < 0.2, _log_uniform(rng, 1e-30, 1e-24, n), body)
        body = np.where(u > 0.8, np.float32(0), body)
        return (body * _signs(rng, n)).astype(np.float32)

    tiny = np.where(rng.random(n) < 0.5, _log_uniform(rng, 1e-43, 1e-38, n), _log_uniform(rng, 4e-23, 1e-19, n)) * _signs(rng, n)
    frames = [mixed(), tiny.astype(np.float32), mixed(2.5e-20, 5e-17)]
    return _finish(np.stack([np.concatenate([[DC], b]) for b in frames]), shape)


def overflow(shape, n_frames=1, seed=6):
    """30 % distinct |v| in [2^65, 1.118 * 2^126] (>= 1.9e19: v * v is +inf), 1 % +-FLT_MAX, 1 % +-inf, the rest N(0, 1e3): the
    +inf keys tie and come back in index order, ahead of the finite ones."""
    h, w = shape
    n = h * w - 1
    frames = []
    for f in range(n_frames):
        rng = _rng(16, seed, h, w, f)
        u = rng.random(n)
        body = (1e3 * rng.standard_normal(n)).astype(np.float32)
        huge = _distinct_unit(rng, n) * np.exp2(rng.integers(65, 127, n)).astype(np.float32) * _signs(rng, n)
        body = np.where(u < 0.30, huge, body)
        body = np.where((u >= 0.30) & (u < 0.31), FLT_MAX * _signs(rng, n), body)
        body = np.where((u >= 0.31) & (u < 0.32), np.float32(np.inf) * _signs(rng, n), body)
        frames.append(np.concatenate([[DC], body.astype(np.float32)]))
    return _finish(np.stack(frames), shape)


def heavy_tail(shape, n_frames=1, seed=7):
    """The control: a 100 / (1 + u + v) spectrum times Laplace noise, 200 exact duplicates injected (half with the sign
    flipped: energy ties)."""
    h, w = shape
    u, v = np.mgrid[0:h, 0:w]
    spec = (100.0 / (1.0 + u + v)).reshape(-1)
    frames = []
    for f in range(n_frames):
        rng = _rng(17, seed, h, w, f)
        body = (spec * rng.laplace(size=h * w)).astype(np.float32)
        pos = rng.permutation(h * w - 1)[:400] + 1
        body[pos[200:]] = body[pos[:200]] * np.where(np.arange(200) % 2 == 0, np.float32(1), np.float32(-1))
        frames.append(body)
    return _finish(np.stack(frames), shape)


NAN_FEW, NAN_MANY_FRACTION = 5, 0.73


def nans(shape, seed=8):
    """+qNaN (0x7FC00000) keys on heavy-tail planes.  Frame 0: five of them; frame 1: 73 % of the plane, more than 3k for
    every k <= 16384, so the sampled threshold digit is the NaN digit itself; frame 2: five again."""
    h, w = shape
    n = h * w - 1
    rng = _rng(18, seed, h, w)
    out = heavy_tail(shape, 3, seed=80 + seed)
    flat = out.reshape(3, -1)
    for f, count in enumerate((NAN_FEW, int(NAN_MANY_FRACTION * n), NAN_FEW)):
        flat[f, rng.permutation(n)[:count] + 1] = QNAN
    return out


def blind(shape, f, k, seed=9):
    """A heavy-tail plane with +0.0 at every quad that frame number f samples for this k: the threshold keeps everything."""
    h, w = shape
    out = heavy_tail(shape, 1, seed=900 + 10 * seed + f)
    flat = out.reshape(-1)
    q = quad_positions(h * w, f, sample_stride(k))
    j = (q[:, None] + np.arange(4)[None, :]).reshape(-1)
    flat[j[j < h * w]] = np.float32(0)
    flat[0] = DC
    return out[0]


def dazzled(shape, f, k, seed=10):
    """Noise of 1e-3 with large, log-uniform, distinct values at the quads that frame number f samples for this k, and nowhere
    else: the threshold sits among them and fewer than k candidates result."""
    h, w = shape
    rng = _rng(20, seed, h, w, f, k)
    flat = (1e-3 * rng.standard_normal(h * w)).astype(np.float32)
    q = quad_positions(h * w, f, sample_stride(k))
    j = (q[:, None] + np.arange(4)[None, :]).reshape(-1)
    j = j[j < h * w]
    flat[j] = _distinct_unit(rng, j.size) * np.exp2(rng.integers(5, 60, j.size)).astype(np.float32) * _signs(rng, j.size)
    return _finish(flat[None], shape)[0]


# ---- the cases --------------------------------------------------------------------------------------------------------------
DISTRIBUTIONS = ("one_digit", "ties", "spikes", "signed", "subnormal", "overflow", "nan", "heavy_tail")


@lru_cache(maxsize=None)
def distribution(name, ordering):
    """Group A: [(k tuple, planes)] -- the batches one distribution is run on with one ordering.  Every batch but the spike
    counts (made for one k each) is run with every k of KS."""
    both = lambda make: [(KS, make(SHAPE_A)), (KS, make(SHAPE_B))]
    if name == "one_digit":
        return both(lambda s: one_digit(s, ordering, 3 if s == SHAPE_B else 1))
    if name == "ties":
        return both(lambda s: ties(s, 3 if s == SHAPE_B else 1))
    if name == "spikes":
        return [((k,), spikes(SHAPE_B if k in (63, 4095, 8191) else SHAPE_A, k, ordering)) for k in KS]
    if name == "signed":
        return [(KS, signed(SHAPE_A)), (KS, signed(SHAPE_B)[[0, 2, 3]])]
    if name == "subnormal":
        return both(subnormal)
    if name == "overflow":
        return both(lambda s: overflow(s, 3 if s == SHAPE_B else 1))
    if name == "nan":
        return [(KS, nans(SHAPE_A)[:2]), (KS, nans(SHAPE_B))]
    if name == "heavy_tail":
        return both(lambda s: heavy_tail(s, 3 if s == SHAPE_B else 2))
    raise KeyError(name)


# Group B through the default capacity max(65536, 16k): (w, h, k, fallbacks); one-digit planes, so n = w h - 1 exactly
BOUNDARY_DEFAULT = ((65537, 1, 1000, 0), (1, 65537, 1000, 0), (10923, 6, 1000, 1),
                    (8889, 9, 5000, 0), (40001, 2, 5000, 1))


def boundary_capped(k):
    """Group B with an explicit candidate capacity C: (C, plane length, fallbacks per frame, what)."""
    out = []
    for c in (k, k + 1):
        out += [(c, c + 1, 0, "n == cap"), (c, c + 2, 1, "n == cap + 1"), (c, k + 1, 0, "n == k: the immediate exit")]
    out += [(k - 1, k + 1, 1, "cap < k"), (k - 1, k + 3, 1, "cap < k")]
    return out


WRONG_KS = (1000, 4096)            # sample strides 64 and 128


@lru_cache(maxsize=None)
def wrong_sampler(kind, k):
    """Group C: three frames of SHAPE_C, only frame 1 adversarial for this k."""
    reg = heavy_tail(SHAPE_C, 3, seed=31)
    bad = blind(SHAPE_C, 1, k) if kind == "blind" else dazzled(SHAPE_C, 1, k)
    return np.stack([reg[0], bad, reg[2]])


@lru_cache(maxsize=None)
def state_calls():
    """Group D: [(k, planes, kinds)] -- three calls made on one context, in this order and in the reverse order."""
    k1, k3 = 1000, 4096
    reg = heavy_tail(SHAPE_C, 4, seed=41)
    call1 = np.stack([blind(SHAPE_C, 0, k1), dazzled(SHAPE_C, 1, k1), dazzled(SHAPE_C, 2, k1), blind(SHAPE_C, 3, k1)])
    call3 = np.stack([reg[2], blind(SHAPE_C, 1, k3), dazzled(SHAPE_C, 2, k3), reg[3], dazzled(SHAPE_C, 4, k3), blind(SHAPE_C, 5, k3)])
    return [(k1, call1, 4), (k1, reg[:2].copy(), 0), (k3, call3, 4)]
