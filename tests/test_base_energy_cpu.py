"""The low-precision tail bound of the base-reader pruning (csrc/base_energy.hip), restated in numpy: operands
and bases as float16 hi + lo halves (the bases scaled by 2^10), three products per term, f32 accumulation.  The documented
per-element bound (|a~1 +/- a~2| + err1 + err2) f, raised by (1 + 2^-20)^2, must be >= the |r32| the exact launches produce --
on adversarial lines, for every accumulation order and for a truncating adder as well as a rounding one -- and on the
synthetic 4K frames of the benchmark it must leave the needed column tiles at [0, 1]."""
import math

import numpy as np
import pytest

from oracle import oracle as O

# the constants of base_energy.hip
BSCALE = np.float32(1024.0)
K1 = np.float32(1.0) + np.float32(2.0 ** -20)
BMAX = np.float32(2.0) * K1                       # forward bases are 2 cos / 2 sin; the split kernel rounds its maximum up


def c_s(kp, b=BMAX):
    n_ops = np.float32(kp + kp // 16 + 16)
    return np.float32((b * (np.float32(3.0) * np.float32(2.0 ** -21) + np.float32(1.02) * n_ops * np.float32(2.0 ** -23)) + np.float32(2.0 ** -23)) * K1)


def c_a(kp, b=BMAX):
    return np.float32(np.float32(1.01) * np.float32(kp) * b * np.float32(2.0 ** -13) * K1 + np.float32(1e-30))


def split16(v32):
    with np.errstate(all="ignore"):
        hi = v32.astype(np.float16)
        lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def trunc32(v64):
    """v64 (float64) to float32, rounded toward zero."""
    f = v64.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(v64)
    return np.where(over, np.nextafter(f, np.float32(0.0)), f).astype(np.float32)


def add32(a, b, truncate):
    s = a.astype(np.float64) + b.astype(np.float64)
    return trunc32(s) if truncate else s.astype(np.float32)


def accumulate(terms, order, truncate):
    """sum over axis -1 of float32 terms, every addition rounded (or truncated) to float32."""
    k = terms.shape[-1]
    if order == "pairwise":
        t = terms
        while t.shape[-1] > 1:
            if t.shape[-1] % 2:
                t = np.concatenate([t, np.zeros(t.shape[:-1] + (1,), np.float32)], axis=-1)
            t = add32(t[..., 0::2], t[..., 1::2], truncate)
        return t[..., 0]
    idx = range(k) if order == "ascending" else range(k - 1, -1, -1)
    acc = np.zeros(terms.shape[:-1], np.float32)
    for i in idx:
        acc = add32(acc, terms[..., i], truncate)
    return acc


def lowp_product(x, b, order, truncate):
    """(a~, S): the kernel's value of sum_k x_k b_k and the line's sum |x_k| (f32), for x [lines][K], b [rows][K] (float64)."""
    xf = x.astype(np.float32)
    xh, xl = split16(xf)
    bh, bl = split16((b * float(BSCALE)).astype(np.float32))
    f = lambda a: a.astype(np.float32)
    with np.errstate(all="ignore"):
        hh = f(xh)[:, None, :] * f(bh)[None, :, :]                      # exact in f32: 11 x 11 bits
        corr = f(xh)[:, None, :] * f(bl)[None, :, :], f(xl)[:, None, :] * f(bh)[None, :, :]
        acc = accumulate(hh, order, truncate)
        t = accumulate(np.concatenate(corr, axis=-1), order, truncate)
        acc = add32(acc, t, truncate)
        s = accumulate(np.abs(xf), "ascending", False)
    return acc * (np.float32(1.0) / BSCALE), s


def bound_elem(a1, a2, s1, s2, kp, pm, factor=np.float32(1.0)):
    """The two per-element bounds of a class, as the kernel forms them (f32 arithmetic)."""
    e1 = ((s1 * c_s(kp) + c_a(kp)) * K1)[:, None]
    e2 = ((s2 * c_s(kp) + c_a(kp)) * K1)[:, None]
    fac = np.abs(factor) * K1
    with np.errstate(all="ignore"):
        if pm:
            o1, o2, e1, e2 = np.abs(a1 + a2), np.abs(a1 - a2), e1 + e2, e1 + e2
        else:
            o1, o2 = np.abs(a1), np.abs(a2)
        return (o1 + e1) * K1 * fac, (o2 + e2) * K1 * fac


def exact32(x, b, factor=np.float32(1.0)):
    """r32 of the exact launches: the f64 sum rounded to f32, times the f32 factor."""
    out = np.empty((x.shape[0], b.shape[0]), np.float64)
    for i in range(x.shape[0]):
        for j in range(b.shape[0]):
            out[i, j] = math.fsum(x[i] * b[j])
    return out


K = 240                       # the sum length of a 4K row class (3840 / 16)


def lines():
    rng = np.random.default_rng(7)
    n = np.arange(K)
    out = {
        "alternating": np.where(n % 2 == 0, 1.0, -1.0),
        "ones": np.ones(K),
        "spike": np.where(n == 17, 1.0, 0.0),
        "1e-7": np.full(K, 1e-7) * rng.choice([-1.0, 1.0], K),
        "1e-3": np.full(K, 1e-3) * rng.uniform(0.5, 1.0, K),
        "6e4": np.full(K, 6e4) * rng.choice([-1.0, 1.0], K),
        "dc dwarfs detail": 1000.0 + 1e-3 * rng.standard_normal(K),
        "dc dwarfs detail, f64 grain": 15.0 + 1e-9 * rng.standard_normal(K),
        "noise": rng.standard_normal(K),
    }
    names = list(out)
    return names, np.stack([out[k] for k in names])


def bases():
    """rows of the quarter-length cosine / sine bases of a rotated class (dct_pair_prep.hip: 2 cos / 2 sin(2 pi j (2 n + 1) / N),
    N = 8 K), low, middle and the highest rows."""
    n = np.arange(K)
    js = np.array([128, 129, 200, 255, 256, 2 * K - 2, 2 * K - 1])
    arg = 2.0 * np.pi * js[:, None] * (2 * n[None, :] + 1) / (8 * K)
    return 2.0 * np.cos(arg), 2.0 * np.sin(arg)


@pytest.mark.parametrize("truncate", [False, True], ids=["rounding", "truncating"])
@pytest.mark.parametrize("order", ["ascending", "descending", "pairwise"])
def test_bound_covers_the_exact_value_on_adversarial_lines(order, truncate):
    names, x = lines()
    cosb, sinb = bases()
    # both products of a rotated class: operand lines i (cosine part) and its neighbour (sine part), and the +/- combination
    x1, x2 = x, np.roll(x, 1, axis=0)
    a1, s1 = lowp_product(x1, cosb, order, truncate)
    a2, s2 = lowp_product(x2, sinb, order, truncate)
    r1, r2 = exact32(x1, cosb), exact32(x2, sinb)
    for factor in (np.float32(1.0), np.float32(math.sqrt(1.0 / (2.0 * 3840.0)))):
        for pm in (1, 0):
            b1, b2 = bound_elem(a1, a2, s1, s2, K, pm, factor)
            t1 = (r1 + r2 if pm else r1).astype(np.float32) * factor
            t2 = (r1 - r2 if pm else r2).astype(np.float32) * factor
            for b, t in ((b1, t1), (b2, t2)):
                bad = ~(b >= np.abs(t))
                assert not bad.any(), (order, truncate, pm, [names[i] for i in np.nonzero(bad.any(axis=1))[0]])
    # ... and the bound is not vacuous: on plain noise it is within 1 % of the value's scale
    i = names.index("noise")
    b1, _ = bound_elem(a1, a2, s1, s2, K, 1)
    assert np.all(b1[i] <= np.abs((r1 + r2)[i]) + 0.01 * np.abs(x[i]).sum())


def test_overflowing_operands_give_non_finite_bounds():
    x = np.full((1, K), 7e4)
    cosb, sinb = bases()
    a1, s1 = lowp_product(x, cosb, "ascending", False)
    b1, b2 = bound_elem(a1, a1, s1, s1, K, 1)
    assert not np.isfinite(b1).any() and not np.isfinite(b2).any()


def row_transform(y):
    """2 sum_x y[x] cos(pi v (2 x + 1) / 2 W) for every row, in f64."""
    w = y.shape[-1]
    f = np.fft.rfft(y.astype(np.float64), n=2 * w, axis=-1)[..., :w]
    return 2.0 * (f * np.exp(-1j * np.pi * np.arange(w) / (2 * w))).real


@pytest.mark.parametrize("frame", [0, 5])
def test_synthetic_4k_frames_keep_tiles_0_and_1(frame):
    """The benchmark's frames (k = 1000): head columns (below 1016) with their exact energies, every other column with the
    bound at the constants of the kernel and the generous line norm S1 + S2 <= 2 sum |Y| (two rotation levels): the needed
    column tiles stay [0, 1]."""
    w, h, k = 3840, 2160, 1000
    y = O.rgb_to_yiq(O.synth_frame(1, frame, w, h))[0].astype(np.float32)
    r32 = row_transform(y).astype(np.float32)
    coef0 = row_transform(r32[:, :128].T).T.astype(np.float32)                  # column pass of tile 0
    keys = (coef0 * coef0).astype(np.float32).reshape(-1)[1:]
    kth = np.partition(keys, keys.size - k)[keys.size - k]
    t = (np.array([kth], np.float32).view(np.uint32) & np.uint32(0xFFE00000)).view(np.float32)[0]
    g = np.nextafter(np.float32(4.0 * h * (1.0 + 1.0 / 32.0)), np.float32(np.inf))
    kp = w // 16
    s = np.float32(2.0) * np.abs(y).sum(axis=1, dtype=np.float64).astype(np.float32)
    err = ((s * c_s(kp) + np.float32(2.0) * c_a(kp)) * K1)[:, None]
    e_exact = (r32.astype(np.float64) ** 2).sum(axis=0)
    e_bound = ((((np.abs(r32) + err) * K1 * K1).astype(np.float64)) ** 2).sum(axis=0) * float(K1)
    e = np.where(np.arange(w) < 1016, e_exact, e_bound)
    need = [0] + [tile for tile in range(1, w // 128) if not np.all(float(g) * e[tile * 128:(tile + 1) * 128] * (1 + 2.0 ** -20) < float(t))]
    assert need == [0, 1], (need, float(t) / float(g))
