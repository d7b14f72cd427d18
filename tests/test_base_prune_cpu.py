"""The key bound of the base-reader pruning (csrc/base_prune.hip), restated in numpy against the oracle's transform:
with r = the f32 row-pass values and E[v] = sum_y r(y, v)^2 accumulated in f32, every key c(u, v)^2 of column v is at most
boundkey(v) = G E[v], G = 4 H (1 + 2^-5) rounded up -- on random, smooth and adversarial planes."""
import numpy as np
import pytest

from oracle import oracle as O


def gain(h):
    return np.nextafter(np.float32(4.0 * h * (1.0 + 1.0 / 32.0)), np.float32(np.inf))


def row_pass(plane):
    """The f32 plane between the passes (dct2d.rs:152-168): the oracle's 1-D transform of every row, times 2."""
    return np.stack([np.float32(2.0) * O.dct1d(r) for r in plane]).astype(np.float32)


def bound_and_keys(plane):
    h, w = plane.shape
    r = row_pass(plane)
    e = np.zeros(w, np.float32)
    for y in range(h):                                   # f32 accumulation, one row at a time
        e = (e + r[y] * r[y]).astype(np.float32)
    coef = np.stack([np.float32(2.0) * O.dct1d(r[:, v]) for v in range(w)], axis=1).astype(np.float32)
    full = O.dct2d(plane)
    assert np.array_equal(coef, full), "the restated passes are the oracle's transform"
    return (gain(h) * e).astype(np.float32), (coef * coef).astype(np.float32)


def planes():
    rng = np.random.default_rng(3)
    h, w = 48, 64                                         # rows first (w >= h), as in the fused path
    y, x = np.mgrid[0:h, 0:w]
    yield "uniform noise", rng.uniform(0, 1, (h, w)).astype(np.float32)
    yield "gaussian", rng.standard_normal((h, w)).astype(np.float32)
    yield "constant", np.full((h, w), 0.75, np.float32)
    yield "dc column (u = 0 is the row that needs the factor 4)", np.cos(np.pi * (2 * x + 1) * 5 / (2 * w)).astype(np.float32)
    yield "one cosine", (np.cos(np.pi * (2 * x + 1) * 7 / (2 * w)) * np.cos(np.pi * (2 * y + 1) * 9 / (2 * h))).astype(np.float32)
    yield "nyquist rows", (np.where(y % 2 == 0, 1.0, -1.0) * np.ones((h, w))).astype(np.float32)
    yield "impulse", np.eye(h, w, dtype=np.float32) * np.float32(1e6)
    yield "tiny", (rng.standard_normal((h, w)) * 1e-12).astype(np.float32)
    yield "huge", (rng.standard_normal((h, w)) * 1e12).astype(np.float32)


@pytest.mark.parametrize("name, plane", list(planes()), ids=[n.split(" (")[0] for n, _ in planes()])
def test_every_key_is_below_the_bound(name, plane):
    bound, keys = bound_and_keys(plane)
    assert np.all(keys <= bound[None, :]), name
    # and the bound is not loose by more than the factor the u = 0 row needs, plus the margin
    col = keys.sum(axis=0, dtype=np.float64)
    assert np.all(bound.astype(np.float64) <= 2.2 * col + 1e-30), name
