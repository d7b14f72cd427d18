"""The planted-spectrum cases of tests/fingerprint_cases.py against the oracle, on the CPU: each case's index list is the planted
one and touches exactly the R first-pass lines it is named after, so tests/test_fingerprint_hard_gpu.py cannot quietly test
another R."""
import numpy as np
import pytest

import fingerprint_cases as FC
from oracle import oracle as O

CASES = FC.line_plan_cases()


def energy(coef):
    return coef.reshape(-1).astype(np.float64) ** 2          # what ORDER_ENERGY sorts by


def lines_of(idx, w, h):
    return {FC.line_pos(w, h, int(i) // w, int(i) % w)[0] for i in idx}


def test_the_case_table():
    assert len(CASES) == len(FC.SHAPES) * len(FC.R_VALUES)
    assert {(w, h) for w, h, _ in CASES.values()} == set(FC.SHAPES)
    for w, h in FC.SHAPES:
        assert {FC.named_R(n, w, h) for n, (cw, ch, _) in CASES.items() if (cw, ch) == (w, h)} == {1, 15, 16, 17, 32, 33, min(w, h)}


@pytest.mark.parametrize("name", list(CASES))
def test_planted_case(name):
    w, h, coords = CASES[name]
    lb, la = FC.first_pass_lines(w, h)
    R, k = FC.named_R(name, w, h), len(coords)
    lp = [FC.line_pos(w, h, u, v) for u, v in coords]
    lines, positions = [l for l, _ in lp], [p for _, p in lp]
    # the shape of the case itself
    assert len(set(lines)) == R
    assert lb - 1 in lines and 0 in positions and la - 1 in positions
    if R == 1:
        assert k == 40 and set(lines) == {lb - 1}
    else:
        assert 0 in lines
        per_line = np.bincount(lines, minlength=lb)
        assert per_line[per_line > 0].min() >= 2
        assert np.sum(np.bincount(positions, minlength=la) >= 2) >= 2, "positions shared across lines"
        # a slot's entries are not in position order in the list: the per-slot sort (by rank) is not the identity on positions
        unsorted = sum(1 for l in set(lines) if [p for ll, p in lp if ll == l] != sorted(p for ll, p in lp if ll == l))
        assert unsorted >= R // 4
    # the frame
    rgb = FC.case_frame(name)
    assert rgb.dtype == np.float32 and rgb.shape == (h, w, 3)
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 0], rgb[..., 2])
    coef = O.dct2d(O.rgb_to_yiq(rgb)[0])
    want = FC.flat(coords, w)
    idx = O.indices(coef, k=k)
    assert np.array_equal(idx, want)
    assert len(lines_of(idx, w, h)) == R
    e = energy(coef)
    rest = e.copy()
    rest[want.astype(np.int64)] = 0.0
    rest[0] = 0.0
    assert e[int(want[-1])] >= 1e3 * rest.max(), (e[int(want[-1])], rest.max())
    # the 8-bit form of the frame (what the rgb8 entry points are given): quantisation noise may swap neighbours of the list,
    # but its list still touches R lines
    c8 = O.dct2d(O.rgb_to_yiq(O.u8_to_f32(O.f32_to_u8(rgb)))[0])
    assert len(lines_of(O.indices(c8, k=k), w, h)) == R


def test_generator_rejects_duplicates_dc_and_out_of_range():
    with pytest.raises(ValueError):
        FC.planted_frame(8, 8, [(1, 2), (3, 4), (1, 2)], 0)
    with pytest.raises(ValueError):
        FC.planted_frame(8, 8, [(0, 0), (1, 1)], 0)
    with pytest.raises(ValueError):
        FC.planted_frame(8, 8, [(8, 1)], 0)


def test_amplitudes_descend_and_sum():
    """One planted coefficient per list entry, 4 % apart, whatever its zero frequencies; |pixel - 0.5| <= 0.45."""
    w, h, coords = CASES["96x40-R17"]
    rgb = FC.case_frame("96x40-R17")
    c = np.abs(O.dct2d(O.rgb_to_yiq(rgb)[0]).reshape(-1)[FC.flat(coords, w).astype(np.int64)].astype(np.float64))
    assert np.allclose(c[:-1] / c[1:], FC.DECAY, rtol=1e-4)
    assert np.abs(rgb.astype(np.float64) - 0.5).max() <= FC.AMPLITUDE_SUM + 1e-6
