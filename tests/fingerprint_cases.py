"""Frames whose index list is chosen, not found: a grey frame that is a sum of a few DCT basis functions has exactly those
coefficients on top of its ORDER_ENERGY list, in the order of their amplitudes.  csrc/fingerprint.hip builds its line plan from
that list (R = the number of distinct first-pass lines in it), so these frames put R, the entries per line and the lines and
positions at the plan's edges under a test's control.  tests/test_fingerprint_cases_cpu.py checks every case against the
oracle; tests/test_fingerprint_hard_gpu.py runs them."""
import numpy as np

AMPLITUDE_SUM = 0.45         # sum of the |a_i|: every pixel stays within 0.5 -+ 0.45
DECAY = 1.04                 # a_i / a_(i+1): 4 % between neighbours of the list, far above f32 noise (about 1e-7 relative)


def first_pass_lines(w, h):
    """(lb, la): the number of first-pass lines of the inverse and their length (rows first when w >= h, src/dct2d.rs:93-98)."""
    return (h, w) if w >= h else (w, h)


def line_pos(w, h, u, v):
    """(first-pass line, position along it) of the coefficient at row u, column v."""
    return (u, v) if w >= h else (v, u)


def flat(coords, w):
    """Flat coefficient indices of (u, v) = (row, column) pairs, as the index list holds them."""
    return np.array([u * w + v for u, v in coords], np.uint64)


def planted_frame(w, h, coords, seed):
    """Grey f32 frame [h, w, 3]: 0.5 + sum_i a_i s_i cos(pi u_i (2y + 1) / 2h) cos(pi v_i (2x + 1) / 2w) over coords = [(u_i, v_i)],
    a_i proportional to 1.04^-i.  The unnormalised DCT-II of a basis function with a zero frequency is twice (u or v zero) the
    one with none, so a_i is halved there: the coefficients, not the pixel amplitudes, descend by 1.04, and the list comes back
    in planted order.  The a_i are scaled to sum to 0.45; signs s_i from `seed`."""
    coords = [(int(u), int(v)) for u, v in coords]
    if len(set(coords)) != len(coords):
        raise ValueError("planted_frame: duplicate coordinate")
    for u, v in coords:
        if not (0 <= u < h and 0 <= v < w):
            raise ValueError(f"planted_frame: ({u}, {v}) outside {w}x{h}")
        if u == 0 and v == 0:
            raise ValueError("planted_frame: the DC term cannot be planted (the index list skips it)")
    a = np.array([DECAY ** -i / ((2.0 if u == 0 else 1.0) * (2.0 if v == 0 else 1.0)) for i, (u, v) in enumerate(coords)])
    a *= AMPLITUDE_SUM / a.sum()
    a *= np.random.default_rng(seed).choice([-1.0, 1.0], len(coords))
    y, x = np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64)
    grey = np.full((h, w), 0.5)
    for (u, v), ai in zip(coords, a):
        grey += ai * np.outer(np.cos(np.pi * u * (2 * y + 1) / (2 * h)), np.cos(np.pi * v * (2 * x + 1) / (2 * w)))
    return np.repeat(grey.astype(np.float32)[:, :, None], 3, axis=2)


SHAPES = [(96, 40), (40, 96), (64, 64)]        # (w, h): rows first, columns first, the tie w >= h
R_VALUES = [1, 15, 16, 17, 32, 33, "lb"]


def _coords_for(w, h, R, rng):
    """(u, v) pairs on exactly R first-pass lines, in list (amplitude) order."""
    lb, la = first_pass_lines(w, h)
    if R == 1:
        # all 40 entries in one slot, on the last line: positions 0, la - 1 and 38 others, shuffled
        pos = np.concatenate([[0, la - 1], rng.choice(np.arange(1, la - 1), 38, replace=False)])
        entries = [(lb - 1, int(p)) for p in rng.permutation(pos)]
    else:
        lines = np.concatenate([[0, lb - 1], rng.choice(np.arange(1, lb - 1), R - 2, replace=False)])
        shared = [int(p) for p in rng.choice(np.arange(1, la - 1), 3, replace=False)]     # positions several lines share
        entries = []
        for j, line in enumerate(int(l) for l in lines):
            n_here = 3 if j % 5 == 2 else 2
            want = {la - 1 if line == 0 else 0 if j % 4 == 1 else shared[j % 3]}          # line 0 cannot take position 0 (DC)
            if line == lb - 1:
                want = {0, la - 1}
            free = [p for p in range(1, la - 1) if p not in want]
            want |= {int(p) for p in rng.choice(free, n_here - len(want), replace=False)} if n_here > len(want) else set()
            entries += [(line, p) for p in want]
        # list order: shuffled over lines and positions, so a slot's entries are neither adjacent nor in position order
        entries = [entries[i] for i in rng.permutation(len(entries))]
    return [(l, p) if w >= h else (p, l) for l, p in entries]


def line_plan_cases():
    """{name: (w, h, coords)}: for each shape R in {1, 15, 16, 17, 32, 33, lb} distinct first-pass lines.  R = 1: 40 entries on
    the last line.  Otherwise two or three entries per line in shuffled list order; every case has line 0, the last line,
    position 0 and the last position, and positions shared by several lines."""
    cases = {}
    for w, h in SHAPES:
        lb, _ = first_pass_lines(w, h)
        for R in R_VALUES:
            r = lb if R == "lb" else R
            rng = np.random.default_rng(1000 * w + 10 * h + r)
            cases[f"{w}x{h}-R{R}"] = (w, h, _coords_for(w, h, r, rng))
    return cases


def case_seed(name):
    """The sign seed of a case's frame: fixed per name, so the CPU check and the GPU run see the same frame."""
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def case_frame(name):
    w, h, coords = line_plan_cases()[name]
    return planted_frame(w, h, coords, case_seed(name))


def named_R(name, w, h):
    r = name.rsplit("-R", 1)[1]
    return first_pass_lines(w, h)[0] if r == "lb" else int(r)
