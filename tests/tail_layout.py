"""The tail layout of a pruned base reader's row pass, restated in plain Python from csrc/dct_pair_class.hip
(pair_class_args), csrc/base_energy.hip (launch_base_energy_bound) and the gate of the tail row launches
(dct_pair_f64_kernel.hpp, SUB == 5).  tests/test_tail_layout_cpu.py binds it to the code on the host
(tests/cpp/tail_layout_test.cpp); the GPU tests take every expected counter from here, never from the library.

A row of W columns is P = W / 16 pairs in each of the eight level-2 classes; a launch covers them in tile columns of 64 pairs
(48 where 64-pair tiles would end in a tile of at most 16 pairs and 48-pair ones need no more tiles).  Tile column 0 is the
head (exact energy launches); the others are the tail: the bound kernel covers their pairs in MFMA tiles of 16 pairs, 11 per
block (more: a second chunk), and their exact launches run gated per (frame, class, tile column) -- a job.  Entry e of a class
lies in column tile e >> 3 (128 frequencies / 16 slots); the first output of pair p is entry p, the second one too, except in
the five classes of E's shape, where it is entry p - 1 (and pair 0's slot carries entry P - 1).  So tile column tn of such a
class also writes one entry of the column tile below its first own one: the seam tile."""
from collections import namedtuple

import numpy as np

# kLevel2Classes, in launch order, and which of them have class E's shape (e2off = 1)
CLASSES = ("R1+ R1-", "R2 rotated", "AS2 BD2", "AD2 BS2", "AS+ BD-", "AS- BD+", 'O rotated "-"', 'O rotated "+"')
E_SHAPED = (0, 1, 1, 0, 1, 0, 1, 1)
GSH = 3                                # 128 / 16 = 8 entries of a class per column tile
BE_NJ = 11                             # MFMA pair tiles per block of the bound kernel

TailLayout = namedtuple("TailLayout", "w tile48 pairs tw tile_cols pair0 tail_pairs mfma_tiles chunks kp ksteps column_tiles bn32 split_bytes")


def tail_layout(w, tile48):
    p = w // 16
    tiles_n, tw = (p + 63) // 64, 64
    if tile48 and p > 64 and p % 64 != 0 and p % 64 <= 16 and (p + 47) // 48 == tiles_n:
        tw, tiles_n = 48, (p + 47) // 48
    kp = max(16, (p + 7) // 8 * 8)
    mfma = (p - tw + 15) // 16 if p > tw else 0
    ksteps = (kp // 8 + 3) // 4
    return TailLayout(w, tile48, p, tw, tuple(min(tw, p - tw * t) for t in range(tiles_n)), tw, p - tw, mfma, (mfma + BE_NJ - 1) // BE_NJ, kp, ksteps,
                      w // 128, 2 if tw == 48 else 0, ksteps * 4 * mfma * 1024 + 16)


def feeds(lay, cls, tn):
    """(lo, hi): the column tiles that tile column tn >= 1 of class cls writes, as the gate computes them."""
    pf = tn * lay.tw
    pl = min(pf + lay.tw - 1, lay.pairs - 1)
    return (pf - E_SHAPED[cls]) >> GSH, pl >> GSH


def jobs(lay, needed):
    """The (class, tile column) jobs that must run for a frame whose needed column tiles are `needed`."""
    needed = set(needed)
    return [(c, tn) for tn in range(1, len(lay.tile_cols)) for c in range(8)
            if any(t in needed for t in range(feeds(lay, c, tn)[0], feeds(lay, c, tn)[1] + 1))]


def seam_tiles(lay):
    """The last column tile that tile column tn - 1 feeds, for tn = 1 ..: tile column tn feeds it too, with one entry."""
    return [tn * lay.tw // 8 - 1 for tn in range(1, len(lay.tile_cols))]


def own_tiles(lay, tn):
    """The column tiles that only tile column tn >= 1 feeds (but for the head's one entry P - 1 in the last tile)."""
    mine = {t for c in range(8) for t in range(feeds(lay, c, tn)[0], feeds(lay, c, tn)[1] + 1)} - set(range(lay.tw >> GSH))
    for other in range(1, len(lay.tile_cols)):
        if other != tn:
            mine -= {t for c in range(8) for t in range(feeds(lay, c, other)[0], feeds(lay, c, other)[1] + 1)}
    return sorted(mine)


def head_width(lay):
    """Columns below it are fed by head pairs only: 128 x (first seam tile)."""
    return 128 * seam_tiles(lay)[0]


def smooth_like(n, h, w, seed):
    """test_base_prune_gpu.smooth (240 cosines of horizontal and vertical frequency below 24, 1 / (1 + fx + fy) amplitudes, noise
    of 1e-4) with the same random draws, the sum of cosines as one matrix product: a 4K-wide frame in milliseconds."""
    rng = np.random.default_rng(seed)
    cx = np.cos(np.pi * (2 * np.arange(w)[None, :] + 1) * np.arange(24)[:, None] / (2 * w))
    cy = np.cos(np.pi * (2 * np.arange(h)[None, :] + 1) * np.arange(24)[:, None] / (2 * h))
    out = np.empty((n, h, w, 3), np.float32)
    for f in range(n):
        amp = np.zeros((24, 24))
        for _ in range(240):
            fx, fy = rng.integers(0, 24), rng.integers(0, 24)
            amp[fy, fx] += rng.uniform(0.2, 1.0) / (1 + fx + fy)
        a = cy.T @ amp @ cx
        a = 0.5 + 0.35 * a / np.abs(a).max()
        for c in range(3):
            out[f, :, :, c] = a + 1e-4 * rng.standard_normal((h, w))
    return np.clip(out, 0.0, 1.0).astype(np.float32)
