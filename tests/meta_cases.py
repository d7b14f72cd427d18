"""Generators and predicates of the metamorphic tests (tests/test_meta_cpu.py, tests/test_meta_gpu.py): frames scaled by
powers of two, frames and marks poisoned with non-finite values, flat integer frames, and the table of shapes with the kernel
family each one is there for.  numpy only: the CPU file pins the oracle's side of every property on exactly these inputs
before the GPU file holds the library to it."""
import numpy as np

# ---- shapes -----------------------------------------------------------------------------------------------------------------
# n frames in chunks of `chunk` (ssw_ctx_set_chunk_frames): two full chunks and a ragged one, both lanes in use.  `plan`: the
# flags of ssw_ctx_transform_plan(chunk, w, h) that make the shape a test of its family; every GPU test asserts them.
# `poison_at`: first frame, last frame of a chunk, ragged tail.
# The pruned derived transform runs only where the compact plane is at most a quarter of the frame's width (4 * ceil32(8 sqrt k)
# <= w): P has k = 200 (128 columns of 512); L2 is 1280 wide, as in tests/test_config_matrix_gpu.py, because a 512-wide frame
# reaches neither the fused derived kernel (k = 600: 224 columns) nor the gathered launches (k = 1056: 288 columns).
# F is the smallest fused case of tests/test_base_prune_gpu.py (384 x 256, k = 64).  The planner takes the fused forward
# transform from 28 frames per pass on, and batch extract prunes the base frames only when every chunk of the call takes it:
# F alone has 86 frames in chunks of 29 (29 + 29 + a ragged 28) where the other shapes have 9 in chunks of 4.
SHAPES = {
    "D": dict(w=100, h=75, n=9, chunk=4, k=150, tuning=None, poison_at=(0, 3, 8),
              plan={"pair_f64": False}),
    "P": dict(w=512, h=288, n=9, chunk=4, k=200, tuning=None, poison_at=(0, 3, 8),
              plan={"pair_f64": True, "rows_deep": True, "cols_deep": True, "rows_level2": False, "cols_level2": False,
                    "class_major": True, "fused_cols": False}),
    "L2": dict(w=1280, h=288, n=9, chunk=4, k=600, tuning="LEVEL2", poison_at=(0, 3, 8),
               plan={"pair_f64": True, "rows_deep": True, "cols_deep": True, "rows_level2": True, "cols_level2": True,
                     "class_major": True, "fused_cols": False}),
    "F": dict(w=384, h=256, n=86, chunk=29, k=64, tuning="FUSED", poison_at=(0, 28, 85),
              plan={"pair_f64": True, "rows_level2": True, "cols_level2": True, "class_major": True, "fused_cols": True}),
    "T": dict(w=272, h=512, n=9, chunk=4, k=300, tuning=None, poison_at=(0, 3, 8),
              plan={"pair_f64": True, "rows_deep": False, "cols_deep": True, "rows_level2": False, "cols_level2": False,
                    "class_major": False, "fused_cols": False}),
}
K_GATHERED = 1056          # L2: the pruned derived row pass as gathered launches (k = 600: one fused kernel)
# History: narrower than P in the same workspaces.  n * 432 lines per column pass are no multiple of the 128-line GEMM tile
# for the chunk sizes used (4, 29); its column pass is deep and takes the staged pre-pass (the level-2 one under the LEVEL2 and
# FUSED tunings), whose planes end in zero padding -- 34 units in rows of kpad(68) = 40 doubles -- that lies where P's planes
# held data; its row operands are padded too (kpad(216) = 112 doubles for 108 terms).  `plan`: per tuning.
NARROW = dict(w=432, h=272, k=300,
              plan={None: {"pair_f64": True, "rows_deep": False, "cols_deep": True, "cols_level2": False, "class_major": False},
                    "LEVEL2": {"pair_f64": True, "rows_deep": False, "cols_deep": True, "cols_level2": True, "class_major": False},
                    "FUSED": {"pair_f64": True, "rows_deep": False, "cols_deep": True, "cols_level2": True, "class_major": False}})

# The same width at a semi-deep height: 264 = 8 * 33 rows (h % 16 == 8, h >= deep_min_cols) take the staged semi-deep column
# pre-pass under every tuning (semi-deep has no level 2).  Its M plane holds H/4 = 66 terms in rows of kpad(H/2) = 72 doubles,
# and no data store reaches [66, 72): only the pre-pass's zero fill does.  The plan flags cannot show semi-deep (it does not
# count as deep), so the GPU test pins it by cols_deep == False and this arithmetic.
NARROW_SEMI = dict(w=432, h=264, k=300,
                   plan={t: {"pair_f64": True, "rows_deep": False, "cols_deep": False, "cols_level2": False, "class_major": False}
                         for t in (None, "LEVEL2", "FUSED")})


def kpad(n):
    """Row stride, in doubles, of an operand plane of a length-n axis (csrc/dct_pair_common.hpp: pair_kpad)."""
    return max(16, (n // 2 + 7) // 8 * 8)


# ---- clean batches ----------------------------------------------------------------------------------------------------------
def smooth(n, h, w, seed):
    """The smooth frames of the base-prune tests (tests/test_base_select_gpu.py: 240 cosines of horizontal and vertical
    frequency below 24, all inside column tile 0, + noise of 1e-4)."""
    rng = np.random.default_rng(seed)
    cy = np.cos(np.pi * (2 * np.arange(h)[:, None] + 1) * np.arange(24)[None, :] / (2 * h))
    cx = np.cos(np.pi * (2 * np.arange(w)[:, None] + 1) * np.arange(24)[None, :] / (2 * w))
    out = np.empty((n, h, w, 3), np.float32)
    for f in range(n):
        amp = np.zeros((24, 24))
        for _ in range(240):
            fx, fy = rng.integers(0, 24), rng.integers(0, 24)
            amp[fy, fx] += rng.uniform(0.2, 1.0) / (1 + fx + fy)
        a = cy @ amp @ cx.T
        a = 0.5 + 0.35 * a / np.abs(a).max()
        for c in range(3):
            out[f, :, :, c] = a + 1e-4 * rng.standard_normal((h, w))
    return np.clip(out, 0.0, 1.0).astype(np.float32)


def with_cosine(frames, col, amp=0.1):
    """+ one strong horizontal cosine of frequency `col` (and vertical frequency 3)."""
    n, h, w, _ = frames.shape
    y, x = np.mgrid[0:h, 0:w]
    c = amp * np.cos(np.pi * (2 * x + 1) * col / (2 * w)) * np.cos(np.pi * (2 * y + 1) * 3 / (2 * h))
    return np.clip(frames + c[None, :, :, None], 0.0, 1.0).astype(np.float32)


def frames_of(name, synth_frame, n=None):
    """The clean batch of a shape: `synth_frame(seed, frame, w, h)` (the oracle's generator), except F, which takes smooth
    frames -- every second one with a strong cosine in the last column tile, so that the frames of a batch have different
    base-prune thresholds and need different tiles."""
    s = SHAPES[name]
    n = s["n"] if n is None else n
    if name == "F":
        a = smooth(n, s["h"], s["w"], 11)
        a[1::2] = with_cosine(a[1::2], 128 * 2 + 5)
        return a
    return np.stack([synth_frame(7, i, s["w"], s["h"]) for i in range(n)])


def marks_of(name, k=None, n=None):
    s = SHAPES[name]
    return np.random.default_rng(s["w"] + (k or s["k"])).standard_normal((n or s["n"], k or s["k"])).astype(np.float32)


# ---- exact scaling ----------------------------------------------------------------------------------------------------------
# f32 keeps 2^e * x exact while neither side leaves the normal range.  Coefficients of frames in [0, 1] lie between about 1e-8
# and 1e3, their energy keys between 1e-16 and 1e6: at e = +-40 the first k keys (>= 1e-8 * 2^-80 ~ 1e-32 at worst, far more
# in practice) stay normal, at e = +60 keys of 1e3^2 * 2^120 overflow to +inf and the index list changes.
EXPONENTS = (-40, -12, 12, 40)
OVERFLOW_EXPONENT = 60
CYCLE = (0, -40, 12, -12, 40)          # frame i of a batch is scaled by 2^CYCLE[i % 5]: neighbours up to 80 binades apart


def cycle_exps(n):
    return [CYCLE[i % len(CYCLE)] for i in range(n)]


def pow2(e):
    return np.float32(2.0 ** int(e))


def scaled(frames, exps):
    """frames [n, ...] f32 -> frame i multiplied by np.float32(2.0 ** exps[i]) (exact in f32 for the exponents above)."""
    a = np.array(frames, np.float32, copy=True)
    assert a.shape[0] == len(exps)
    for i, e in enumerate(exps):
        a[i] *= pow2(e)
    return a


# ---- poison -----------------------------------------------------------------------------------------------------------------
FRAME_POISONS = ("nan_last", "inf_first", "ninf_middle", "all_nan", "all_3e38")         # kinds (a) .. (e)
ALL_NAN_PLANE = FRAME_POISONS[:4]      # the kinds whose coefficient plane the oracle fixes: every coefficient NaN (test_meta_cpu.py)
MARK_POISONS = ("nan", "inf", "ninf", "3e38")
BIG = np.float32(3e38)                 # finite; any sum of two of them rounds to +inf in f32
_MARK_VALUE = {"nan": np.float32(np.nan), "inf": np.float32(np.inf), "ninf": np.float32(-np.inf), "3e38": BIG}


def poison(frame, kind):
    """A copy of one f32 frame [h, w, 3] with
    nan_last     one NaN in the last channel of the last pixel
    inf_first    one +Inf in channel 0 of pixel (0, 0)
    ninf_middle  one -Inf in channel 1 of pixel (h // 2, w // 2)
    all_nan      every value NaN
    all_3e38     every value 3e38."""
    a = np.array(frame, np.float32, copy=True)
    h, w, _ = a.shape
    if kind == "nan_last":
        a[h - 1, w - 1, 2] = np.nan
    elif kind == "inf_first":
        a[0, 0, 0] = np.inf
    elif kind == "ninf_middle":
        a[h // 2, w // 2, 1] = -np.inf
    elif kind == "all_nan":
        a[...] = np.nan
    elif kind == "all_3e38":
        a[...] = BIG
    else:
        raise ValueError(kind)
    return a


def poison_sites(frame_shape, kind):
    """Boolean mask [h, w, 3] of the values `poison` replaces."""
    h, w, _ = frame_shape
    m = np.zeros(frame_shape, bool)
    if kind == "nan_last":
        m[h - 1, w - 1, 2] = True
    elif kind == "inf_first":
        m[0, 0, 0] = True
    elif kind == "ninf_middle":
        m[h // 2, w // 2, 1] = True
    elif kind in ("all_nan", "all_3e38"):
        m[...] = True
    else:
        raise ValueError(kind)
    return m


def poison_batch(frames, j, kind):
    a = np.array(frames, np.float32, copy=True)
    a[j] = poison(a[j], kind)
    return a


def mark_sites(k):
    return (0, k // 2, k - 1)


def poison_mark(mark, kind):
    """A copy of one mark [k] with the first, the middle and the last entry replaced by NaN, +Inf, -Inf or 3e38."""
    m = np.array(mark, np.float32, copy=True)
    m[list(mark_sites(m.size))] = _MARK_VALUE[kind]
    return m


def poison_marks(marks, j, kind):
    m = np.array(marks, np.float32, copy=True)
    m[j] = poison_mark(m[j], kind)
    return m


FLAT_FRAMES = ((np.uint8, 0), (np.uint8, 255), (np.uint16, 65535))


def flat(h, w, dtype, value):
    """A flat integer frame: every AC coefficient is zero, and Option 2 extraction from it is 0 / 0."""
    return np.full((h, w, 3), value, dtype)


def flat_batch(frames, j, value):
    a = np.array(frames, copy=True)
    a[j] = value
    return a


# ---- predicates -------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def others_same(clean, got, j):
    """Every frame i != j of `got` [n, ...] is byte-identical to `clean`'s.  Returns the list of frames that differ."""
    assert clean.shape == got.shape and clean.dtype == got.dtype
    return [i for i in range(clean.shape[0]) if i != j and clean[i].tobytes() != got[i].tobytes()]


def same_nan_mask(a, b):
    """Poisoned outputs: NaN payloads are not fixed, so only the positions of the NaNs are compared -- and the rest as bytes."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()
