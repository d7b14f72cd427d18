"""Identifying a suspect's original (ssw_signature_rgb8, ssw_signature_match): the parts that need no GPU -- the numpy
restatement of the definition in include/ssw.h (the yardstick of tests/test_identify_gpu.py, which imports it from here), the
grid's values worked by hand, what the signature tells apart on the reference's photograph, the catalogue file and the CLI's
`index` / `identify` / `trace --catalogue` arguments."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli, storage

NONE = 0xFFFFFFFF


# ---- the definition of include/ssw.h, restated ------------------------------------------------------------------------------
def luma(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def signature_ref(frame):
    """Frame [h][w][3 or 4] u8 -> uint8 [1024]: sig[j][i] = (sum of L over cell (i, j) + n / 2) / n, alpha ignored."""
    h, w = frame.shape[:2]
    assert w >= 32 and h >= 32 and frame.shape[2] in (3, 4)
    lum = luma(frame)
    sig = np.zeros((32, 32), np.uint8)
    for j in range(32):
        y0, y1 = j * h // 32, (j + 1) * h // 32
        for i in range(32):
            x0, x1 = i * w // 32, (i + 1) * w // 32
            n = (x1 - x0) * (y1 - y0)
            sig[j, i] = (int(lum[y0:y1, x0:x1].sum()) + n // 2) // n
    return sig.reshape(1024)


def distance_ref(a, b):
    """D(a, b) = sum |a[t] - b[t]|; a [..., 1024], b [..., 1024] broadcast."""
    return np.abs(a.astype(np.int64) - b.astype(np.int64)).sum(-1)


def all_distances_ref(query, catalogue):
    """[nq][nc] int64.  |a - b| of bytes as max - min stays in uint8, which keeps large catalogues quick; the same sums."""
    query, catalogue = np.asarray(query, np.uint8).reshape(-1, 1024), np.asarray(catalogue, np.uint8).reshape(-1, 1024)
    out = np.zeros((query.shape[0], catalogue.shape[0]), np.int64)
    for q in range(query.shape[0]):
        for c0 in range(0, catalogue.shape[0], 8192):
            c = catalogue[c0:c0 + 8192]
            out[q, c0:c0 + 8192] = (np.maximum(c, query[q]) - np.minimum(c, query[q])).sum(-1, dtype=np.int64)
    return out


def match_ref(query, catalogue, top, dist=None):
    """-> (index [nq][top], distance [nq][top]) u32: the `top` smallest (D, index), the rest 0xFFFFFFFF."""
    d = all_distances_ref(query, catalogue) if dist is None else dist
    nq, nc = d.shape
    idx, dst = np.full((nq, top), NONE, np.uint32), np.full((nq, top), NONE, np.uint32)
    for q in range(nq):
        order = np.lexsort((np.arange(nc), d[q]))[:top]
        idx[q, :len(order)], dst[q, :len(order)] = order, d[q][order]
    return idx, dst


def test_restatement_agrees_with_itself():
    rng = np.random.default_rng(0)
    q, c = rng.integers(0, 256, (3, 1024), dtype=np.uint8), rng.integers(0, 256, (11, 1024), dtype=np.uint8)
    assert np.array_equal(all_distances_ref(q, c), distance_ref(q[:, None], c[None]))
    assert int(distance_ref(np.zeros(1024, np.uint8), np.full(1024, 255, np.uint8))) == 261120
    c[7] = c[2]
    idx, dst = match_ref(c[2:3], c, 3)
    assert list(idx[0][:2]) == [2, 7] and list(dst[0][:2]) == [0, 0]             # ties: the lower index first
    idx, dst = match_ref(q, c[:2], 8)
    assert (idx[:, 2:] == NONE).all() and (dst[:, 2:] == NONE).all() and (idx[:, :2] != NONE).all()


# ---- grid values by hand ------------------------------------------------------------------------------------------------------
def test_grid_32x32_is_the_luma():
    f = np.random.default_rng(1).integers(0, 256, (32, 32, 3), dtype=np.uint8)
    assert np.array_equal(signature_ref(f).reshape(32, 32), luma(f))


def test_grid_33x35_by_hand():
    """w = 33: floor(i 33 / 32) = i for i < 32 and 33 for i = 32 -- the last grid column is 2 pixels wide.  h = 35:
    floor(j 35 / 32) steps by 2 after j = 10, 21 and 31 -- those grid rows are 2 pixels high."""
    h, w = 35, 33
    rows = [(j * h // 32, (j + 1) * h // 32) for j in range(32)]
    assert [j for j, (a, b) in enumerate(rows) if b - a == 2] == [10, 21, 31] and all(b - a in (1, 2) for a, b in rows)
    cols = [(i * w // 32, (i + 1) * w // 32) for i in range(32)]
    assert [i for i, (a, b) in enumerate(cols) if b - a == 2] == [31]
    # grey pixels (R = G = B = v: luma (256 v + 128) >> 8 = v), so the sums can be done by hand
    v = np.zeros((h, w), np.int64)
    v[10, 0], v[11, 0] = 10, 13              # cell (0, 10): 2 px, sum 23 -> (23 + 1) / 2 = 12  (11.5 rounds up)
    v[0, 31], v[0, 32] = 7, 8                # cell (31, 0): 2 px, sum 15 -> (15 + 1) / 2 = 8
    v[22, 31], v[22, 32], v[23, 31], v[23, 32] = 1, 2, 3, 3   # cell (31, 21): 4 px, sum 9 -> (9 + 2) / 4 = 2  (2.25 rounds down)
    v[33, 31], v[33, 32], v[34, 31], v[34, 32] = 250, 251, 252, 253   # cell (31, 31): sum 1006 -> (1006 + 2) / 4 = 252
    v[5, 5] = 200                            # a one-pixel cell is the pixel
    f = np.repeat(v[:, :, None], 3, 2).astype(np.uint8)
    sig = signature_ref(f).reshape(32, 32)
    assert (sig[10, 0], sig[0, 31], sig[21, 31], sig[31, 31], sig[5, 5]) == (12, 8, 2, 252, 200)
    assert sig.sum() == 12 + 8 + 2 + 252 + 200
    # an alpha channel does not matter
    a = np.concatenate([f, np.random.default_rng(2).integers(0, 256, (h, w, 1), dtype=np.uint8)], 2)
    assert np.array_equal(signature_ref(a), signature_ref(f))


# ---- what it tells apart, on the reference's photograph ---------------------------------------------------------------------------
def cat():
    g = np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))
    return g["cat"], g["watermarked_with_1"]


CATALOGUE_NAMES = ["cat", "mirror", "flip", "turn180", "roll40", "roll160", "negative", "noise", "grey"]
QUERY_SIZES = [None, (320, 222), (213, 149), (960, 666), (64, 44), (500, 444)]


def cat_catalogue(base):
    noise = np.random.default_rng(11).integers(0, 256, base.shape, dtype=np.uint8)
    return [base, base[:, ::-1], base[::-1], base[::-1, ::-1], np.roll(base, 40, 1), np.roll(base, 160, 1), 255 - base, noise,
            np.full_like(base, 128)]


def test_whole_frame_copies_are_told_apart_and_cut_outs_are_not():
    base, marked = cat()
    sigs = np.stack([signature_ref(np.ascontiguousarray(f)) for f in cat_catalogue(base)])
    worst = None
    for size in QUERY_SIZES:
        q = marked if size is None else O.resize_rgb8(marked, *size)
        idx, dst = match_ref(signature_ref(q)[None], sigs, 2)
        print("query", size or "as is", "best", CATALOGUE_NAMES[idx[0, 0]], int(dst[0, 0]), "runner-up", CATALOGUE_NAMES[idx[0, 1]], int(dst[0, 1]))
        assert idx[0, 0] == 0, size                                    # the cat
        assert dst[0, 1] >= 2 * dst[0, 0], (size, dst)                 # the condition: the runner-up is at least twice as far
        assert dst[0, 0] <= api.IDENTIFY_MAX_DISTANCE < dst[0, 1], (size, dst)
        worst = max(worst or 0, int(dst[0, 0]))
    # the documented limit: a cut-out is as far from its original as an unrelated picture
    cut = np.ascontiguousarray(marked[20:424, 30:610])
    assert cut.shape[:2] == (404, 580)
    d = int(distance_ref(signature_ref(cut), sigs[0]))
    print("580x404 cut-out against its original", d, "largest whole-frame distance", worst)
    assert d > api.IDENTIFY_MAX_DISTANCE


# ---- the catalogue file ----------------------------------------------------------------------------------------------------------
def test_catalogue_save_load_round_trip(tmp_path):
    base, marked = cat()
    frames = [base, np.ascontiguousarray(base[:, ::-1]), O.resize_rgb8(marked, 320, 222)]
    c = api.Catalogue()
    c.add_signatures(["cat.jpg", 'mir"ror.png', "späße/half.png"], [signature_ref(f) for f in frames], [(f.shape[1], f.shape[0]) for f in frames],
                     ["cat_fp.json", None, ""])
    assert len(c) == 3 and c.marks_files == ["cat_fp.json", None, None]
    path = str(tmp_path / "catalogue.npz")
    c.save(path)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["marks_files", "names", "signatures", "sizes", "version"]
        assert z["signatures"].dtype == np.uint8 and z["signatures"].shape == (3, 1024)
        assert z["sizes"].dtype == np.uint32 and z["sizes"].tolist() == [[640, 444], [640, 444], [320, 222]] and int(z["version"]) == 1
    d = api.Catalogue.load(path)
    assert len(d) == 3 and d.names == c.names and d.marks_files == c.marks_files
    assert np.array_equal(d.signatures, c.signatures) and np.array_equal(d.sizes, c.sizes)
    # appending after a load, and an empty catalogue
    d.add_signatures(["grey"], [signature_ref(np.full((40, 50, 3), 9, np.uint8))], [(50, 40)])
    d.save(path)
    e = api.Catalogue.load(path)
    assert len(e) == 4 and e.names[3] == "grey" and (e.signatures[3] == 9).all() and e.sizes[3].tolist() == [50, 40]
    empty = str(tmp_path / "empty.npz")
    api.Catalogue().save(empty)
    assert len(api.Catalogue.load(empty)) == 0
    with pytest.raises(ValueError):
        c.add_signatures(["a", "b"], [signature_ref(base)], [(640, 444)])
    np.savez(str(tmp_path / "other.npz"), x=np.zeros(3))
    with pytest.raises(ValueError):
        storage.load_catalogue(str(tmp_path / "other.npz"))


def test_abi_constants_and_header():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    assert [f[0] for f in L.ImageShape._fields_] == ["w", "h", "channels"]
    assert "typedef struct ssw_image_shape { uint32_t w, h, channels; } ssw_image_shape;" in text
    for name in ("ssw_signature_rgb8", "ssw_signature_host_rgb8", "ssw_signature_match"):
        assert name in L.SIGNATURES and name + "(" in text
    decl = text.index("ssw_signature_rgb8(")
    section = text[text.rfind("identifying a suspect's original", 0, decl):decl]
    assert "examples/main.rs:369-415" in section and "Reader::base" in section and "SSW_STAGE_LOCATE" in section
    assert (L.SIGNATURE_BYTES, L.MATCH_NONE, L.MATCH_TOP_MAX) == (1024, NONE, 8) and api.IDENTIFY_MAX_DISTANCE == 8192
    src = open(os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc", "catalogue.hip")).read()
    assert f"MT_C = {L.MATCH_TILE};" in src and f"MATCH_CHUNK = {L.MATCH_CHUNK};" in src and f"MT_Q = {L.MATCH_QUERY_TILE};" in src


# ---- the CLI's arguments --------------------------------------------------------------------------------------------------------
def test_index_and_identify_arguments():
    p = cli.build_parser()
    a = p.parse_args(["index", "a.png", "b.jpg", "-o", "originals.npz"])
    assert (a.command, a.files, a.output, a.marks) == ("index", ["a.png", "b.jpg"], "originals.npz", None)
    a = p.parse_args(["index", "a.png", "--output", "o.npz", "--marks", "a_fp.json"])
    assert a.marks == ["a_fp.json"]
    a = p.parse_args(["identify", "x.png", "y.png", "--catalogue", "o.npz"])
    assert (a.command, a.suspects, a.catalogue, a.top, a.max_distance) == ("identify", ["x.png", "y.png"], "o.npz", 1, 8192)
    a = p.parse_args(["identify", "x.png", "--catalogue", "o.npz", "--top", "3", "--max-distance", "5000"])
    assert (a.top, a.max_distance) == (3, 5000)
    for bad in (["index", "a.png"], ["index", "-o", "o.npz"], ["identify", "x.png"], ["identify", "--catalogue", "o.npz"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_index_default_marks_file_and_record_text(tmp_path):
    img = tmp_path / "photo.jpg"
    img.write_bytes(b"")
    assert cli.default_marks_file(str(img)) is None
    (tmp_path / "photo_fp.json").write_text("{}")
    assert cli.default_marks_file(str(img)) == str(tmp_path / "photo_fp.json")
    hit = api.Identified("photo.jpg", "photo.jpg", 2951, (3840, 2160), None, 0, [])
    miss = api.Identified(None, "photo.jpg", 15640, (3840, 2160), None, 0, [])
    assert cli.original_text(hit) == '"photo.jpg" 3840x2160 (distance 2951)'
    assert cli.original_text(miss) == 'none (nearest "photo.jpg", distance 15640)'


def test_trace_demands_its_original_without_a_catalogue(capsys):
    p = cli.build_parser()
    with pytest.raises(SystemExit) as e:
        p.parse_args(["trace", "--suspects", "a.png", "--marks", "m.json"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "trace: error: the following arguments are required: base" in err
    with pytest.raises(SystemExit):
        p.parse_args(["trace", "base.png", "--suspects", "a.png"])
    assert "the following arguments are required: --marks" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(["trace", "base.png", "--marks", "m.json"])
    assert "the following arguments are required: --suspects" in capsys.readouterr().err
    # as before with the original; with a catalogue the original (and the marks) may be left out, not given twice
    a = p.parse_args(["trace", "base.png", "--suspects", "a.png", "--marks", "m.json"])
    assert (a.base, a.suspects, a.marks, a.catalogue) == ("base.png", ["a.png"], ["m.json"], None)
    a = p.parse_args(["trace", "--catalogue", "o.npz", "--suspects", "a.png", "b.png", "--locate", "b.png"])
    assert (a.base, a.marks, a.catalogue, a.max_distance) == (None, None, "o.npz", 8192) and list(a.locates) == ["b.png"]
    with pytest.raises(SystemExit):
        p.parse_args(["trace", "base.png", "--catalogue", "o.npz", "--suspects", "a.png"])
    with pytest.raises(SystemExit):
        p.parse_args(["trace", "--catalogue", "o.npz"])
