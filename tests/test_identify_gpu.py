"""Identifying a suspect's original on the GPU (ssw_signature_rgb8, ssw_signature_host_rgb8, ssw_signature_match): signatures,
indices and distances must EQUAL the numpy restatement of the definition (tests/test_identify_cpu.py) -- everything is an
integer, there is no tolerance -- and `trace --catalogue` must name the recipient a direct trace on the named original names."""
import argparse
import ctypes as C
import io
import os

import numpy as np
import pytest

import gpu_util as G
import spread_spectrum_watermarking_amd as wm
from conftest import GOLDEN
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import cli
from spread_spectrum_watermarking_amd.storage import Configuration, DescribedWatermark, Version1Storage
from test_identify_cpu import NONE, all_distances_ref, match_ref, signature_ref

pytestmark = pytest.mark.gpu

# one more than a chunk and a tile: the last entry is alone in the second tile of the second launch
NC_CROSS = L.MATCH_CHUNK + L.MATCH_TILE + 1


def cat():
    g = np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))
    return g["cat"], g["watermarked_with_1"]


# ---- signatures -----------------------------------------------------------------------------------------------------------------
def mixed_frames():
    rng = np.random.default_rng(5)
    rnd = lambda w, h, c: rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    big = O.f32_to_u8(O.synth_frame(7, 0, 2048, 1100))                   # several blocks per row of cells
    return [rnd(32, 32, 3), rnd(33, 35, 3), rnd(35, 33, 4), rnd(97, 64, 3), cat()[0], rnd(1000, 37, 4), np.ascontiguousarray(big)]


_SIG = {}


def frames_and_refs():
    if not _SIG:
        _SIG["frames"] = mixed_frames()
        _SIG["refs"] = np.stack([signature_ref(f) for f in _SIG["frames"]])
    return _SIG["frames"], _SIG["refs"]


def device_signatures(frames, offsets):
    """ssw_signature_rgb8 on frames that lie `offsets[i]` bytes into their allocations."""
    lib, ctx = G.lib(), G.ctx()
    bufs = [ctx.alloc(f.nbytes + 3) for f in frames]
    ptrs = []
    for b, f, o in zip(bufs, frames, offsets):
        p = C.c_void_p(b.ptr.value + o)
        L.check(lib.ssw_copy_to_dev(ctx.handle, p, f.ctypes.data, f.nbytes), "ssw_copy_to_dev")
        ptrs.append(p.value)
    shapes = (L.ImageShape * len(frames))(*[L.ImageShape(f.shape[1], f.shape[0], f.shape[2]) for f in frames])
    out = ctx.alloc(len(frames) * 1024 + 3)
    sig_ptr = C.c_void_p(out.ptr.value + (offsets[0] % 4))
    L.check(lib.ssw_signature_rgb8(ctx.handle, (C.c_void_p * len(frames))(*ptrs), shapes, len(frames), sig_ptr), "ssw_signature_rgb8")
    got = np.empty((len(frames), 1024), np.uint8)
    L.check(lib.ssw_copy_to_host(ctx.handle, got.ctypes.data, sig_ptr, got.nbytes), "ssw_copy_to_host")
    for b in bufs + [out]:
        b.free()
    return got


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_signatures_of_mixed_shapes_in_one_call(shift):
    frames, refs = frames_and_refs()
    got = device_signatures(frames, [(i + shift) % 4 for i in range(len(frames))])
    for f, g, r in zip(frames, got, refs):
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, (f.shape, shift, bad[:8], g[bad[:8]], r[bad[:8]])


def test_alpha_does_not_matter_and_each_frame_alone_gives_the_same():
    frames, refs = frames_and_refs()
    rgba = frames[2].copy()
    rgba[..., 3] = 255 - rgba[..., 3]
    assert np.array_equal(device_signatures([rgba], [0])[0], refs[2])
    assert np.array_equal(device_signatures([np.ascontiguousarray(frames[2][..., :3])], [1])[0], refs[2])
    for i in (1, 6):
        assert np.array_equal(device_signatures([frames[i]], [0])[0], refs[i])
    many = [frames[i % 6] for i in range(70)]                              # more than one launch's 32 descriptors
    assert np.array_equal(device_signatures(many, [i % 4 for i in range(70)]), np.stack([refs[i % 6] for i in range(70)]))


def test_host_form_gives_the_same_bytes():
    frames, refs = frames_and_refs()
    assert np.array_equal(wm.signature(frames, ctx=G.ctx()), refs)
    assert wm.signature([], ctx=G.ctx()).shape == (0, 1024)


# ---- match ------------------------------------------------------------------------------------------------------------------------
def gpu_match(query, catalogue, top, want_all=True):
    lib, ctx = G.lib(), G.ctx()
    nq, nc = len(query), len(catalogue)
    dq = ctx.to_device(query) if nq else None
    dc = ctx.to_device(catalogue) if nc else None
    di, dd = ctx.alloc(max(nq * top, 1) * 4), ctx.alloc(max(nq * top, 1) * 4)
    da = ctx.alloc(max(nq * nc, 1) * 4) if want_all else None
    st = lib.ssw_signature_match(ctx.handle, dq.ptr if dq else None, nq, dc.ptr if dc else None, nc, top, di.ptr, dd.ptr, da.ptr if da else None)
    assert st == L.SSW_OK, st
    idx, dst = di.to_host(np.uint32, (nq, top)), dd.to_host(np.uint32, (nq, top))
    every = da.to_host(np.uint32, (nq, nc)) if want_all and nq * nc else None
    for b in (dq, dc, di, dd, da):
        if b is not None:
            b.free()
    return idx, dst, every


def planted(nq, nc, seed):
    """Random signatures with structure: near copies of the queries (a few bytes changed), exact copies and duplicates."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 1024), dtype=np.uint8)
    c = rng.integers(0, 256, (nc, 1024), dtype=np.uint8)
    for t in range(min(nc, 4 * nq + 8)):
        pos = int(rng.integers(0, nc))
        c[pos] = q[t % nq]
        flips = rng.integers(0, 1024, int(rng.integers(0, 40)))
        c[pos, flips] = rng.integers(0, 256, flips.size, dtype=np.uint8)
    if nc > 3:
        c[nc - 1] = c[nc // 2]
    return q, c


_REF = {}


def reference(nq, nc):
    if (nq, nc) not in _REF:
        q, c = planted(nq, nc, 100 * nq + nc % 97)
        _REF[nq, nc] = (q, c, all_distances_ref(q, c))
    return _REF[nq, nc]


@pytest.mark.parametrize("nc", [1, 7, 8, 9, 1000, NC_CROSS])
@pytest.mark.parametrize("nq", [1, 33])
def test_match_equals_the_restatement(nq, nc):
    q, c, dist = reference(nq, nc)
    for top in (1, 3, 8):
        ri, rd = match_ref(q, c, top, dist)
        idx, dst, every = gpu_match(q, c, top, want_all=top == 8)
        assert np.array_equal(idx, ri), (nq, nc, top, np.argwhere(idx != ri)[:4])
        assert np.array_equal(dst, rd), (nq, nc, top)
        if every is not None:
            assert np.array_equal(every, dist.astype(np.uint32)), (nq, nc)


def test_ties_across_blocks_and_chunks():
    nc = NC_CROSS
    rng = np.random.default_rng(9)
    c = rng.integers(0, 256, (nc, 1024), dtype=np.uint8)
    triple = rng.integers(0, 256, 1024, dtype=np.uint8)
    c[5] = c[600] = c[nc - 1] = triple                     # tiles 0 and 4 of the first launch, the last tile of the second
    q = np.stack([triple.copy(), triple.copy(), rng.integers(0, 256, 1024, dtype=np.uint8)])
    q[0, :7] ^= 1                                           # 7 away from the triple ...
    c[20000] = q[0]                                         # ... and an exact copy of itself further on
    c[3] = c[31000] = q[2]
    idx, dst, _ = gpu_match(q, c, 8, want_all=False)
    assert list(idx[0][:4]) == [20000, 5, 600, nc - 1] and list(dst[0][:4]) == [0, 7, 7, 7]
    assert list(idx[1][:4])[:3] == [5, 600, nc - 1] and list(dst[1][:4]) == [0, 0, 0, 7] and idx[1][3] == 20000
    assert list(idx[2][:2]) == [3, 31000] and list(dst[2][:2]) == [0, 0]
    ri, rd = match_ref(q, c, 8)
    assert np.array_equal(idx, ri) and np.array_equal(dst, rd)
    for top in (1, 3):
        i2, d2, _ = gpu_match(q, c, top, want_all=False)
        assert np.array_equal(i2, ri[:, :top]) and np.array_equal(d2, rd[:, :top])


def test_extremes_and_sentinels():
    zeros, ones = np.zeros((1, 1024), np.uint8), np.full((1, 1024), 255, np.uint8)
    idx, dst, every = gpu_match(zeros, ones, 1)
    assert idx.tolist() == [[0]] and dst.tolist() == [[261120]] and every.tolist() == [[261120]]
    q = np.random.default_rng(3).integers(0, 256, (5, 1024), dtype=np.uint8)
    idx, dst, _ = gpu_match(q, q[:0], 8, want_all=False)                   # nc == 0
    assert (idx == NONE).all() and (dst == NONE).all()
    idx, dst, _ = gpu_match(q, q[:3], 8, want_all=False)                   # nc < top
    ri, rd = match_ref(q, q[:3], 8)
    assert np.array_equal(idx, ri) and np.array_equal(dst, rd) and (idx[:, 3:] == NONE).all() and (dst[:, 3:] == NONE).all()
    assert [idx[i, 0] for i in range(3)] == [0, 1, 2] and (dst[:3, 0] == 0).all()


def test_status_codes():
    lib, ctx = G.lib(), G.ctx()
    f = np.zeros((40, 40, 3), np.uint8)
    d, sig = ctx.to_device(f), ctx.alloc(4 * 1024)
    ptr = (C.c_void_p * 1)(d.ptr.value)
    host = (C.c_void_p * 1)(f.ctypes.data)
    out = np.zeros((1, 1024), np.uint8)
    shape = lambda w, h, c: (L.ImageShape * 1)(L.ImageShape(w, h, c))
    for call in (lambda s, n: lib.ssw_signature_rgb8(ctx.handle, ptr, s, n, sig.ptr),
                 lambda s, n: lib.ssw_signature_host_rgb8(ctx.handle, host, s, n, out.ctypes.data)):
        assert call(shape(40, 40, 3), 1) == L.SSW_OK
        assert call(shape(31, 40, 3), 1) == L.SSW_ERR_BAD_ARG
        assert call(shape(40, 31, 3), 1) == L.SSW_ERR_BAD_ARG
        assert call(shape(40, 40, 2), 1) == L.SSW_ERR_BAD_ARG
        assert call(shape(40, 40, 5), 1) == L.SSW_ERR_BAD_ARG
        assert call(shape(31, 31, 7), 0) == L.SSW_OK                       # n == 0: nothing is looked at
        assert call(None, 1) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_signature_rgb8(None, ptr, shape(40, 40, 3), 1, sig.ptr) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_signature_rgb8(ctx.handle, ptr, shape(40, 40, 3), 1, None) == L.SSW_ERR_BAD_ARG
    idx, dst = ctx.alloc(64), ctx.alloc(64)
    match = lambda nq, nc, top, q=sig.ptr, c=sig.ptr: lib.ssw_signature_match(ctx.handle, q, nq, c, nc, top, idx.ptr, dst.ptr, None)
    assert match(1, 2, 1) == L.SSW_OK
    assert match(1, 2, 0) == L.SSW_ERR_BAD_ARG and match(1, 2, 9) == L.SSW_ERR_BAD_ARG
    assert match(1, 1 << 32, 1) == L.SSW_ERR_BAD_ARG
    assert match(0, 2, 9) == L.SSW_ERR_BAD_ARG and match(0, 2, 8) == L.SSW_OK
    assert match(1, 0, 8, c=None) == L.SSW_OK
    assert idx.to_host(np.uint32, (8,)).tolist() == [NONE] * 8 and dst.to_host(np.uint32, (8,)).tolist() == [NONE] * 8
    assert match(1, 2, 1, c=None) == L.SSW_ERR_BAD_ARG and match(1, 2, 1, q=None) == L.SSW_ERR_BAD_ARG
    for b in (d, sig, idx, dst):
        b.free()
    with pytest.raises(ValueError):
        wm.signature([np.zeros((31, 40, 3), np.uint8)], ctx=ctx)
    with pytest.raises(ValueError):
        wm.Catalogue(ctx).match_signatures(out, top=9)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
_E2E = {}


def end_to_end():
    """A catalogue of the cat and 15 synthetic pictures; three marked cats; one synthetic picture held back."""
    if not _E2E:
        ctx = G.ctx()
        base, _ = cat()
        synth = [np.ascontiguousarray(f) for f in O.f32_to_u8(G.synth(21, 0, 16, 640, 444))]
        marks = np.random.default_rng(21).standard_normal((3, 1000)).astype(np.float32)
        copies = wm.Writer(base, ctx=ctx).mark_copies_rgb8(list(marks))
        catalogue = wm.Catalogue(ctx)
        catalogue.add("cat", base)
        catalogue.add_many([f"synth{i}" for i in range(15)], synth[:15])
        _E2E.update(base=base, synth=synth, marks=marks, copies=copies, catalogue=catalogue,
                    suspects=[copies[1], O.resize_rgb8(np.ascontiguousarray(copies[2]), 320, 222), synth[15]])
    return _E2E


def test_identify_names_the_cat_and_refuses_the_stranger():
    e = end_to_end()
    catalogue = e["catalogue"]
    assert len(catalogue) == 16
    assert np.array_equal(catalogue.signatures, np.stack([signature_ref(f) for f in [e["base"]] + e["synth"][:15]]))
    found = wm.identify(catalogue, e["suspects"], top=3)
    for f in found:
        print(f.name, f.nearest, f.distance, f.candidates)
    assert [f.name for f in found] == ["cat", "cat", None]
    assert found[0].distance <= 8192 and found[1].distance <= 8192 and found[2].distance > 8192
    assert found[0].size == (640, 444) and found[0].index == 0 and len(found[0].candidates) == 3
    qs = np.stack([signature_ref(s) for s in e["suspects"]])
    ri, rd = match_ref(qs, catalogue.signatures, 3)
    assert [[c[1] for c in f.candidates] for f in found] == rd.tolist()
    assert [[c[0] for c in f.candidates] for f in found] == [[catalogue.names[i] for i in row] for row in ri]
    # a looser bound names the stranger's nearest entry: max_distance is the only thing that refuses it
    assert wm.identify(catalogue, e["suspects"][2:], max_distance=261120)[0].name == found[2].nearest


def test_two_match_calls_leave_no_residue():
    e = end_to_end()
    catalogue, sus = e["catalogue"], e["suspects"]
    a = catalogue.match(sus[:1], top=8)
    b = catalogue.match([e["synth"][3], sus[2], e["synth"][9]], top=2)
    c = catalogue.match(sus[:1], top=8)
    assert a == c and a[0][0][0] == "cat" and len(a[0]) == 8
    assert [r[0][0] for r in b] == ["synth3", wm.identify(catalogue, sus[2:])[0].nearest, "synth9"] and b[0][0][1] == 0 and b[2][0][1] == 0
    ri, rd = match_ref(np.stack([signature_ref(f) for f in [e["synth"][3], sus[2], e["synth"][9]]]), catalogue.signatures, 2)
    assert [[x[1] for x in r] for r in b] == rd.tolist() and [[x[0] for x in r] for r in b] == [[catalogue.names[i] for i in row] for row in ri]
    # an entry added between two calls is seen by the next one
    grown = wm.Catalogue(G.ctx())
    grown.add_signatures(catalogue.names, catalogue.signatures, catalogue.sizes)
    assert grown.match(sus[2:])[0][0][1] > 8192
    grown.add("held back", e["synth"][15])
    assert grown.match(sus[2:])[0][0] == ("held back", 0, (640, 444))


def test_cli_index_identify_and_trace_with_a_catalogue(tmp_path):
    from PIL import Image
    e = end_to_end()
    paths = {}
    for name, img in [("cat", e["base"])] + [(f"synth{i}", e["synth"][i]) for i in range(3)] + \
            [("leak_full", e["suspects"][0]), ("leak_half", e["suspects"][1]), ("stranger", e["suspects"][2])]:
        paths[name] = str(tmp_path / f"{name}.png")
        Image.fromarray(img).save(paths[name])
    with open(str(tmp_path / "cat_fp.json"), "w") as f:
        f.write(Version1Storage(Configuration(), [DescribedWatermark(m, f"buyer #{i}") for i, m in enumerate(e["marks"])]).to_json())
    npz = str(tmp_path / "originals.npz")
    out = io.StringIO()
    assert cli.cmd_index(argparse.Namespace(files=[paths["cat"], paths["synth0"]], output=npz, marks=None), out) == 0
    assert cli.cmd_index(argparse.Namespace(files=[paths["synth1"], paths["synth2"]], output=npz, marks=None), out) == 0      # appends
    loaded = wm.Catalogue.load(npz)
    assert loaded.names == [paths[n] for n in ("cat", "synth0", "synth1", "synth2")]
    assert loaded.marks_files == [str(tmp_path / "cat_fp.json"), None, None, None] and "4 originals" in out.getvalue()
    suspects = [paths["leak_full"], paths["stranger"], paths["leak_half"]]
    out = io.StringIO()
    assert cli.cmd_identify(argparse.Namespace(suspects=suspects, catalogue=npz, top=2, max_distance=8192), out) == 0
    rec = out.getvalue().split("-\n")[1:]
    print(out.getvalue())
    assert len(rec) == 3 and f'Original: "{paths["cat"]}" 640x444 (distance ' in rec[0] and rec[0].count("Next: ") == 1
    assert f'Original: none (nearest "' in rec[1] and f'Original: "{paths["cat"]}" 640x444' in rec[2]
    # trace --catalogue: the recipient and the similarity a direct trace on the named original gives
    args = cli.build_parser().parse_args(["trace", "--catalogue", npz, "--suspects", *suspects])
    out = io.StringIO()
    assert cli.cmd_trace(args, out) == 0
    print(out.getvalue())
    rec = out.getvalue().split("-\n")[1:]
    direct = wm.trace_many(e["base"], [e["suspects"][0], e["suspects"][1]], list(e["marks"]), ctx=G.ctx(), placements=[None, None])
    assert list(direct.best) == [1, 2]
    for r, s, who in ((rec[0], 0, 1), (rec[2], 1, 2)):
        lines = r.splitlines()
        assert lines[0] == f'  Suspect: "{suspects[0 if s == 0 else 2]}"' and lines[1].startswith(f'  Original: "{paths["cat"]}" 640x444 (distance ')
        assert "  Matches: true" in lines and f'  Description: "buyer #{who}"' in lines
        assert f"  Similarity: {cli._rust_f32(direct.best_sim[s])}" in lines, (lines, direct.best_sim)
    assert "Restored:" in rec[2] and "Restored:" not in rec[0]
    assert rec[1].splitlines()[0] == f'  Suspect: "{paths["stranger"]}"' and rec[1].splitlines()[1].startswith('  Original: none (nearest "')
    assert "Matches" not in rec[1] and len(rec[1].splitlines()) == 2
