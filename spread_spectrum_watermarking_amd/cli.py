"""Command line front-end mirroring the reference's example binary (examples/main.rs).

    python -m spread_spectrum_watermarking_amd.cli watermark <file> [--length 1000] [--ordering energy]
            [--alpha 0.1] [--method option2] [-d DESCRIPTION] [-p]
        -> <stem>_wm.png and <stem>_wm.json next to <file>            (main.rs:240-319)
    python -m spread_spectrum_watermarking_amd.cli test [--similarity-exceed 6.0] <base> <watermarked> <json|wm>...
        -> one YAML-ish record per stored watermark                     (main.rs:346-434)
    python -m spread_spectrum_watermarking_amd.cli fingerprint <file> --copies N [--length 1000] [--ordering energy]
            [--alpha 0.1] [--method option2] [-d DESCRIPTION]
        -> <stem>_fp<i>.png (i zero-padded) and one <stem>_fp.json holding the N marks, described "<desc> #i";
           `test <file> <stem>_fp<i>.png <stem>_fp.json` then names the copy that leaked
    python -m spread_spectrum_watermarking_amd.cli trace <base> --suspects A.png B.png ... --marks X_fp.json [Y.json ...]
            [--similarity-exceed 6.0] [--place FILE=X,Y[,WxH] | FILE=rotate:DEGREES | FILE=rotate:? | FILE=rotate:LO..HI ...] [--locate FILE[=WxH|=W0..W1[~A]|=rotate:?|=rotate:LO..HI] ...]
        -> one record per suspect: the stored mark it carries (or none) and every further mark above the threshold;
           one GPU call per group of stored marks with equal (config, length), whatever the number of suspects.
           Attacked copies are restored on the GPU first (tests/attack_resize.rs:31-36, tests/attack_crop.rs:56-70): a
           suspect of another size is resized back to the base's, an alpha channel is blended over the base, and
           --place puts a cut-out where it belongs (at X,Y, scaled to WxH when given); their records say "Restored:".
           --place FILE=rotate:DEGREES turns back a copy of the base's size that was turned by a known angle; FILE=rotate:?
           searches for the angle first (-10 .. 10 degrees; FILE=rotate:LO..HI: that range, within +-45), all such suspects in
           one search on the GPU, and the record says "Turned:".
           --locate finds where a cut-out belongs (the size WxH it had in the base when it was scaled afterwards) by a
           search over every translation on the GPU; its record says "Located:" too.  FILE=W0..W1: the size is not known
           either, only that the cut-out was between W0 and W1 wide in the base -- a search over scale as well.
           FILE=W0..W1~A (A from 1 to 4): its sides were rounded on their own, as a thumbnail's are -- the sizes within A
           pixels of the scale search's answer are rescored in both dimensions.
           FILE=rotate:? (or FILE=rotate:LO..HI): the cut-out was taken from a copy TURNED by an unknown angle -- a search over
           angle and position together; the record says "Located: centre X,Y turned DEGREES"
    python -m spread_spectrum_watermarking_amd.cli index FILES... -o catalogue.npz [--marks FILE_fp.json ...]
        -> creates catalogue.npz or appends to it: one signature (1024 bytes) per original, with its size and the marks file
           that goes with it (given in the order of FILES, else <stem>_fp.json beside the image where that exists)
    python -m spread_spectrum_watermarking_amd.cli identify SUSPECTS... --catalogue catalogue.npz [--top N] [--max-distance D]
        -> one record per suspect: the original it is a copy of, found among all signatures on the GPU, or none when even
           the nearest is further than D (whole-frame copies only: cut-outs, mirrored and turned copies are not identified)
    python -m spread_spectrum_watermarking_amd.cli trace --catalogue catalogue.npz --suspects A.png B.png ... [--marks ...]
        -> `identify` for every suspect in one call, then the trace above once per original that was named, with the marks
           file the catalogue holds for it; every record gains an "Original:" line
    python -m spread_spectrum_watermarking_amd.cli strength <file> --alpha 0.02 0.05 0.1 [-n 1000] [--copies 8] [--collude 2 4]
            [--method average median min max minmax mosaic] [--jpeg 90 75 50] [--filter blur:1.5 median unsharp:2,150,3] [--scale 0.5 0.25:lanczos 640x360:bilinear] [--rotate 0.5 2:bilinear -1 1.3:? 1.3:?-5..5]
            [--crop 0.5 340,160,225x225 0.5:? 0.75@0.5 0.75@0.5:lanczos:? 0.5@0.5:?200..640] [--ssim]
            [--similarity-exceed 6.0] [--json]
        -> before a copy ships: per alpha the PSNR range of the marked copies (with --ssim also their mean SSIM and the worst
           8 x 8 window), and per collusion method and coalition size
           how many of the colluders a trace of their forgery still finds, the weakest colluder's and the strongest innocent
           recipient's similarity; with --jpeg, per quality what a trace still finds in every copy after it was saved as a
           JPEG; with --filter the same after a Gaussian blur (blur:RADIUS), an unsharp mask (unsharp[:RADIUS[,PERCENT[,THRESHOLD]]])
           or a 3 x 3 median (median), as Pillow's filters of those names do them; with --scale the same after the copy was
           scaled as Pillow's Image.resize does it (FACTOR[:FILTER] or WIDTHxHEIGHT[:FILTER]) and brought back to size; with --rotate
           the same after the copy was turned as Pillow's Image.rotate does it (DEGREES[:FILTER]) and turned back by the known
           angle, with the share of the frame that survives the two turns (DEGREES[:FILTER]:? -- the tracer is NOT told the
           angle: every copy's angle is searched for in -10 .. 10 degrees, or in LO..HI with :?LO..HI, and the copy turned back by
           the angle found; the line says which angles were found); with --crop the same after a part of the copy was cut out
           and laid over the original again, as the reference's crop test does it (FRACTION of both sides, centred, or
           X,Y,WIDTHxHEIGHT; @FACTOR or @WIDTHxHEIGHT: the piece was also made a thumbnail, [:FILTER]; :? -- the tracer is NOT
           told where the piece came from and searches for it, a thumbnail's size too, over the widths from its own to the frame's
           or over LO..HI with :?LO..HI; the line says how many copies were placed exactly); everything stays on the GPU between the original going up and the numbers coming down

Host plumbing only (argument parsing, PIL image I/O, JSON); all arithmetic goes through the GPU
library via the crate-surface mirror in api.py.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np

from ._lib import COLLUDE_METHODS
from .api import (IDENTIFY_MAX_DISTANCE, Catalogue, Crop, CropResult, Filter, Locate, MarkBuf, Placement, Reader, Rotate, Rotated, Scale, Tester, TraceResult, Writer, identify, locate, locate_turned, restore_turned,
                  strength_report)
from .storage import Configuration, DescribedWatermark, Version1Storage

_ORDERING_ARGS = {"energy": "Energy", "energy-orthogonal": "EnergyOrthogonal", "legacy": "Legacy"}
_METHOD_ARGS = {"option1": "Option1", "option2": "Option2", "option3": "Option3"}


def _filter_arg(text: str) -> Filter:
    """blur:RADIUS | unsharp[:RADIUS[,PERCENT[,THRESHOLD]]] | median[:3]"""
    name, _, rest = text.partition(":")
    parts = rest.split(",") if rest else []
    try:
        if name == "blur" and len(parts) == 1:
            return Filter.blur(float(parts[0]))
        if name == "unsharp" and len(parts) <= 3:
            return Filter.unsharp(*([float(parts[0])] if parts else []), *[int(v) for v in parts[1:]])
        if name == "median" and parts in ([], ["3"]):
            return Filter.median()
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"{text!r}: {e}") from e
    raise argparse.ArgumentTypeError(f"{text!r}: blur:RADIUS, unsharp[:RADIUS[,PERCENT[,THRESHOLD]]] or median")


def _scale_arg(text: str) -> Scale:
    """FACTOR[:FILTER] | WIDTHxHEIGHT[:FILTER]"""
    what, colon, name = text.partition(":")
    try:
        if colon and not name:
            raise ValueError("a filter's name after the colon")
        if "x" in what:
            nw, _, nh = what.partition("x")
            return Scale.to(int(nw), int(nh), name or "bicubic")
        return Scale(float(what), name or "bicubic")
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"{text!r}: FACTOR[:FILTER] or WIDTHxHEIGHT[:FILTER] ({e})") from e


def _rotate_arg(text: str) -> Rotate:
    """DEGREES[:FILTER][:?[LO..HI]] -- a last part that begins with `?`: the tracer is not told the angle and searches for it, in
    -10 .. 10 degrees or in LO..HI"""
    what, *rest = text.split(":")
    try:
        search = None
        if rest and rest[-1].startswith("?"):
            spec = rest.pop()[1:]
            search = True
            if spec:
                lo, dots, hi = spec.partition("..")
                if not dots:
                    raise ValueError("?LO..HI names both ends of the range")
                search = (float(lo), float(hi))
        if len(rest) > 1 or (rest and not rest[0]):
            raise ValueError("a filter's name after the colon")
        return Rotate(float(what), rest[0] if rest else "bicubic", search)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"{text!r}: DEGREES[:FILTER][:?[LO..HI]] ({e})") from e


def _crop_arg(text: str) -> Crop:
    """FRACTION | X,Y,WIDTHxHEIGHT, then [@FACTOR | @WIDTHxHEIGHT][:FILTER][:?[LO..HI]] -- a last part that begins with `?`: the
    tracer is not told where the piece came from and searches for it"""
    what, *rest = text.split(":")
    try:
        search = None
        if rest and rest[-1].startswith("?"):
            spec = rest.pop()[1:]
            search = True
            if spec:
                lo, dots, hi = spec.partition("..")
                if not dots:
                    raise ValueError("?LO..HI names both ends of the range")
                search = (int(lo), int(hi))
        if len(rest) > 1 or (rest and not rest[0]):
            raise ValueError("a filter's name after the colon")
        what, at, size = what.partition("@")
        more = {"filter": rest[0] if rest else "bicubic", "search": search}
        if at:
            if "x" in size:
                tw, _, th = size.partition("x")
                more["to"] = (int(tw), int(th))
            else:
                more["scale"] = float(size)
                if not more["scale"]:
                    raise ValueError("a factor above 0 after the @")
        elif rest:
            raise ValueError("a filter goes with @FACTOR or @WIDTHxHEIGHT")
        if "," in what:
            x, y, size = what.split(",")
            cw, _, ch = size.partition("x")
            return Crop.rect(int(x), int(y), int(cw), int(ch), **more)
        return Crop(float(what), **more)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"{text!r}: FRACTION or X,Y,WIDTHxHEIGHT, then [@FACTOR|@WIDTHxHEIGHT][:FILTER][:?[LO..HI]] ({e})") from e


def _rust_f32(x: float) -> str:
    """`{}` of an f32 in Rust: shortest round-trip digits, no trailing `.0`."""
    s = np.format_float_positional(np.float32(x), unique=True, trim="-")
    return s


def _open_image(path: str) -> np.ndarray:
    from PIL import Image
    try:
        return np.asarray(Image.open(path).convert("RGB"))
    except Exception as e:                       # the reference panics with this message
        raise SystemExit(f"Could not load image at {path!r}") from e


def _open_suspect(path: str) -> np.ndarray:
    """A suspect keeps its alpha channel (RGBA); anything else is read like the base."""
    from PIL import Image
    try:
        im = Image.open(path)
        has_alpha = im.mode in ("RGBA", "LA", "PA") or (im.mode == "P" and "transparency" in im.info)
        return np.asarray(im.convert("RGBA" if has_alpha else "RGB"))
    except Exception as e:
        raise SystemExit(f"Could not load image at {path!r}") from e


def parse_place(text: str):
    """FILE=X,Y[,WxH] -> (FILE, Placement); FILE=rotate:DEGREES, FILE=rotate:? or FILE=rotate:LO..HI -> (FILE, Rotated);
    ValueError on anything else."""
    name, sep, spec = text.rpartition("=")
    if sep and name and spec.startswith("rotate:"):
        what = spec[len("rotate:"):]
        try:
            if what == "?":
                return name, Rotated()
            if ".." in what:
                lo, _, hi = what.partition("..")
                return name, Rotated(search=(float(lo), float(hi)))
            return name, Rotated(float(what))
        except ValueError:
            raise ValueError(f"--place {text!r}: expected FILE=rotate:DEGREES, FILE=rotate:? or FILE=rotate:LO..HI (within -45 .. 45)") from None
    parts = spec.split(",")
    if not sep or not name or len(parts) not in (2, 3):
        raise ValueError(f"--place {text!r}: expected FILE=X,Y[,WxH]")
    try:
        x, y = int(parts[0]), int(parts[1])
        w = h = None
        if len(parts) == 3:
            ws, xs, hs = parts[2].partition("x")
            if not xs:
                raise ValueError
            w, h = int(ws), int(hs)
    except ValueError:
        raise ValueError(f"--place {text!r}: expected FILE=X,Y[,WxH]") from None
    if x < 0 or y < 0 or (w is not None and (w <= 0 or h <= 0)):
        raise ValueError(f"--place {text!r}: negative position or empty size")
    return name, Placement(x, y, w, h)


def turned_text(f) -> str:
    """The record's "Turned:" value of a suspect whose angle was searched for (f: a FoundAngle)."""
    degrees = f"{f.angle:.5f}".rstrip("0").rstrip(".")          # n / 32: five decimals are all there are
    return f"{degrees} (mean luma difference {f.mean:.2f})"


def trace_placements(suspects: List[str], place: Optional[List[str]]) -> Dict[str, Placement]:
    """The --place options by suspect; ValueError for a malformed one, a FILE not among --suspects, or one placed twice."""
    out: Dict[str, Placement] = {}
    for text in place or []:
        name, p = parse_place(text)
        if name not in suspects:
            raise ValueError(f"--place {text!r}: {name!r} is not among --suspects")
        if name in out:
            raise ValueError(f"--place {text!r}: {name!r} is placed twice")
        out[name] = p
    return out


def parse_locate(text: str, suspects: List[str]) -> Tuple[str, Locate]:
    """FILE[=WxH] or FILE=W0..W1[~A] -> (FILE, Locate); a text that is one of the suspects as it stands is a FILE without a size.
    ValueError on anything else."""
    if text in suspects:
        return text, Locate()
    name, sep, spec = text.rpartition("=")
    if spec.startswith("rotate:"):                       # a cut-out of a turned copy: angle and position are both unknown
        try:
            if not sep or not name:
                raise ValueError
            lo, dots, hi = spec[len("rotate:"):].partition("..")
            z = Locate(turned=True) if (lo, dots, hi) == ("?", "", "") else Locate(turned=(float(lo), float(hi)))
            z.turned_range()
        except ValueError:
            raise ValueError(f"--locate {text!r}: expected FILE=rotate:? or FILE=rotate:LO..HI, degrees within +-45") from None
        return name, z
    if ".." in spec:                                     # a range of widths: the scale is unknown
        spec, tilde, slack = spec.partition("~")         # ~A: the height may differ from the kept-aspect one by up to A pixels
        lo, _, hi = spec.partition("..")
        if not sep or not name or not (lo.isascii() and lo.isdigit() and hi.isascii() and hi.isdigit()):
            raise ValueError(f"--locate {text!r}: expected FILE=W0..W1[~A]")
        if tilde and not (slack.isascii() and slack.isdigit() and len(slack) == 1 and 0 <= int(slack) <= 4):
            raise ValueError(f"--locate {text!r}: expected FILE=W0..W1~A with A from 0 to 4")
        if not 0 < int(lo) <= int(hi):
            raise ValueError(f"--locate {text!r}: an empty range of widths")
        return name, (Locate(widths=(int(lo), int(hi)), aspect=int(slack)) if tilde else Locate(widths=(int(lo), int(hi))))
    ws, xs, hs = spec.partition("x")
    if not sep or not name or not xs or not (ws.isascii() and ws.isdigit() and hs.isascii() and hs.isdigit()):
        raise ValueError(f"--locate {text!r}: expected FILE[=WxH]")
    if int(ws) <= 0 or int(hs) <= 0:
        raise ValueError(f"--locate {text!r}: empty size")
    return name, Locate(int(ws), int(hs))


def located_text(f, ranged: bool) -> str:
    """The record's "Located:" value; an entry whose size was searched for says what was found."""
    size = f" as {f.placement.w}x{f.placement.h}" if ranged else ""
    return f"{f.placement.x},{f.placement.y}{size} (mean luma difference {f.mean_abs_diff:.2f})"


def located_turned_text(f) -> str:
    """The record's "Located:" value of a cut-out of a turned copy (f: a LocatedTurned)."""
    degrees = f"{f.angle:.5f}".rstrip("0").rstrip(".")          # n / 32: five decimals are all there are
    return f"centre {f.centre[0]:.1f},{f.centre[1]:.1f} turned {degrees} (mean luma difference {f.mean_abs_diff:.2f})"


def trace_locates(suspects: List[str], locates: Optional[List[str]], placed: Dict[str, Placement]) -> Dict[str, Locate]:
    """The --locate options by suspect; ValueError for a malformed one, a FILE not among --suspects, one located twice, or one
    that also has a --place."""
    out: Dict[str, Locate] = {}
    for text in locates or []:
        name, z = parse_locate(text, suspects)
        if name not in suspects:
            raise ValueError(f"--locate {text!r}: {name!r} is not among --suspects")
        if name in out:
            raise ValueError(f"--locate {text!r}: {name!r} is located twice")
        if name in placed:
            raise ValueError(f"--locate {text!r}: {name!r} also has a --place")
        out[name] = z
    return out


class _TraceParser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if getattr(a, "command", None) == "trace":
            # the original and the marks may come from a catalogue instead; without one they are required, in argparse's words
            needed = ["--suspects"] if a.catalogue is not None else ["base", "--suspects", "--marks"]
            missing = [n for n in needed if getattr(a, n.lstrip("-")) is None]
            if missing:
                self.trace_parser.error("the following arguments are required: " + ", ".join(missing))
            if a.catalogue is not None and a.base is not None:
                self.trace_parser.error("give the original or --catalogue, not both")
            try:
                a.placements = trace_placements(a.suspects, a.place)
                a.locates = trace_locates(a.suspects, a.locate, a.placements)
            except ValueError as e:
                self.error(str(e))
        return a


def build_parser() -> argparse.ArgumentParser:
    p = _TraceParser(prog="spread_spectrum_watermarking_amd.cli")
    sub = p.add_subparsers(dest="command", parser_class=argparse.ArgumentParser)
    w = sub.add_parser("watermark", help="Embed a watermark into a file.")
    w.add_argument("file", help="The file to to watermark.")
    w.add_argument("--length", type=int, default=1000, help="Watermark length.")
    w.add_argument("--ordering", choices=sorted(_ORDERING_ARGS), default="energy", help="The ordering to be used.")
    w.add_argument("--alpha", type=float, default=0.1, help="Strength, alpha in the equations.")
    w.add_argument("--method", choices=sorted(_METHOD_ARGS), default="option2", help="Method to insert and extract with.")
    w.add_argument("-d", "--description", default=None, help="Description to associate with the watermark.")
    w.add_argument("-p", dest="print_similarity", action="store_true", help="Show embedded watermark similarity.")
    f = sub.add_parser("fingerprint", help="Make individually watermarked copies of a file, one mark per recipient.")
    f.add_argument("file", help="The file to make copies of.")
    f.add_argument("--copies", type=int, required=True, help="Number of copies (one watermark each).")
    f.add_argument("--length", type=int, default=1000, help="Watermark length.")
    f.add_argument("--ordering", choices=sorted(_ORDERING_ARGS), default="energy", help="The ordering to be used.")
    f.add_argument("--alpha", type=float, default=0.1, help="Strength, alpha in the equations.")
    f.add_argument("--method", choices=sorted(_METHOD_ARGS), default="option2", help="Method to insert and extract with.")
    f.add_argument("-d", "--description", default=None, help="Description; copy i is described \"<description> #i\".")
    t = sub.add_parser("test", help="Test if any of the watermarks are present in the watermarked file.")
    t.add_argument("--similarity-exceed", type=float, default=6.0,
                   help="If the similarity exceeds this value it is considered to be matching.")
    t.add_argument("base", help="The original file.")
    t.add_argument("watermarked", help="The derived (watermarked) file.")
    t.add_argument("watermark_files", nargs="+", help="The watermark files to test from.")
    r = sub.add_parser("trace", help="Name, for each suspect file, the stored watermark it carries.")
    r.add_argument("--similarity-exceed", type=float, default=6.0,
                   help="If the similarity exceeds this value it is considered to be matching.")
    r.add_argument("base", nargs="?", default=None, help="The original file (not with --catalogue).")
    r.add_argument("--suspects", nargs="+", help="The files to trace.")
    r.add_argument("--marks", nargs="+", help="The watermark files to test from (with --catalogue: besides the catalogue's own).")
    r.add_argument("--catalogue", default=None, metavar="CATALOGUE.npz",
                   help="Name each suspect's original from this catalogue (see `index`) instead of giving it.")
    r.add_argument("--max-distance", type=int, default=IDENTIFY_MAX_DISTANCE,
                   help="With --catalogue: the largest signature distance that still names an original.")
    p.trace_parser = r
    r.add_argument("--place", action="append", metavar="FILE=X,Y[,WxH]",
                   help="Where the cut-out FILE (one of --suspects) lies in the base, and the size it had there; "
                        "FILE=rotate:DEGREES: a copy turned by a known angle; FILE=rotate:? or FILE=rotate:LO..HI: the angle is "
                        "searched for. Repeatable.")
    r.add_argument("--locate", action="append", metavar="FILE[=WxH|=W0..W1[~A]|=rotate:?|=rotate:LO..HI]",
                   help="Find where the cut-out FILE (one of --suspects) lies in the base; WxH: the size it had there; "
                        "W0..W1: the widths it may have had there (the scale is searched too; ~A, 1 to 4: width and height may each be "
                        "up to A pixels off the size that search answers, as a thumbnail's rounded sides are); rotate:? or rotate:LO..HI: it was "
                        "cut out of a turned copy (angle and position are searched together). Repeatable.")
    x = sub.add_parser("index", help="Add originals to an image catalogue (created when it does not exist).")
    x.add_argument("files", nargs="+", help="The originals.")
    x.add_argument("-o", "--output", required=True, metavar="CATALOGUE.npz", help="The catalogue file.")
    x.add_argument("--marks", nargs="+", default=None, metavar="FILE_fp.json",
                   help="The marks file of each original, in the order of the files (default: <stem>_fp.json beside it, if there).")
    i = sub.add_parser("identify", help="Name, for each suspect file, the original in the catalogue it is a copy of.")
    i.add_argument("suspects", nargs="+", help="The files to identify.")
    i.add_argument("--catalogue", required=True, metavar="CATALOGUE.npz", help="The catalogue file (see `index`).")
    i.add_argument("--top", type=int, default=1, help="Also list the runners-up, N entries in all (1 .. 8).")
    i.add_argument("--max-distance", type=int, default=IDENTIFY_MAX_DISTANCE,
                   help="The largest signature distance that still names an original.")
    g = sub.add_parser("strength", help="Report a mark's visibility and its collusion resistance for one or more strengths.")
    g.add_argument("file", help="The file copies would be made of.")
    g.add_argument("--alpha", type=float, nargs="+", required=True, help="The strengths to report on.")
    g.add_argument("-n", "--length", type=int, default=1000, help="Watermark length.")
    g.add_argument("--copies", type=int, default=8, help="Number of recipients.")
    g.add_argument("--collude", type=int, nargs="+", default=[2, 4], metavar="C", help="Coalition sizes (the first C recipients).")
    g.add_argument("--method", nargs="+", choices=list(COLLUDE_METHODS), default=list(COLLUDE_METHODS), help="Collusion methods.")
    g.add_argument("--similarity-exceed", type=float, default=6.0,
                   help="If the similarity exceeds this value it is considered to be matching.")
    g.add_argument("--jpeg", type=int, nargs="+", default=[], metavar="Q",
                   help="Also compress every copy as a JPEG of these qualities (1 .. 100) and trace what is left.")
    g.add_argument("--filter", type=_filter_arg, nargs="+", default=[], metavar="FILTER", dest="filters",
                   help="Also put every copy through these filters and trace what is left: blur:RADIUS (0 < RADIUS <= 8), "
                        "unsharp[:RADIUS[,PERCENT[,THRESHOLD]]] (default 2,150,3), median.")
    g.add_argument("--scale", type=_scale_arg, nargs="+", default=[], metavar="SCALE", dest="scales",
                   help="Also scale every copy as Pillow's Image.resize does, bring it back to size and trace what is left: "
                        "FACTOR[:FILTER] (0 < FACTOR <= 4) or WIDTHxHEIGHT[:FILTER]; FILTER box, bilinear, bicubic (default) or lanczos.")
    g.add_argument("--rotate", type=_rotate_arg, nargs="+", default=[], metavar="ROTATION", dest="rotations",
                   help="Also turn every copy as Pillow's Image.rotate does, turn it back by the known angle and trace what is left: "
                        "DEGREES[:FILTER]; FILTER bilinear or bicubic (default).  With :? at the end (1.3:?, 2:bilinear:?, 1.3:?-5..5) the "
                        "angle is not told: it is searched for in -10 .. 10 degrees (or LO..HI) and the copy turned back by the angle found.")
    g.add_argument("--crop", type=_crop_arg, nargs="+", default=[], metavar="CROP", dest="crops",
                   help="Also cut a part out of every copy, lay it over the original again and trace what is left: FRACTION (of both "
                        "sides, centred) or X,Y,WIDTHxHEIGHT; with @FACTOR or @WIDTHxHEIGHT[:FILTER] the piece is also made a thumbnail.  "
                        "With :? at the end (0.5:?, 0.75@0.5:lanczos:?, 0.5@0.5:?200..640) the tracer is not told where the piece came "
                        "from: its position, and a thumbnail's size over its own width up to the frame's (or LO..HI), are searched for.")
    g.add_argument("--ssim", action="store_true", help="Also report the structural similarity (SSIM) of every copy and its worst window.")
    g.add_argument("--json", action="store_true", help="Print the report as one JSON document.")
    return p


def out_paths(image_path: str) -> Tuple[str, str]:
    """/tmp/foo.jpg -> /tmp/foo_wm.png, /tmp/foo_wm.json (main.rs:245-251)."""
    stem = os.path.splitext(image_path)[0] + "_wm"
    return stem + ".png", stem + ".json"


def cmd_watermark(args, out=sys.stdout) -> int:
    orig = _open_image(args.file)
    image_out, json_out = out_paths(args.file)
    for path in (image_out, json_out):                       # main.rs:253-265
        if os.path.exists(path):
            raise SystemExit(f"{path} file already exists")
    cfg = Configuration(alpha=args.alpha, method=_METHOD_ARGS[args.method], ordering=_ORDERING_ARGS[args.ordering])
    mark = MarkBuf.generate_normal(args.length)              # main.rs:269
    # main.rs:271-278: Writer::new(orig).mark(&[&mark]).into_rgb8() -- 8-bit in, 8-bit out, quantised on the device
    derived8 = Writer(orig, cfg.to_write_config()).mark_rgb8([mark])
    from PIL import Image
    Image.fromarray(derived8).save(image_out)
    storage = Version1Storage(cfg, [DescribedWatermark(mark.data(), args.description or "")])
    with open(json_out, "w") as f:
        f.write(storage.to_json())
    if args.print_similarity:                                # main.rs:306-316 (default ReadConfig, like the reference)
        from .api import ReadConfig
        ext = Reader.base(orig, ReadConfig.default()).extract(Reader.derived(derived8), args.length)
        sim = Tester(ext).similarity(mark)
        print(f"sim: Similarity {{ similarity: {_rust_f32(sim.similarity)} }}", file=out)
        print(f"exceeds 6 sigma: {'true' if sim.exceeds_sigma(6.0) else 'false'}", file=out)
    return 0


def fingerprint_paths(image_path: str, copies: int) -> Tuple[List[str], str]:
    """/tmp/foo.jpg, 12 -> [/tmp/foo_fp00.png .. /tmp/foo_fp11.png], /tmp/foo_fp.json."""
    stem = os.path.splitext(image_path)[0] + "_fp"
    digits = len(str(max(copies - 1, 0)))
    return [f"{stem}{i:0{digits}d}.png" for i in range(copies)], stem + ".json"


def cmd_fingerprint(args, out=sys.stdout) -> int:
    if args.copies < 1:
        raise SystemExit("--copies must be at least 1")
    images_out, json_out = fingerprint_paths(args.file, args.copies)
    for path in images_out + [json_out]:                     # like `watermark` (main.rs:253-265): never overwrite
        if os.path.exists(path):
            raise SystemExit(f"{path} file already exists")
    orig = _open_image(args.file)
    cfg = Configuration(alpha=args.alpha, method=_METHOD_ARGS[args.method], ordering=_ORDERING_ARGS[args.ordering])
    marks = [MarkBuf.generate_normal(args.length) for _ in range(args.copies)]
    # main.rs:266-278 once per recipient, as one call: Writer::new(orig) once, then every copy from the shared transform
    copies8 = Writer(orig, cfg.to_write_config()).mark_copies_rgb8(marks)
    from PIL import Image
    for path, img in zip(images_out, copies8):
        Image.fromarray(img).save(path)
    desc = args.description or ""
    storage = Version1Storage(cfg, [DescribedWatermark(m.data(), f"{desc} #{i}" if desc else f"#{i}") for i, m in enumerate(marks)])
    with open(json_out, "w") as f:
        f.write(storage.to_json())
    print(f"{args.copies} copies: {images_out[0]} .. {images_out[-1]}, marks in {json_out}", file=out)
    return 0


def cmd_test(args, out=sys.stdout) -> int:
    base = _open_image(args.base)
    watermarked = _open_image(args.watermarked)
    stored: List[Tuple[str, Version1Storage]] = [(p, Version1Storage.load(p)) for p in args.watermark_files]
    retrieved: Dict[Tuple[Configuration, int], np.ndarray] = {}          # main.rs:369-371
    for path, info in stored:
        for wmk in info.watermarks:
            key = (info.config, len(wmk.values))
            if key not in retrieved:                                     # main.rs:383-407
                reader = Reader.base(base, info.config.to_read_config())
                retrieved[key] = reader.extract(Reader.derived(watermarked), key[1])
            sim = Tester(retrieved[key]).similarity(wmk.values)
            desc = wmk.description.replace('"', '\\"')
            print("-", file=out)                                          # main.rs:418-429
            print(f"  Matches: {'true' if sim.exceeds_sigma(args.similarity_exceed) else 'false'}", file=out)
            print(f"  Similarity: {_rust_f32(sim.similarity)}", file=out)
            print(f"  MatchExceed: {_rust_f32(args.similarity_exceed)}", file=out)
            print(f"  Description: \"{desc}\"", file=out)
            print(f"  File: \"{path}\"", file=out)
    return 0


def group_stored_marks(stored: List[Tuple[str, Version1Storage]]) -> Dict[Tuple[Configuration, int], List[Tuple[str, DescribedWatermark]]]:
    """The stored marks by (config, length) -- the key `test` caches its extractions under (main.rs:369-371) -- in file order."""
    groups: Dict[Tuple[Configuration, int], List[Tuple[str, DescribedWatermark]]] = {}
    for path, info in stored:
        for wmk in info.watermarks:
            groups.setdefault((info.config, len(wmk.values)), []).append((path, wmk))
    return groups


def default_marks_file(image_path: str) -> Optional[str]:
    """<stem>_fp.json beside the image (what `fingerprint` writes), if it exists."""
    path = os.path.splitext(image_path)[0] + "_fp.json"
    return path if os.path.exists(path) else None


def cmd_index(args, out=sys.stdout) -> int:
    if args.marks is not None and len(args.marks) != len(args.files):
        raise SystemExit(f"--marks: {len(args.marks)} files for {len(args.files)} originals (one each, in order)")
    cat = Catalogue.load(args.output) if os.path.exists(args.output) else Catalogue()
    marks = args.marks if args.marks is not None else [default_marks_file(f) for f in args.files]
    cat.add_many(args.files, [_open_image(f) for f in args.files], marks)
    cat.save(args.output)
    print(f"{len(args.files)} added, {len(cat)} originals in {args.output}", file=out)
    return 0


def original_text(r) -> str:
    """The value of a record's "Original:" line for one `Identified`."""
    if r.nearest is None:
        return "none (the catalogue is empty)"
    name = r.nearest.replace('"', '\\"')
    if r.name is None:
        return f"none (nearest \"{name}\", distance {r.distance})"
    return f"\"{name}\" {r.size[0]}x{r.size[1]} (distance {r.distance})"


def cmd_identify(args, out=sys.stdout) -> int:
    if not 1 <= args.top <= 8:
        raise SystemExit("--top must be 1 .. 8")
    cat = Catalogue.load(args.catalogue)
    found = identify(cat, [_open_suspect(p) for p in args.suspects], args.top, args.max_distance)
    for path, r in zip(args.suspects, found):
        print("-", file=out)
        print(f"  Suspect: \"{path}\"", file=out)
        print(f"  Original: {original_text(r)}", file=out)
        for name, d, (w, h) in r.candidates[1:]:
            n = name.replace('"', '\\"')
            print(f"  Next: \"{n}\" {w}x{h} (distance {d})", file=out)
    return 0


def cmd_strength(args, out=None) -> int:
    out = out or sys.stdout                                  # looked up at the call: a caller may have redirected it
    orig = _open_image(args.file)
    scales, rotations, crops = getattr(args, "scales", []), getattr(args, "rotations", []), getattr(args, "crops", [])
    try:
        rows = strength_report(orig, args.alpha, k=args.length, copies=args.copies, sizes=args.collude, methods=args.method,
                               threshold=args.similarity_exceed, jpeg=args.jpeg, ssim=args.ssim, filters=args.filters, scales=scales,
                               rotations=rotations, **({"crops": crops} if crops else {}))
    except ValueError as e:
        raise SystemExit(str(e)) from e
    if args.json:
        import json
        num = lambda v: None if v != v else (v if abs(v) != float("inf") else str(v))      # JSON has no NaN / Infinity

        def attack(key, a):                                  # a JpegResult or a FilterResult: `key` names its first field
            return {key: getattr(a, key), "survived": a.survived, "accused": a.accused, "weakest_own": num(a.weakest_own),
                    "strongest_innocent": num(a.strongest_innocent), "psnr_min": num(a.psnr_min), "psnr_max": num(a.psnr_max)}
        doc = [{"alpha": r.alpha,
                "copies": [{"psnr": num(q.psnr), "psnr_luma": num(q.psnr_luma), "sse": list(q.sse), "sse_luma": q.sse_luma,
                            "changed": q.changed, "max_abs": q.max_abs, "pixels": q.pixels} for q in r.quality],
                "collusions": [{"method": c.method, "size": c.size, "found": c.found, "accused": c.accused,
                                "weakest_colluder": num(c.weakest_colluder), "strongest_innocent": num(c.strongest_innocent)}
                               for c in r.collusions],
                "jpeg": [attack("quality", j) for j in r.jpeg], "filters": [attack("filter", f) for f in r.filters]} for r in rows]
        for d, r in zip(doc, rows):
            for c, s in zip(d["copies"], r.ssim):
                c.update({"ssim": s.mean, "ssim_worst": s.worst_value, "ssim_worst_at": list(s.worst_position)})
            if scales:                                       # the key is there when --scale was given
                d["scales"] = [dict(attack("scale", a), size=list(a.size)) for a in r.scales]
            if rotations:                                    # ... when --rotate was given
                d["rotations"] = [dict(attack("rotation", a), kept=a.kept) for a in r.rotations]
                for row, a in zip(d["rotations"], r.rotations):
                    if a.search is not None:             # the angle was searched for: what was found
                        row.update(search=list(a.search), found_min=a.found_min, found_max=a.found_max, worst_angle_error=a.worst_angle_error)
            if crops:                                        # ... when --crop was given
                d["crops"] = [dict(attack("crop", a), rect=list(a.rect), thumb=list(a.thumb) if a.thumb else None, kept=a.kept) for a in r.crops]
                for row, a in zip(d["crops"], r.crops):
                    if a.search is not None:             # the place was searched for: what was found
                        row.update(search=list(a.search), found=[list(f) for f in a.found], found_exact=a.found_exact,
                                   worst_offset=list(a.worst_offset), worst_size_error=list(a.worst_size_error))
        print(json.dumps(doc), file=out)
        return 0
    for r in rows:
        psnr = [q.psnr for q in r.quality]
        print("-", file=out)
        print(f"  Alpha: {_rust_f32(r.alpha)}", file=out)
        print(f"  PSNR: {min(psnr):.2f} .. {max(psnr):.2f} dB over {len(psnr)} copies "
              f"(largest byte difference {max(q.max_abs for q in r.quality)})", file=out)
        if r.ssim:
            mean, worst = [s.mean for s in r.ssim], min(range(len(r.ssim)), key=lambda i: r.ssim[i].worst)
            x, y = r.ssim[worst].worst_position
            print(f"  SSIM: {min(mean):.4f} .. {max(mean):.4f} over {len(mean)} copies, "
                  f"worst window {r.ssim[worst].worst_value:.4f} at {x},{y} (copy {worst})", file=out)
        for c in r.collusions:
            innocent = "none" if c.strongest_innocent != c.strongest_innocent else f"{c.strongest_innocent:.2f}"
            accused = f", {c.accused} innocent accused" if c.accused else ""
            print(f"  {c.method} of {c.size}: found {c.found}/{c.size}, weakest colluder {c.weakest_colluder:.2f}, "
                  f"strongest innocent {innocent}{accused}", file=out)
        for label, a in ([(f"jpeg {j.quality}", j) for j in r.jpeg] + [(f.filter, f) for f in r.filters] +
                         [(f"{a.scale} ({a.size[0]}x{a.size[1]})", a) for a in r.scales] + [(a.rotation, a) for a in r.rotations] +
                         [(f"{a.crop} ({a.size[0]}x{a.size[1]} at {a.rect[0]},{a.rect[1]}" + (f" -> {a.thumb[0]}x{a.thumb[1]})" if a.thumb else ")"), a)
                          for a in r.crops]):
            innocent = "none" if a.strongest_innocent != a.strongest_innocent else f"{a.strongest_innocent:.1f}"
            accused = f", {a.accused} innocent accused" if a.accused else ""
            ssim = f", ssim {a.ssim_min:.2f} .. {a.ssim_max:.2f}" if r.ssim else ""
            kept = f", {100 * a.kept:.1f} % kept" if hasattr(a, "kept") else ""
            found = ""
            if getattr(a, "search", None) is not None:
                found = (f"place searched: exact in {a.found_exact}/{len(r.quality)}, worst offset {a.worst_offset[0]},{a.worst_offset[1]}, "
                         f"worst size {a.worst_size_error[0]}x{a.worst_size_error[1]}, " if isinstance(a, CropResult)
                         else f"found {a.found_min:g} .. {a.found_max:g}, ")
            print(f"  {label}: {found}own mark found {a.survived}/{len(r.quality)}, weakest {a.weakest_own:.1f}, "
                  f"strongest innocent {innocent}{accused}, {a.psnr_min:.1f} .. {a.psnr_max:.1f} dB{ssim}{kept}", file=out)
    return 0


def _beside(path: str, catalogue_path: str) -> str:
    """A file named in a catalogue: as it is named, else relative to the catalogue's directory."""
    if os.path.exists(path) or os.path.isabs(path):
        return path
    return os.path.join(os.path.dirname(os.path.abspath(catalogue_path)), path)


def cmd_trace_catalogue(args, out=sys.stdout) -> int:
    """trace --catalogue: every suspect identified in one match call, then today's trace once per original that was named,
    with its stored marks file; an unidentified suspect gets a record that says so and is not traced."""
    import argparse as _ap
    import io
    cat = Catalogue.load(args.catalogue)
    found = identify(cat, [_open_suspect(p) for p in args.suspects], 1, args.max_distance)
    groups: Dict[int, List[int]] = {}
    for s, r in enumerate(found):
        if r.name is not None:
            groups.setdefault(r.index, []).append(s)
    records: Dict[int, List[str]] = {}
    for index, members in groups.items():
        r = found[members[0]]
        marks = ([_beside(r.marks_file, args.catalogue)] if r.marks_file else []) + list(args.marks or [])
        if not marks:
            raise SystemExit(f"{r.name}: the catalogue holds no marks file for it and no --marks was given")
        paths = [args.suspects[s] for s in members]
        sub = _ap.Namespace(base=_beside(r.name, args.catalogue), suspects=paths, marks=marks, similarity_exceed=args.similarity_exceed,
                            placements={k: v for k, v in getattr(args, "placements", {}).items() if k in paths},
                            locates={k: v for k, v in getattr(args, "locates", {}).items() if k in paths})
        buf = io.StringIO()
        cmd_trace(sub, buf)
        lines = buf.getvalue().splitlines()
        starts = [i for i, ln in enumerate(lines) if ln == "-"] + [len(lines)]
        for s, a, b in zip(members, starts[:-1], starts[1:]):
            records[s] = lines[a:b]
    for s, path in enumerate(args.suspects):
        rec = records.get(s) or ["-", f"  Suspect: \"{path}\""]
        for ln in rec[:2]:
            print(ln, file=out)
        print(f"  Original: {original_text(found[s])}", file=out)
        for ln in rec[2:]:
            print(ln, file=out)
    return 0


def cmd_trace(args, out=sys.stdout) -> int:
    if getattr(args, "catalogue", None) is not None:
        return cmd_trace_catalogue(args, out)
    base = _open_image(args.base)
    suspects = [_open_suspect(p) for p in args.suspects]
    H, W = base.shape[:2]
    # what restoration does to each suspect (None: same-shape RGB, traced as it is): tests/attack_resize.rs:31-36 for another
    # size, tests/attack_crop.rs:56-70 for an alpha channel or a placed cut-out
    placements: List[Optional[Placement]] = []
    restored: List[Optional[str]] = []
    # --locate: every cut-out at an unknown position is found with one call; from here on it is a placed suspect
    placed: Dict[str, Placement] = dict(getattr(args, "placements", {}))
    located: Dict[str, str] = {}
    wanted = [(path, img, z) for path, img in zip(args.suspects, suspects) for z in [getattr(args, "locates", {}).get(path)] if z is not None]
    # ... and every cut-out of a turned copy with one call per range; laid back into the frame, it is a whole frame from here on
    laid_back: Dict[str, str] = {}
    cuts = [(path, img, z) for path, img, z in wanted if z.turned_range() is not None]
    wanted = [(path, img, z) for path, img, z in wanted if z.turned_range() is None]
    for path, img, _ in cuts:
        if img.shape[2] != 3:
            raise SystemExit(f"{path}: a cut-out of a turned copy has no alpha channel")
    for search in sorted({z.turned_range() for _, _, z in cuts}):
        group = [(path, img) for path, img, z in cuts if z.turned_range() == search]
        found = locate_turned(base, [img for _, img in group], search)
        for (path, _), f, frame in zip(group, found, restore_turned(base, [img for _, img in group], found)):
            suspects[args.suspects.index(path)] = frame
            located[path] = located_turned_text(f)
            laid_back[path] = f"turned back by {f.angle:g} degrees about {f.centre[0]:.1f},{f.centre[1]:.1f}, completed with the base"
    for path, img, z in wanted:
        if z.widths is not None:
            continue                                     # the ladder drops the widths that do not fit
        zw, zh = (z.w, z.h) if z.w is not None else (img.shape[1], img.shape[0])
        if zw > W or zh > H:
            raise SystemExit(f"{path}: a {zw}x{zh} cut-out does not fit the base ({W}x{H})")
    if wanted:
        for (path, _, z), f in zip(wanted, locate(base, [img for _, img, _ in wanted], [z for _, _, z in wanted])):
            placed[path] = f.placement
            located[path] = located_text(f, z.widths is not None)
    for path, img in zip(args.suspects, suspects):
        sh, sw, c = img.shape
        p = placed.get(path)
        if path in laid_back:
            placements.append(None)
            restored.append(laid_back[path])
            continue
        if isinstance(p, Rotated):
            if (sw, sh, c) != (W, H, 3):
                raise SystemExit(f"{path}: a turned copy has the base's size ({W}x{H}) and no alpha channel")
            placements.append(p)
            restored.append(f"turned back by {p.angle:g} degrees, completed with the base" if p.angle is not None
                            else "turned back by the angle found, completed with the base")
            continue
        if p is None and c == 3 and (sw, sh) == (W, H):
            placements.append(None)
            restored.append(None)
            continue
        if p is None:
            p = Placement()
            if c == 3 and sw <= W and sh <= H and (sw < W or sh < H):
                print(f"{path}: smaller than the base and not placed: taken as a scaled copy of the whole frame "
                      f"(--place {path}=X,Y for a cut-out at a known position, --locate {path} to find it)", file=sys.stderr)
        whole = p.w is None and (p.x, p.y) == (0, 0) and (sw, sh) != (W, H)
        pw, ph = (W, H) if whole else ((p.w, p.h) if p.w is not None else (sw, sh))
        if p.x + pw > W or p.y + ph > H:
            raise SystemExit(f"{path}: placed at {p.x},{p.y} with size {pw}x{ph}, it leaves the base ({W}x{H})")
        what = []
        if (pw, ph) != (sw, sh):
            what.append(f"resize {sw}x{sh} -> {pw}x{ph}")
        if (p.x, p.y, pw, ph) != (0, 0, W, H):
            what.append(f"placed {pw}x{ph} at {p.x},{p.y}")
        if c == 4:
            what.append("alpha blended over the base")
        placements.append(p)
        restored.append(", ".join(what))
    any_restored = any(r is not None for r in restored)
    stored = [(p, Version1Storage.load(p)) for p in args.marks]
    exceed = args.similarity_exceed
    # per suspect: (exact similarity or None, GEMM similarity, path, mark) of every stored mark, in file order per group
    rows: List[list] = [[] for _ in suspects]
    turned: Dict[int, str] = {}
    for (config, length), members in group_stored_marks(stored).items():   # main.rs:383-415, once per group for ALL suspects
        reader = Reader.base(base, config.to_read_config())
        if any_restored:
            res = reader.trace(suspects, [w.values for _, w in members], exceed, k=length, placements=placements, base=base)
            for s, f in res.turned.items():          # found once, with the first group; every later group is told the angle
                turned[s] = turned_text(f)
                placements[s] = Rotated(f.angle)
        else:
            res = reader.trace(suspects, [w.values for _, w in members], exceed, k=length)
        for s in range(len(suspects)):
            for j, (path, wmk) in enumerate(members):
                best = int(res.best[s]) == j
                rows[s].append((float(res.best_sim[s]) if best else None, float(res.sims[s][j]), path, wmk))
    for s, spath in enumerate(args.suspects):                            # the record of main.rs:418-429, per suspect
        exact = [r for r in rows[s] if r[0] is not None]
        top = max(exact, key=lambda r: r[0]) if exact else None
        print("-", file=out)
        print(f"  Suspect: \"{spath}\"", file=out)
        if spath in located:
            print(f"  Located: \"{located[spath]}\"", file=out)
        if s in turned:
            print(f"  Turned: \"{turned[s]}\"", file=out)
        if restored[s] is not None:
            print(f"  Restored: \"{restored[s]}\"", file=out)
        if top is None:
            print("  Matches: false", file=out)
            print(f"  MatchExceed: {_rust_f32(exceed)}", file=out)
            continue
        desc = top[3].description.replace('"', '\\"')
        print(f"  Matches: {'true' if top[0] > exceed else 'false'}", file=out)
        print(f"  Similarity: {_rust_f32(top[0])}", file=out)
        print(f"  MatchExceed: {_rust_f32(exceed)}", file=out)
        print(f"  Description: \"{desc}\"", file=out)
        print(f"  File: \"{top[2]}\"", file=out)
        for r in rows[s]:
            if r is not top and (r[0] if r[0] is not None else r[1]) > exceed:
                d = r[3].description.replace('"', '\\"')
                print(f"  Also: \"{d}\" ({_rust_f32(r[0] if r[0] is not None else r[1])}) in \"{r[2]}\"", file=out)
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    if args.command == "watermark":
        return cmd_watermark(args)
    if args.command == "test":
        return cmd_test(args)
    if args.command == "fingerprint":
        return cmd_fingerprint(args)
    if args.command == "trace":
        return cmd_trace(args)
    if args.command == "index":
        return cmd_index(args)
    if args.command == "identify":
        return cmd_identify(args)
    if args.command == "strength":
        return cmd_strength(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
