"""Writes crop_answers.json: what the CPU oracle and the committed restatements answer for the crop rows of the strength report,
on the cat at 640 x 444 with k = 1000, marks from default_rng(3), copies 0 .. 2, Option2 / Energy, f64 backend -- the record
tests/test_crop_cpu.py checks itself against and tests/test_crop_gpu.py may read.
  "placed":  per rectangle and alpha the own-mark similarity of copies 0 .. 2 after the cut was laid over the original (the
             reference's tests/attack_crop.rs), the largest |similarity| with the innocent mark c + 3, and where `locate_ref`
             finds copy 0's piece
  "scaled":  per crop -> thumbnail case (copy 0, Pillow's BICUBIC) what `locate_scaled_ref` answers over the range, and per alpha
             the similarity with the piece laid where it was found and where it belongs
Run from the repository root (about a minute; the three ladders take 4 - 12 s each):
    python tests/golden/gen_crop_answers.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from oracle import oracle as O  # noqa: E402
from test_crop_cpu import ALPHAS, COPIES, K, PLACED, SCALED, cat_image, crop_ref, marks  # noqa: E402

RECORD = os.path.join(HERE, "crop_answers.json")


def marked_copies(alpha):
    rgb = O.u8_to_f32(cat_image())
    return [O.f32_to_u8(O.embed_frame(rgb, marks()[c], alpha=alpha)) for c in range(COPIES)]


def similarity(frame, c, alpha, which):
    ext, _ = O.extract_frame(O.u8_to_f32(cat_image()), O.u8_to_f32(frame), marks()[c], alpha=alpha)
    return float(O.similarity(ext, marks()[which]))


def measure():
    base = cat_image()
    copies = {alpha: marked_copies(alpha) for alpha in ALPHAS}
    placed, scaled = {}, {}
    for rect in PLACED:
        row = {}
        for alpha in ALPHAS:
            outs = [crop_ref(base, copies[alpha][c], rect).out for c in range(COPIES)]
            found = crop_ref(base, copies[alpha][0], rect, search=(0, 0)).found
            row[str(alpha)] = {"own": [round(similarity(o, c, alpha, c), 2) for c, o in enumerate(outs)],
                               "innocent": round(max(abs(similarity(o, c, alpha, c + 3)) for c, o in enumerate(outs)), 2),
                               "found": list(found)}
        placed["%d,%d,%dx%d" % rect] = row
    for rect, thumb, rng in SCALED:
        row = {}
        for alpha in ALPHAS:
            r = crop_ref(base, copies[alpha][0], rect, thumb, "bicubic", rng)
            p = crop_ref(base, copies[alpha][0], rect, thumb, "bicubic")
            row[str(alpha)] = {"found": list(r.found), "sad": r.sad, "sim_found": round(similarity(r.out, 0, alpha, 0), 2),
                               "sim_placed": round(similarity(p.out, 0, alpha, 0), 2)}
        scaled["%d,%d,%dx%d->%dx%d" % (rect + thumb)] = row
    return {"k": K, "copies": COPIES, "placed": placed, "scaled": scaled}


if __name__ == "__main__":
    with open(RECORD, "w") as f:
        json.dump(measure(), f, indent=1)
        f.write("\n")
