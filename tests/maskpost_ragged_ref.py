"""CPU restatement of the ragged mask post-processing's statistics and misfit rule (test-side only, numpy only), on top of
tests/maskpost_ref.py: the eight numbers per image that uwm_optimize_masks_ragged returns (include/uwm.h)."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ref as R  # noqa: E402

TYPES = R.MASK_TYPES + ("none",)
KEEP_ABOVE = {"text": 50, "mixed": 100, "none": 0}


def pre_selection(m, mask_type):
    """the plane whose components are selected: the type's morphology, or for 'none' the binarised plane itself"""
    return m.copy() if mask_type == "none" else R._chain(m, mask_type)


def kept_areas(areas, mask_type):
    """areas of all components (in id order) -> the areas of the kept ones: the keep rules of DESIGN.md §8b"""
    areas = np.asarray(areas, np.int64)
    if len(areas) == 0:
        return areas
    if mask_type == "watermark":
        return areas[areas > 200] if areas.max() < 500 else areas[[int(np.argmax(areas))]]
    return areas[areas > KEEP_ABOVE[mask_type]]


def optimize(mask_u8, mask_type):
    """uint8 (h, w) -> (uint8 {0,255} output, the stats row of 8 ints with status 0)"""
    m = np.asarray(mask_u8) > 127
    plane = pre_selection(m, mask_type)
    labels, areas = R.components(plane)
    flat = areas.reshape(-1)
    ids = np.nonzero(flat)[0]
    if mask_type == "none":
        out = plane
        summary = [len(ids), int(flat[ids].max()) if len(ids) else 0, int(plane.sum()), int(ids[np.argmax(flat[ids])]) if len(ids) else -1]
    else:
        out, summary = R._select(plane, mask_type)
    kept = kept_areas(flat[ids], mask_type)
    row = [int(v) for v in summary] + [len(kept), int(kept.max()) if len(kept) else 0, int(m.size), 0]
    return out.astype(np.uint8) * 255, row


MISFIT_ROW = [0, 0, 0, 0, 0, 0, 0, 1]


def misfits(descs, mask_bytes, max_pixels, rows):
    """-> bool per image: the misfit rule.  An image whose sides (1 .. 2^30), pixel count (<= max_pixels) and region (inside
    [0, mask_bytes)) are in order takes part in the running sums of rows and plane words; it is still a misfit when a sum up to and
    including its own exceeds `rows` or the plane's mask_bytes // 64 + rows words."""
    out, sum_rows, sum_words = [], 0, 0
    for d in descs:
        off, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
        ok = 1 <= h <= 2 ** 30 and 1 <= w <= 2 ** 30 and h * w <= max_pixels and 0 <= off <= mask_bytes - h * w
        if ok:
            sum_rows += h
            sum_words += h * ((w + 63) // 64)
            ok = sum_rows <= rows and sum_words <= mask_bytes // 64 + rows
        out.append(not ok)
    return out


# ------------------------------------------------------------------ stress planes for 'none' (65 x 130: one word and two bits wide, odd height)
def stress_planes(h=65, w=130):
    """-> {name: (bool plane, components, largest area)} with the hand-computed numbers for 65 x 130:
    checkerboard: every other pixel, joined diagonally into one component of 65 * 130 / 2 = 4225;
    comb: the top row and every other column below it: 130 + 65 * 64 = 4290;
    serpentine: every other row, joined alternately at the right and left end: 33 * 130 + 32 = 4322;
    isolated: the pixels with even y and even x, none touching another: 33 * 65 = 2145 components of area 1"""
    yy, xx = np.mgrid[:h, :w]
    checker = (yy + xx) % 2 == 0
    comb = (yy == 0) | (xx % 2 == 0)
    serp = yy % 2 == 0
    odd = yy % 2 == 1
    serp = serp | (odd & (yy % 4 == 1) & (xx == w - 1)) | (odd & (yy % 4 == 3) & (xx == 0))
    isolated = (yy % 2 == 0) & (xx % 2 == 0)
    planes = {"checkerboard": [checker, 1, None], "comb": [comb, 1, None], "serpentine": [serp, 1, None], "isolated": [isolated, None, 1]}
    if (h, w) == (65, 130):
        planes["checkerboard"][2], planes["comb"][2], planes["serpentine"][2], planes["isolated"][1] = 4225, 4290, 4322, 2145
    return {k: tuple(v) for k, v in planes.items()}
