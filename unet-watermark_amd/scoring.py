"""Scoring predicted masks against ground truth (include/uwm.h): thin host wrappers over uwm_score_masks_ragged in
csrc/mask_score.hip, which counts tp / fp / fn / tn and the three Boundary-IoU counts of a ragged batch of mask pairs on the
device, and the formulas that turn those counts into the reference's five metrics (src/utils/metrics.py::get_metrics) plus
Boundary IoU (Cheng et al., CVPR 2021).  Below them the surface distances: wrappers over uwm_edt_ragged and
uwm_surface_distances_ragged in csrc/mask_dist.hip, and the formulas that turn a record of squared distances into the Hausdorff
distance, HD95, ASSD and the covering radius.  No CPU fallback for the counting or the distances."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _device as D, _lib as L

COUNT_FIELDS = ("tp", "fp", "fn", "tn", "boundary_intersection", "boundary_pred", "boundary_truth", "status")
METRIC_FIELDS = ("iou", "f1", "accuracy", "recall", "precision", "boundary_iou")
MAX_RADIUS = 32767


def boundary_radius(h: int, w: int, ratio: float = 0.02) -> int:
    """Boundary IoU's dilation distance for an h x w image: `ratio` of the diagonal, at least 1 (the paper's mask_to_boundary:
    29 at 720 x 1280, 88 at 2160 x 3840)."""
    return max(1, int(round(float(ratio) * math.sqrt(int(h) * int(h) + int(w) * int(w)))))


def score_workspace(device, n: int, mask_bytes: int, rows: int):
    """The score call's scratch for the capacities (n, mask_bytes, rows): one buffer per device, kept and grown like
    postprocess.ragged_workspace; a captured graph holds the buffer it was captured with."""
    return D.workspace("score", device, L.lib().uwm_score_masks_workspace_bytes(int(n), int(mask_bytes), int(rows)))


def score_masks_ragged(pred, truth, descs, radii, *, n: Optional[int] = None, max_pixels: Optional[int] = None,
                       rows: Optional[int] = None, out=None):
    """A ragged batch of mask pairs through ONE library call (uwm_score_masks_ragged).  pred, truth: uint8 1-d device tensors of
    the same size; pair i is descs[i]'s (h, w), one byte per pixel, at [descs[i].offset:] of both, binarised as > 127 (pred may be
    truth).  descs: a host record array with the fields offset / h / w (uploaded here), or a device tensor of uwm_image_desc bytes
    — then n, max_pixels and rows must be given, nothing about the batch is read on the host, and the call can be captured.
    radii: the Boundary-IoU distance of every pair (0 .. 32767; 0: no boundary counts), a host sequence or an int32 device tensor.
    -> the int64 (n, 8) device tensor COUNT_FIELDS (`out`: a tensor to write them into).  max_pixels / rows: capacities, at least
    the largest h*w and the sum of h; a pair beyond a capacity is a misfit (status 1, zeros)."""
    d, n, caps = D.ragged_args("score_masks_ragged", (pred, truth), descs, n, max_pixels=max_pixels, rows=rows)
    mask_bytes = min(pred.numel(), truth.numel())
    if isinstance(radii, torch.Tensor):
        if radii.device != pred.device or radii.dtype != torch.int32 or radii.numel() < int(n) or not radii.is_contiguous():
            raise RuntimeError("score_masks_ragged: radii must be a contiguous int32 tensor of n entries on the buffers' device")
        r = radii
    else:
        host = np.ascontiguousarray(np.asarray(radii, dtype=np.int64).reshape(-1))
        if host.size != int(n):
            raise ValueError(f"score_masks_ragged: {host.size} radii for {n} pairs")
        r = torch.from_numpy(host.clip(-1, 2 ** 31 - 1).astype(np.int32)).to(pred.device)
    out = D.stats_like("score_masks_ragged", out, n, 8, pred.device, what="out")
    with L.on_device(pred):
        ws = score_workspace(pred.device, n, mask_bytes, caps["rows"])
        L.check(L.lib().uwm_score_masks_ragged(D.ptr(pred), D.ptr(truth), mask_bytes, D.ptr(d), D.ptr(r), n, caps["max_pixels"], caps["rows"],
                                               D.ptr(out), D.ptr(ws), ws.numel(), C.c_void_p(L.stream_ptr(pred.device))))
    return out


def _ratio(num: float, den: float) -> float:
    return float(num) / float(den) if den else 1.0


def metrics_from_counts(row) -> dict:
    """One COUNT_FIELDS row (or a sum of rows) -> {iou, f1, accuracy, recall, precision, boundary_iou}.  The first five are
    segmentation_models_pytorch's formulas as the reference's get_metrics calls them (iou_score, f1_score, accuracy, recall,
    precision), restated here, not run: smp is not installed with this project.
        iou = tp / (tp + fp + fn)      f1 = 2 tp / (2 tp + fp + fn)      accuracy = (tp + tn) / (tp + fp + fn + tn)
        recall = tp / (tp + fn)        precision = tp / (tp + fp)        boundary_iou = c4 / (c5 + c6 - c4)
    0 / 0 gives 1.0: smp's default zero_division = 1.0, which get_metrics does not override."""
    tp, fp, fn, tn, bi, bp, bt = (int(v) for v in list(row)[:7])
    return {"iou": _ratio(tp, tp + fp + fn), "f1": _ratio(2 * tp, 2 * tp + fp + fn), "accuracy": _ratio(tp + tn, tp + fp + fn + tn),
            "recall": _ratio(tp, tp + fn), "precision": _ratio(tp, tp + fp), "boundary_iou": _ratio(bi, bp + bt - bi)}


def summarize(counts) -> dict:
    """(n, 8) COUNT_FIELDS rows -> {"micro": the formulas on the counts summed over the images (the reference's
    reduction="micro" over a batch), "imagewise": the mean over the images of each image's own values}.  Misfit rows (status != 0)
    are left out; with no rows left every value is 1.0, as 0 / 0 is above."""
    rows = np.asarray(counts, dtype=np.int64).reshape(-1, 8)
    rows = rows[rows[:, 7] == 0]
    micro = metrics_from_counts([int(v) for v in rows[:, :7].sum(axis=0)] if len(rows) else [0] * 7)
    each = [metrics_from_counts(r) for r in rows]
    imagewise = {k: (float(sum(m[k] for m in each) / len(each)) if each else 1.0) for k in METRIC_FIELDS}
    return {"micro": micro, "imagewise": imagewise}


# ---------------------------------------------------------------- surface distances (csrc/mask_dist.hip)
SURFACE_FIELDS = ("border_pred", "border_truth", "hd_d2_pred", "hd_d2_truth", "p95_d2_lo", "p95_d2_hi", "p95_rem", "cover_d2", "defined",
                  "status")
EDT_NONE = 2 ** 31 - 1                                    # UWM_EDT_NONE: D2 of an image without a set pixel
MAX_SIDE = 32768


def _dist_workspace(device, call: str, n: int, mask_bytes: int, rows: int):
    """the scratch of uwm_edt_ragged ('edt') or uwm_surface_distances_ragged ('surface_distances'), kept and grown like score_workspace"""
    return D.workspace(call, device, getattr(L.lib(), f"uwm_{call}_workspace_bytes")(int(n), int(mask_bytes), int(rows)))


def distance_transform_ragged(masks, descs, *, n: Optional[int] = None, max_pixels: Optional[int] = None, rows: Optional[int] = None,
                              out=None):
    """The exact squared Euclidean distance transform of a ragged batch of masks through ONE library call (uwm_edt_ragged).  masks: a
    uint8 1-d device tensor; image i is descs[i]'s (h, w), one byte per pixel, at [descs[i].offset:], binarised as > 127.  descs: as
    score_masks_ragged takes them (host records, or a device tensor with n, max_pixels and rows).  -> an int32 device tensor of
    masks.numel() entries: D2 of image i's pixel k at [descs[i].offset + k], 0 on set pixels, EDT_NONE throughout an image without
    one; entries no image covers, and those of a misfit (a side above 32768, a pair beyond a capacity), are not written (`out`: a
    tensor to write into; a fresh one is zero-filled)."""
    d, n, caps = D.ragged_args("distance_transform_ragged", (masks,), descs, n, max_pixels=max_pixels, rows=rows)
    mask_bytes = masks.numel()
    if out is None:
        out = torch.zeros(mask_bytes, dtype=torch.int32, device=masks.device)
    elif out.dtype != torch.int32 or out.device != masks.device or out.numel() < mask_bytes or not out.is_contiguous():
        raise RuntimeError("distance_transform_ragged: out must be a contiguous int32 tensor of masks.numel() entries on the masks' device")
    with L.on_device(masks):
        ws = _dist_workspace(masks.device, "edt", n, mask_bytes, caps["rows"])
        L.check(L.lib().uwm_edt_ragged(D.ptr(masks), mask_bytes, D.ptr(d), n, caps["max_pixels"], caps["rows"], D.ptr(out), D.ptr(ws), ws.numel(),
                                       C.c_void_p(L.stream_ptr(masks.device))))
    return out


def surface_distances_ragged(pred, truth, descs, *, n: Optional[int] = None, max_pixels: Optional[int] = None, rows: Optional[int] = None,
                             out=None):
    """The surface distances of a ragged batch of mask pairs through ONE library call (uwm_surface_distances_ragged): the buffers and
    descriptors of score_masks_ragged (pred may be truth) -> (records, sums): the int64 (n, 10) device tensor SURFACE_FIELDS and the
    float64 (n, 2) device tensor of the sums of sqrt over the two border-distance lists (`out`: a pair of tensors to write them
    into).  surface_from_record / summarize_surface turn them into Hausdorff, HD95, ASSD and the covering radius."""
    d, n, caps = D.ragged_args("surface_distances_ragged", (pred, truth), descs, n, max_pixels=max_pixels, rows=rows)
    mask_bytes = min(pred.numel(), truth.numel())
    out = (None, None) if out is None else out
    records = D.stats_like("surface_distances_ragged", out[0], n, 10, pred.device, what="out[0]")
    sums = D.stats_like("surface_distances_ragged", out[1], n, 2, pred.device, torch.float64, what="out[1]")
    with L.on_device(pred):
        ws = _dist_workspace(pred.device, "surface_distances", n, mask_bytes, caps["rows"])
        L.check(L.lib().uwm_surface_distances_ragged(D.ptr(pred), D.ptr(truth), mask_bytes, D.ptr(d), n, caps["max_pixels"], caps["rows"],
                                                     D.ptr(records), D.ptr(sums), D.ptr(ws), ws.numel(), C.c_void_p(L.stream_ptr(pred.device))))
    return records, sums


SURFACE_KEYS = ("hd", "hd95", "assd", "asd_pred_to_truth", "asd_truth_to_pred", "cover_radius")


def surface_from_record(row, sums) -> dict:
    """One SURFACE_FIELDS row and its two sums -> {hd, hd95, assd, asd_pred_to_truth, asd_truth_to_pred, cover_radius}, in pixels:
        hd = sqrt(max(hd_d2_pred, hd_d2_truth))          hd95 = sqrt(lo) + (sqrt(hi) - sqrt(lo)) * rem / 100
        asd_pred_to_truth = sums[0] / border_pred         asd_truth_to_pred = sums[1] / border_truth       assd = their mean
        cover_radius = ceil(sqrt(cover_d2)): the radius of the smallest Euclidean disc dilation of the prediction that covers the truth
    hd95 is numpy's linear 95th percentile of the two border-distance lists together (MedPy's hd95).  Both masks empty: every
    value is 0.  Exactly one empty (defined == 0): the four distances are None; cover_radius is 0 when the truth is the empty one
    and None when the prediction is.  A misfit row (status != 0): every value None."""
    r = [int(v) for v in list(row)[:10]]
    bp, bt, hp, ht, lo, hi, rem, cover, defined, status = r
    out = dict.fromkeys(SURFACE_KEYS)
    if status != 0:
        return out
    out["cover_radius"] = None if cover < 0 else int(math.isqrt(cover - 1) + 1 if cover > 0 else 0)
    if not defined:
        return out
    if bp == 0 and bt == 0:
        out.update(hd=0.0, hd95=0.0, assd=0.0, asd_pred_to_truth=0.0, asd_truth_to_pred=0.0)
        return out
    sa, sb = (float(v) for v in list(sums)[:2])
    out["hd"] = math.sqrt(max(hp, ht))
    out["hd95"] = math.sqrt(lo) + (math.sqrt(hi) - math.sqrt(lo)) * rem / 100
    out["asd_pred_to_truth"], out["asd_truth_to_pred"] = sa / bp, sb / bt
    out["assd"] = (out["asd_pred_to_truth"] + out["asd_truth_to_pred"]) / 2
    return out


def summarize_surface(records, sums) -> dict:
    """(n, 10) SURFACE_FIELDS rows and their (n, 2) sums -> {"images": the defined pairs, "undefined": the pairs with exactly one empty
    mask, "imagewise": the means of hd, hd95, assd and cover_radius over the defined pairs, "worst": the maxima of hd and
    cover_radius over them}.  Misfit rows are left out; with no defined pair the means and maxima are None."""
    rows = np.asarray(records, dtype=np.int64).reshape(-1, 10)
    sm = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    keep = rows[:, 9] == 0
    rows, sm = rows[keep], sm[keep]
    each = [surface_from_record(r, s) for r, s in zip(rows, sm) if int(r[8])]
    names = ("hd", "hd95", "assd", "cover_radius")
    return {"images": len(each), "undefined": int(len(rows) - len(each)),
            "imagewise": {k: (float(sum(m[k] for m in each) / len(each)) if each else None) for k in names},
            "worst": {k: (type(each[0][k])(max(m[k] for m in each)) if each else None) for k in ("hd", "cover_radius")}}
