"""Watermark cut-outs from watermarked / clean pairs on the device: the reference's extract_watermarks.py.

Two library calls with a small host plan between them: extract_regions (uwm_extract_regions_ragged: difference mask, closing and
opening, fill, regions, polygon sums), plan_cutouts (centres, clustering, margins, names: pure Python over a few rows per image) and
extract_cutouts (uwm_extract_cutouts_ragged: RGBA crops through Pillow's Contrast / Sharpness / Brightness chain).  The files written
are transparent RGBA PNGs, which `--logos-dir` of `synth` and `train --synthesize` reads.  No CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
import os
import random

import numpy as np
import torch

from . import _lib as L
from .data import DESC_DTYPE, PAIR_IMAGE_EXTENSIONS, descs_tensor, device_resize, mask_descs_for, pack_images
from ._device import ptr, ragged_capacities, upload_records, workspace

MAX_REGIONS = 254                                          # UWM_EXTRACT_MAX_REGIONS: kept regions of one image
ROW_FIELDS = ("id", "a00", "a10", "a01", "x0", "y0", "x1", "y1", "pixels")
STATS_FIELDS = ("found", "kept", "status", "pixels")
STATUS_DONE, STATUS_MISFIT, STATUS_TOO_MANY = 0, 1, 2
EXTRACT_JOB_DTYPE = np.dtype([("image", "<i4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("reserved", "<i4"),
                              ("out_offset", "<i8"), ("member", "u1", (256,))])      # = uwm_extract_job, 288 bytes
_REFUSAL = "watermark extraction runs only on a HIP device (no CPU fallback): flat uint8 tensors on the device are needed"


def _device_flat(t):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or t.numel() == 0:
        raise RuntimeError(_REFUSAL)
    return t


def _descs(d, n=None):
    d = np.ascontiguousarray(d)
    if d.dtype != DESC_DTYPE or d.ndim != 1 or len(d) == 0 or (n is not None and len(d) != n):
        raise ValueError("expected a 1-D array of data.DESC_DTYPE" + (f" with {n} entries" if n is not None else ""))
    return d


def extract_regions(wm_buf, clean_buf, descs, threshold=30, min_area=100, clean_descs=None, plane_descs=None, max_pixels=None,
                    total_pixels=None):
    """Stage 1 for every pair of a ragged batch (uwm_extract_regions_ragged; the rule is in include/uwm.h).  wm_buf / clean_buf: flat
    uint8 device tensors of RGB images (pack_images) with their uwm_image_desc arrays (clean_descs: descs when absent).  -> (plane,
    plane_descs, stats, table): the flat uint8 plane with, per pixel, the index of the kept region or 255 (layout plane_descs, default
    mask_descs_for(descs)); stats int64 (N, 4) STATS_FIELDS; table int64 (N, 254, 9) ROW_FIELDS, kept regions in ascending id order.
    All on the device, nothing synchronised.  max_pixels / total_pixels: capacities, at least the largest and the sum of h*w."""
    t, a = int(threshold), int(min_area)
    if not 0 <= t <= 255:
        raise ValueError(f"extract_regions: threshold must be 0..255 (got {threshold})")
    if not 0 <= a <= 1 << 30:
        raise ValueError(f"extract_regions: min_area must be 0 .. 2^30 (got {min_area})")
    wm, cl = _device_flat(wm_buf), _device_flat(clean_buf)
    if cl.device != wm.device:
        raise RuntimeError(_REFUSAL)
    wd = _descs(descs)
    n = len(wd)
    cd = wd if clean_descs is None else _descs(clean_descs, n)
    pd = mask_descs_for(wd) if plane_descs is None else _descs(plane_descs, n)
    caps = ragged_capacities(wd)
    max_pixels = caps["max_pixels"] if max_pixels is None else int(max_pixels)
    total_pixels = caps["total_pixels"] if total_pixels is None else int(total_pixels)
    nplane = max(1, int((pd["offset"].astype(np.int64) + pd["h"].astype(np.int64) * pd["w"]).max()))
    plane = torch.full((nplane,), 255, dtype=torch.uint8, device=wm.device)
    stats = torch.empty((n, 4), dtype=torch.int64, device=wm.device)
    table = torch.empty((n, MAX_REGIONS, len(ROW_FIELDS)), dtype=torch.int64, device=wm.device)
    dd = descs_tensor(np.concatenate([wd, cd, pd]), wm.device)
    step = n * DESC_DTYPE.itemsize
    lib = L.lib()
    with L.on_device(wm):
        ws = workspace("extract", wm.device, lib.uwm_extract_workspace_bytes(n, total_pixels, 0), ValueError)
        L.check(lib.uwm_extract_regions_ragged(ptr(wm), wm.numel(), ptr(dd), ptr(cl), cl.numel(), C.c_void_p(dd.data_ptr() + step), n, 3, t, a,
                                               max_pixels, total_pixels, ptr(plane), plane.numel(), C.c_void_p(dd.data_ptr() + 2 * step),
                                               ptr(stats), ptr(table), ptr(ws), ws.numel(), C.c_void_p(L.stream_ptr(wm.device))), ValueError)
    return plane, pd, stats, table


def host_regions(stats, table):
    """The device results of extract_regions -> what plan_cutouts reads: per image (status, rows), rows the int (kept, 9) array"""
    s = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    tb = table.cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    return [(int(s[i, 2]), tb[i, :int(s[i, 1])] if int(s[i, 2]) == STATUS_DONE else tb[i, :0]) for i in range(len(s))]


def cluster_centres(centres, eps):
    """sklearn.cluster.DBSCAN(eps, min_samples=1).fit(centres).labels_, written directly: with min_samples = 1 every point is a core
    point, so the clusters are the connected components of the graph "distance <= eps", numbered by their first point.  The
    comparison is made on squares, d^2 <= eps*eps in float64, as the neighbour search does."""
    n = len(centres)
    labels = [-1] * n
    r2 = float(eps) * float(eps)
    k = 0
    for s in range(n):
        if labels[s] >= 0:
            continue
        labels[s] = k
        stack = [s]
        while stack:
            i = stack.pop()
            for j in range(n):
                if labels[j] < 0:
                    dx, dy = centres[i][0] - centres[j][0], centres[i][1] - centres[j][1]
                    if float(dx * dx + dy * dy) <= r2:
                        labels[j] = k
                        stack.append(j)
        k += 1
    return labels


def _crop(x0, y0, x1, y1, W, H, floor, share):
    """the reference's margins and clipping, literally: margins from the box's own size, x = max(0, x - mx), then w = min(W - x, w + 2*mx)
    (so a box near the left or top edge keeps both margins' worth of width although one of them was cut)"""
    w, h = x1 - x0 + 1, y1 - y0 + 1
    mx, my = max(floor, int(w * share)), max(floor, int(h * share))
    x, y = max(0, x0 - mx), max(0, y0 - my)
    return x, y, min(W - x, w + 2 * mx), min(H - y, h + 2 * my)


def plan_cutouts(stats, sizes, stems=None):
    """The host plan between the two device stages.  stats: per image (status, rows) as host_regions gives them, rows = the kept
    regions' table rows ROW_FIELDS in ascending id order; sizes: per image (h, w); stems: per image the file stem (default 'image{i}').
    -> per image a list of cut-outs dict(name, x, y, w, h, members): one region -> '{stem}_watermark.png' with margins max(20, 15 %);
    several -> their centres (a10 // (3*a00), a01 // (3*a00)) clustered at eps = a quarter of the diagonal; one cluster -> one combined
    '{stem}_watermark.png', several -> '{stem}_watermark_part{k}.png' per cluster, k from 1 in ascending order of each cluster's lowest
    region id, margins max(25, 12 %).  An image whose status is not 0, or without a kept region, gives an empty list."""
    plans = []
    for i, ((status, rows), (H, W)) in enumerate(zip(stats, sizes)):
        stem = f"image{i}" if stems is None else stems[i]
        rows = [[int(v) for v in r] for r in rows]
        if int(status) != STATUS_DONE or not rows:
            plans.append([])
            continue
        if len(rows) > MAX_REGIONS:
            raise ValueError(f"plan_cutouts: image {i} has {len(rows)} rows, more than {MAX_REGIONS}")
        H, W = int(H), int(W)
        if len(rows) == 1:
            r = rows[0]
            x, y, w, h = _crop(r[4], r[5], r[6], r[7], W, H, 20, 0.15)
            plans.append([dict(name=f"{stem}_watermark.png", x=x, y=y, w=w, h=h, members=[0])])
            continue
        centres = [(r[2] // (3 * r[1]), r[3] // (3 * r[1])) for r in rows]
        labels = cluster_centres(centres, math.sqrt(H * H + W * W) * 0.25)
        nclusters = max(labels) + 1
        cuts = []
        for k in range(nclusters):
            members = [j for j, lab in enumerate(labels) if lab == k]
            x, y, w, h = _crop(min(rows[j][4] for j in members), min(rows[j][5] for j in members), max(rows[j][6] for j in members),
                               max(rows[j][7] for j in members), W, H, 25, 0.12)
            name = f"{stem}_watermark.png" if nclusters == 1 else f"{stem}_watermark_part{k + 1}.png"
            cuts.append(dict(name=name, x=x, y=y, w=w, h=h, members=members))
        plans.append(cuts)
    return plans


def cutout_jobs(plans):
    """plan_cutouts' result -> (jobs, out_bytes): the EXTRACT_JOB_DTYPE records of every cut-out, image by image, their RGBA outputs
    back to back"""
    flat = [(i, c) for i, cuts in enumerate(plans) for c in cuts]
    jobs = np.zeros(len(flat), EXTRACT_JOB_DTYPE)
    off = 0
    for j, (i, c) in enumerate(flat):
        for f, v in (("image", i), ("x", c["x"]), ("y", c["y"]), ("w", c["w"]), ("h", c["h"]), ("out_offset", off)):
            jobs[f][j] = v
        jobs["member"][j, list(c["members"])] = 1
        off += int(c["w"]) * int(c["h"]) * 4
    return jobs, off


def extract_cutouts(wm_buf, descs, plane, plane_descs, jobs, out_bytes=None, max_crop_pixels=None):
    """Stage 2 (uwm_extract_cutouts_ragged): every job's crop of the watermarked image as RGBA, alpha 255 on the job's member regions
    of `plane`, through ImageEnhance.Contrast(1.3), Sharpness(1.4), Brightness(1.1) (bit for bit Pillow's).  jobs: EXTRACT_JOB_DTYPE
    records (cutout_jobs).  -> (out, status): the flat uint8 buffer with job j's w*h*4 bytes at its out_offset, int32 (J,) 0 done |
    1 misfit, both on the device."""
    wm, pl = _device_flat(wm_buf), _device_flat(plane)
    if pl.device != wm.device:
        raise RuntimeError(_REFUSAL)
    wd = _descs(descs)
    n = len(wd)
    pd = _descs(plane_descs, n)
    jb = np.ascontiguousarray(jobs)
    if jb.dtype != EXTRACT_JOB_DTYPE or jb.ndim != 1 or len(jb) == 0:
        raise ValueError("extract_cutouts: jobs must be a non-empty 1-D array of EXTRACT_JOB_DTYPE")
    area = np.clip(jb["w"].astype(np.int64), 0, None) * np.clip(jb["h"].astype(np.int64), 0, None)
    if out_bytes is None:
        out_bytes = int((jb["out_offset"].astype(np.int64) + 4 * area).max())
    max_crop_pixels = max(1, int(area.max())) if max_crop_pixels is None else int(max_crop_pixels)
    out = torch.zeros(max(4, int(out_bytes)), dtype=torch.uint8, device=wm.device)
    status = torch.empty(len(jb), dtype=torch.int32, device=wm.device)
    dd = descs_tensor(np.concatenate([wd, pd]), wm.device)
    dj = upload_records(jb, wm.device)
    lib = L.lib()
    with L.on_device(wm):
        ws = workspace("extract", wm.device, lib.uwm_extract_workspace_bytes(0, 0, len(jb)), ValueError)
        L.check(lib.uwm_extract_cutouts_ragged(ptr(wm), wm.numel(), ptr(dd), ptr(pl), pl.numel(), C.c_void_p(dd.data_ptr() + n * DESC_DTYPE.itemsize),
                                               n, ptr(dj), len(jb), max_crop_pixels, ptr(out), out.numel(), ptr(status), ptr(ws), ws.numel(),
                                               C.c_void_p(L.stream_ptr(wm.device))), ValueError)
    return out, status


def list_pairs(clean_dir, watermarked_dir):
    """-> sorted [(stem, clean path, watermarked path)]: files of the two folders matched by stem over the extensions the pair loaders
    accept (the reference globs *.jpg only); of several files with one stem the first in sorted order counts"""
    def by_stem(d):
        out = {}
        for f in sorted(os.listdir(d)):
            if f.lower().endswith(PAIR_IMAGE_EXTENSIONS):
                out.setdefault(os.path.splitext(f)[0], os.path.join(d, f))
        return out
    c, w = by_stem(clean_dir), by_stem(watermarked_dir)
    return [(s, c[s], w[s]) for s in sorted(set(c) & set(w))]


def sample_pairs(pairs, limit=None, seed=0):
    """--limit: a seeded sample (random.Random(seed).sample over the sorted pairs; the reference's draw is unseeded)"""
    if limit and int(limit) < len(pairs):
        return random.Random(f"uwm-extract:{int(seed)}").sample(pairs, int(limit))
    return list(pairs)


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class WatermarkExtractor:
    """The reference's WatermarkExtractor on the device.  process_all_images -> dict(processed, extracted, written, errors): pairs
    run, pairs that yielded cut-outs, files written, pairs that could not be read or did not fit (a side below 3, more than 254 kept
    regions)."""

    def __init__(self, clean_dir, watermarked_dir, output_dir, threshold=30, min_area=100, batch_size=16, device=None):
        self.clean_dir, self.watermarked_dir, self.output_dir = str(clean_dir), str(watermarked_dir), str(output_dir)
        self.threshold, self.min_area, self.batch_size = int(threshold), int(min_area), max(1, int(batch_size))
        if not 0 <= self.threshold <= 255:
            raise ValueError(f"threshold must be 0..255 (got {threshold})")
        if self.min_area < 0:
            raise ValueError(f"min_area must be >= 0 (got {min_area})")
        self.device = device

    def _stage(self, wms, cleans, device):
        """both images of every pair at one size on the device: a pair whose files differ is brought to (min h, min w) by
        uwm_resize_u8(LINEAR), each side that needs it, as the reference's cv2.resize does -> (wm buffer, clean buffer, descs)"""
        targets = [(min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])) for a, b in zip(wms, cleans)]
        bufs = []
        for arrs in (wms, cleans):
            host = [a if a.shape[:2] == t else np.zeros(t + (3,), np.uint8) for a, t in zip(arrs, targets)]
            packed, descs, _ = pack_images(host)
            buf = packed.to(device, non_blocking=True)
            for a, t, d in zip(arrs, targets, descs):
                if a.shape[:2] != t:
                    one, od, _ = pack_images([a])
                    o = int(d["offset"])
                    buf[o:o + t[0] * t[1] * 3] = device_resize(one.to(device), od, t, 3, "linear").reshape(-1)
            bufs.append(buf)
        return bufs[0], bufs[1], descs

    def process_all_images(self, limit=None, seed=0):
        from PIL import Image
        if not torch.cuda.is_available():
            raise RuntimeError("extract needs a HIP device (this path has no CPU fallback)")
        device = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        pairs = sample_pairs(list_pairs(self.clean_dir, self.watermarked_dir), limit, seed)
        os.makedirs(self.output_dir, exist_ok=True)
        res = dict(processed=0, extracted=0, written=0, errors=0)
        for b in range(0, len(pairs), self.batch_size):
            stems, wms, cleans = [], [], []
            for stem, cpath, wpath in pairs[b:b + self.batch_size]:
                try:
                    c, w = _read_rgb(cpath), _read_rgb(wpath)
                except Exception as e:                             # counted, stops nothing
                    res["errors"] += 1
                    print(f"{stem}: unreadable ({e.__class__.__name__})")
                    continue
                stems.append(stem); wms.append(w); cleans.append(c)
            if not stems:
                continue
            wm, clean, descs = self._stage(wms, cleans, device)
            plane, pdescs, stats, table = extract_regions(wm, clean, descs, self.threshold, self.min_area)
            regions = host_regions(stats, table)
            res["processed"] += len(stems)
            for stem, (status, _) in zip(stems, regions):
                if status != STATUS_DONE:
                    res["errors"] += 1
                    print(f"{stem}: skipped ({'more than 254 regions' if status == STATUS_TOO_MANY else 'a side below 3 pixels'})")
            plans = plan_cutouts(regions, [(int(d["h"]), int(d["w"])) for d in descs], stems)
            res["extracted"] += sum(1 for p in plans if p)
            jobs, nbytes = cutout_jobs(plans)
            if len(jobs) == 0:
                continue
            out, _ = extract_cutouts(wm, descs, plane, pdescs, jobs, nbytes)
            out = out.cpu().numpy()
            for j, c in zip(jobs, (c for cuts in plans for c in cuts)):
                o, w, h = int(j["out_offset"]), int(j["w"]), int(j["h"])
                Image.fromarray(out[o:o + w * h * 4].reshape(h, w, 4)).save(os.path.join(self.output_dir, c["name"]))
                res["written"] += 1
        return res
