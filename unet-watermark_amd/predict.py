"""Batched mask prediction — counterpart of WatermarkPredictor._load_unet_model / predict_mask /
step1_batch_predict_watermark_masks (/root/reference/src/predict.py:68-99,303-368,560-664) for the model
part of that path: checkpoint -> eval() -> logits -> threshold -> uint8 mask.  The reference runs batch 1
per image; here a whole batch goes through ONE hipGraph replay of the eval forward (BASELINE config 5).
The reference's mask post-processing (_optimize_mask, src/predict.py:161-301) is opt-in through `mask_type` and runs on the
device inside the same graph (postprocess.py); its image enhancement for text watermarks (_enhance_text_features,
src/predict.py:370-404) is opt-in through `text_enhance` and runs in front of the forward inside the same graph (textenh.py); its
`repair` is served by remove_watermarks with the membrane fill of inpaint.py behind the prediction; its automatic type
detection, IOPaint / LaMa, OCR and diffusion models stay out of scope."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .checkpoint import load_checkpoint
from .config import get_cfg_defaults, update_config
from .constants import IMAGENET_MEAN, IMAGENET_STD  # noqa: F401   (predict.IMAGENET_MEAN is part of this module's surface)
from .data import descs_tensor, device_preprocess, pack_images
from .metrics import threshold_mask
from .model import create_model_from_config
from ._device import ragged_views, recording
from .textenh import text_enhance_ragged
from .tta import view_mask
from .postprocess import RAGGED_TYPES, mask_type_code, optimize_mask, optimize_masks_ragged

# the groups of captured graphs, by what a graph replays on beside the model's arena (WatermarkPredictor._drop): a cloned input of its
# own; the staging buffers; those and the enhanced images; the same under test-time augmentation; the staging buffers and the tile tables
GRAPH_GROUPS = ("input", "images", "text", "tta", "tiled")


class WatermarkPredictor:
    def __init__(self, model_path: Optional[str] = None, config_path: Optional[str] = None, config=None,
                 device: str = "cuda", model=None, precision: Optional[str] = None, freeze: bool = False):
        """freeze=True: the weights are frozen after loading (model.freeze): BatchNorm scale / shift and filter banks are made once
        instead of in every forward, logits unchanged bit for bit; the arena is re-made when a new graph shape selects other bank
        forms."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("WatermarkPredictor runs only on a HIP device (no CPU fallback)")
        self.cfg = config if config is not None else get_cfg_defaults()
        if config_path:
            update_config(self.cfg, config_path)
        self.model = model if model is not None else create_model_from_config(self.cfg)
        if model_path:
            load_checkpoint(model_path, self.model)
        self.model.to(self.device).eval()
        if precision is not None:
            # "f16x3": the 3x3 convolutions on the fp16x3 kernels (fp32-class accuracy).  The fill threshold is dropped to 1 so that
            # the kernel choice does not depend on the batch size: an image's logits stay bit-identical whatever batch it rides in
            self.model.set_precision(precision, min_workgroups=1 if precision.startswith("f16x3") else None)
        self.threshold = float(self.cfg.PREDICT.THRESHOLD)
        # slot -> entry(key, graph, static, out, keep, group) of every captured graph (_captured).  One entry per kind for 'logits',
        # 'mask', 'mask_u8', 'images', 'images_post' (with a mask_type), 'text_images', 'text_images_post' (the same two with
        # text_enhance: graphs of their own, so the default ones stay as captured) and 'counts', where a new key replaces the graph;
        # one entry per key under ('tiled', key) and ('tta', key)
        self._graphs = {}
        self._ibuf = self._idesc = self._mdesc = self._mbuf = None      # predict_images' static staging buffers
        self._ebuf = None                     # text_enhance: the enhanced images, a second staging buffer of _ibuf's size
        self._caps = {}                       # the capacities captured ragged calls were given, grown geometrically (_capacity)
        self._merged = None                   # tta: the merged logit planes (n, IMG_SIZE, IMG_SIZE) of the last such call
        self._xtiles = self._xplans = self._xlbuf = None      # predict_images_tiled's static tile table, per-image plans and ragged logit plane
        self._gtbuf = None                    # score_images: the staged ground-truth masks, under _mbuf's descriptors
        self._hbuf = self._hevt = None        # pinned host staging of the packed bytes + the event of its last upload
        self.freeze = bool(freeze)
        if self.freeze:
            self.model.freeze()               # the first forward fixes the bank forms

    # --- input contract of dataset.get_val_transform: Resize -> Normalize(ImageNet) -> NCHW fp32
    def preprocess(self, images_u8_nhwc: torch.Tensor) -> torch.Tensor:
        return device_preprocess(images_u8_nhwc.to(self.device, non_blocking=True))      # one kernel: uint8 HWC -> normalised NCHW fp32

    @torch.no_grad()
    def logits(self, x: torch.Tensor, use_graph: bool = True) -> torch.Tensor:
        """x (N,3,H,W) fp32 on the device -> logits (N,1,H,W).  With use_graph the eval forward of this
        batch shape is captured once into a hipGraph and replayed (static input/output buffers)."""
        if not use_graph:
            return self.model(x)
        e = self._captured("logits", tuple(x.shape), (x.shape[0], x.shape[2], x.shape[3]), lambda st: self.model(st["x"]),
                           lambda: {"x": x.clone()}, "input")
        e.static["x"].copy_(x)
        e.graph.replay()
        return e.out

    @torch.no_grad()
    def predict_mask(self, x: torch.Tensor, apply_sigmoid: bool = False, use_graph: bool = True, mask_type: Optional[str] = None) -> torch.Tensor:
        """-> uint8 {0,255} (N,H,W); default reproduces predict.py:624 (raw logits > THRESHOLD).  mask_type 'watermark' | 'text' |
        'mixed': the reference's _optimize_mask on that mask (predict.py:357-362), inside the same captured graph."""
        if mask_type is None:
            return threshold_mask(self.logits(x, use_graph), self.threshold, apply_sigmoid)
        mask_type_code(mask_type)
        run = lambda t: optimize_mask(threshold_mask(self.model(t), self.threshold, apply_sigmoid), mask_type)
        if not use_graph:
            return run(x)
        e = self._captured("mask", (tuple(x.shape), bool(apply_sigmoid), mask_type), (x.shape[0], x.shape[2], x.shape[3]),
                           lambda st: run(st["x"]), lambda: {"x": x.clone()}, "input")
        e.static["x"].copy_(x)
        e.graph.replay()
        return e.out

    def _captured(self, slot, key, shape, run, statics=dict, group="images"):
        """the entry of `slot`, captured now when the slot is empty or holds another key: the arena re-made for the forward batch
        `shape` = (n, h, w) where it must be, the static tensors allocated (`statics`() -> dict), one eager run(static) as warm-up (it
        plans the workspaces and sets kernel attributes), then the capture of run(static), whose result is the entry's `out`.  `keep`
        pins what the graph replays on beside the statics: the model's workspaces and every workspace the store handed out during
        warm-up and capture.  The caller copies its inputs into entry.static and replays entry.graph."""
        e = self._graphs.get(slot)
        if e is None or e.key != key:
            self._refreeze_for(*shape)
            static = statics()
            with recording() as used:
                run(static)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = run(static)
            keep = (self.model._ws, getattr(self.model, "_filter_ws", None), *used)
            e = self._graphs[slot] = SimpleNamespace(key=key, graph=g, static=static, out=out, keep=keep, group=group)
        return e

    def _drop(self, *groups):
        """the captured graphs of `groups` (GRAPH_GROUPS) go: what they replay on was replaced"""
        self._graphs = {slot: e for slot, e in self._graphs.items() if e.group not in groups}

    def _capacity(self, name: str, need: int, limit: int) -> int:
        """the capacity `name` of the captured ragged calls covers `need`: kept, and grown geometrically up to `limit` when it does not;
        the capacities are in the graphs' keys, so a batch that fits them replays and one that exceeds one re-captures"""
        have = self._caps.get(name, 0)
        if have < need:
            have = self._caps[name] = min(max(need, 2 * have), limit)
        return have

    def _refreeze_for(self, n: int, h: int, w: int):
        """freeze=True: a new graph shape whose bank forms differ from the frozen ones gets the arena re-made for it; the graphs
        captured on the old arena contents go."""
        if self.freeze and not self.model.frozen_serves(n, h, w):
            self.model.freeze(batch_shape=(n, h, w))
            self._drop(*GRAPH_GROUPS)

    @torch.no_grad()
    def predict_mask_u8(self, images_u8_nhwc: torch.Tensor, out_size=None, apply_sigmoid: bool = False,
                        use_graph: bool = True, mask_type: Optional[str] = None, return_summary: bool = False):
        """uint8 (N,H,W,3) images -> uint8 {0,255} masks (N,out_h,out_w) through ONE library call (uwm_predict_u8): ImageNet
        Normalize written straight into the forward's input layout, eval forward, resize to `out_size` (default: the input
        size) + threshold.  Same masks as preprocess -> predict_mask / resize_threshold, bit for bit.
        mask_type 'watermark' | 'text' | 'mixed': the reference's _optimize_mask (uwm_optimize_mask) on the resized, thresholded
        mask, in place and inside the same captured graph; return_summary then adds the int64 (N,4) device tensor {components,
        largest area, foreground pixels, id of the largest or -1} (the reference's watermark_ratio / "no watermark found" test,
        src/predict.py:636-645, without copying the mask back).  mask_type=None: the masks as they were, untouched."""
        x = images_u8_nhwc.to(self.device, non_blocking=True)
        if mask_type is None:
            if return_summary:
                raise ValueError("return_summary needs a mask_type ('watermark', 'text' or 'mixed')")
            run = lambda t: self.model.predict_u8(t, IMAGENET_MEAN, IMAGENET_STD, self.threshold, apply_sigmoid, out_size)
        else:
            mask_type_code(mask_type)

            def run(t):
                m = self.model.predict_u8(t, IMAGENET_MEAN, IMAGENET_STD, self.threshold, apply_sigmoid, out_size)
                return optimize_mask(m, mask_type, return_summary=True, out=m)
        pick = (lambda r: r) if mask_type is None or return_summary else (lambda r: r[0])
        if not use_graph:
            return pick(run(x))
        key = (tuple(x.shape), None if out_size is None else tuple(out_size), bool(apply_sigmoid)) + (() if mask_type is None else (mask_type,))
        e = self._captured("mask_u8", key, x.shape[:3], lambda st: run(st["x"]), lambda: {"x": x.clone()}, "input")
        e.static["x"].copy_(x)
        e.graph.replay()
        return pick(e.out)

    def _staging(self, name: str, need: int):
        """the static device buffer `name` holds at least `need` bytes; grown geometrically.  A graph captured on the old buffer
        goes with it."""
        buf = getattr(self, name)
        if buf is not None and buf.numel() >= need:
            return
        cap = max(need, 256 if buf is None else 2 * buf.numel())
        setattr(self, name, torch.zeros(cap, dtype=torch.uint8, device=self.device))
        self._drop("images", "text", "tta", "tiled")

    def _stage_images(self, images):
        """pack `images` into the static staging buffers (_ibuf, _idesc, _mdesc; _mbuf sized for their masks) -> (n, IMG_SIZE, descs,
        mask descs, areas, mask bytes)"""
        # pack into ONE persistent pinned buffer (pinned allocation is expensive), grown geometrically; the previous batch's upload
        # from it must have finished before it is overwritten
        need = sum((int(np.prod(im.shape)) + 3) // 4 * 4 for im in images)
        if self._hbuf is None or self._hbuf.numel() < need:
            self._hbuf = torch.empty(max(need, 2 * (0 if self._hbuf is None else self._hbuf.numel())), dtype=torch.uint8, pin_memory=True)
        elif self._hevt is not None:
            self._hevt.synchronize()
        packed, descs, mdescs = pack_images(images, out=self._hbuf)
        channels = int(images[0].shape[2])
        if channels != self.model.in_channels:
            raise RuntimeError(f"the model takes {self.model.in_channels}-channel images, got {channels}")
        n, s = len(descs), int(self.cfg.DATA.IMG_SIZE)
        areas = descs["h"].astype("int64") * descs["w"]
        mask_bytes = int(mdescs["offset"][-1] + areas[-1])
        for name, need in (("_ibuf", packed.numel()), ("_idesc", 16 * n), ("_mdesc", 16 * n), ("_mbuf", mask_bytes)):
            self._staging(name, need)
        self._ibuf[:packed.numel()].copy_(packed, non_blocking=True)
        if self._hevt is None:
            self._hevt = torch.cuda.Event()
        self._hevt.record()
        self._idesc[:16 * n].copy_(descs_tensor(descs))
        self._mdesc[:16 * n].copy_(descs_tensor(mdescs))
        return n, s, descs, mdescs, areas, mask_bytes

    def _run_images(self, images, apply_sigmoid: bool, mask_type: Optional[str], use_graph: bool, text_enhance: bool = False, views: int = 1):
        """stage `images`, run uwm_predict_images_u8 and, with a mask_type, uwm_optimize_masks_ragged in place on _mbuf — one captured
        graph for both -> (descs, mask descs, areas, mask bytes, the int64 (n, 8) device stats or None).  The ragged call's
        capacities (the largest h*w, the sum of h) are kept and grown geometrically like the staging buffers; they and the buffer
        sizes are all the graph knows about a batch, so a batch that fits them replays it and one that exceeds one re-captures.
        text_enhance: the staged images first go through uwm_text_enhance_ragged into a second staging buffer (_ebuf), which the
        forward then reads — the same graph, kept in slots of its own, with the enhancement's two capacities (the largest h*w, the
        sum of h*w) in its key.
        views != 1 (a tta.view_mask): uwm_predict_images_tta_u8 in place of uwm_predict_images_u8, PREDICT.BATCH_SIZE slots per forward;
        its graphs have a slot each, ('tta', the plain call's key + (mask, batch)), with the static stats and the merged logit planes
        (n, IMG_SIZE, IMG_SIZE) of the graph in the entry; `_merged` is the latter after the call."""
        n, s, descs, mdescs, areas, mask_bytes = self._stage_images(images)
        batch = int(self.cfg.PREDICT.BATCH_SIZE)
        tcaps = ()
        if text_enhance:
            if self.model.in_channels != 3:
                raise RuntimeError(f"text_enhance takes RGB images; the model takes {self.model.in_channels} channels")
            if int(areas.max()) > 2 ** 30:
                raise ValueError("text_enhance: an image of more than 2^30 pixels")
            tcaps = ("text_enhance", self._capacity("text_pixels", int(areas.max()), 2 ** 30), self._capacity("text_total", int(areas.sum()), 2 ** 40))
            if self._ebuf is None or self._ebuf.numel() != self._ibuf.numel():
                self._ebuf = torch.zeros_like(self._ibuf)
                self._drop("text", "tta")
        caps = () if mask_type is None else (mask_type,) + self._mask_capacities(descs, areas)

        def run(static):
            if text_enhance:
                text_enhance_ragged(self._ibuf, self._idesc, out=self._ebuf, n=n, max_pixels=tcaps[1], total_pixels=tcaps[2])
            if views != 1:
                self.model.predict_images_tta_u8(self._ebuf if text_enhance else self._ibuf, self._idesc, self._mdesc, self._mbuf, n, batch,
                                                 (s, s), views, IMAGENET_MEAN, IMAGENET_STD, self.threshold, apply_sigmoid)
            else:
                self.model.predict_images_u8(self._ebuf if text_enhance else self._ibuf, self._idesc, self._mdesc, self._mbuf, n, (s, s),
                                             IMAGENET_MEAN, IMAGENET_STD, self.threshold, apply_sigmoid)
            if mask_type is not None:
                optimize_masks_ragged(self._mbuf, self._mdesc, mask_type, True, out=self._mbuf, n=n, max_pixels=caps[1], rows=caps[2],
                                      stats=static["stats"])
            return self.model._merged_store if views != 1 else None

        def statics():
            return {"stats": torch.empty((n, 8), dtype=torch.int64, device=self.device)} if mask_type is not None else {}
        key = (n, s, s, bool(apply_sigmoid), float(self.threshold)) + caps + tcaps      # (the threshold and the capacities are captured arguments)
        if not use_graph:
            static = statics()
            merged = run(static)
        else:
            if views != 1:
                key += ("tta", views, batch)
                e = self._captured(("tta", key), key, (batch, s, s), run, statics, "tta")
            else:                                     # (the graph without post-processing stays when the other is captured)
                slot = ("text_images" if text_enhance else "images") + ("" if mask_type is None else "_post")
                e = self._captured(slot, key, (n, s, s), run, statics, "text" if text_enhance else "images")
            e.graph.replay()
            static, merged = e.static, e.out
        if views != 1:
            self._merged = merged
        return descs, mdescs, areas, mask_bytes, static.get("stats")

    def _mask_capacities(self, descs, areas):
        """-> the capacities (max_pixels, rows) a captured uwm_optimize_masks_ragged gets for this batch: the largest h*w, the sum of h"""
        return (self._capacity("pixels", int(areas.max()), 2 ** 31 - 2), self._capacity("rows", int(descs["h"].astype("int64").sum()), 2 ** 40))

    def _mask_views(self, mdescs, mask_bytes):
        return ragged_views(self._mbuf[:mask_bytes].clone(), mdescs)      # (the staging buffer is overwritten by the next call)

    @torch.no_grad()
    def predict_images(self, images, apply_sigmoid: bool = False, mask_type: Optional[str] = None, use_graph: bool = True,
                       return_stats: bool = False, text_enhance: bool = False, tta=None, return_logits: bool = False):
        """uint8 (h_i, w_i, C) images of ANY sizes (arrays or tensors) -> a list of uint8 {0,255} device masks, one per image at its
        own size: the reference's predict path (src/predict.py:327-335,614-625) device-resident from the image bytes on — cv2's
        INTER_LINEAR resize to IMG_SIZE (A.Resize) + Normalize, eval forward, bilinear resize of the logits back to (h_i, w_i) +
        threshold, in ONE library call (uwm_predict_images_u8).  The per-image geometry lives in device memory, so one captured
        graph per (N, IMG_SIZE, apply_sigmoid) serves every batch of N images; it is re-captured only when a staging buffer had
        to grow or the frozen arena was re-made.  mask_type 'watermark' | 'text' | 'mixed': every mask then goes through the
        reference's _optimize_mask at its own size (uwm_optimize_masks_ragged), in place and inside the same graph; the graph is
        then also re-captured when the largest image or the sum of the heights outgrows the capacity it was captured with.
        return_stats (needs a mask_type): also the int64 (N, 8) HOST array of postprocess.STATS_FIELDS.
        text_enhance: every image first goes through the reference's _enhance_text_features at its own size
        (uwm_text_enhance_ragged, textenh.py) and the network sees the enhanced image; an image with a side below 16 goes in as it
        is.  Independent of mask_type: mask_type='text', text_enhance=True is the reference's predict_text_watermark_mask.
        tta 'hflip' | 'flips' | 'd4' or a view mask (tta.view_mask): test-time augmentation — the network sees every (enhanced,
        resized) image under each view of the set, PREDICT.BATCH_SIZE network inputs per forward, and the logit planes are mapped
        back and averaged on the device before the resize back (uwm_predict_images_tta_u8; the mean of the LOGITS);
        one graph per view mask beside the others.  None / 'none': the call as it is without it.  return_logits (needs tta): also
        the float32 (N, IMG_SIZE, IMG_SIZE) device tensor of merged logits, last in the result."""
        views = view_mask(tta)
        if mask_type is not None:
            mask_type_code(mask_type)
        elif return_stats:
            raise ValueError("return_stats needs a mask_type ('watermark', 'text' or 'mixed')")
        if return_logits and views == 1:
            raise ValueError("return_logits needs tta ('hflip', 'flips', 'd4' or a view mask other than 1)")
        descs, mdescs, areas, mask_bytes, stats = self._run_images(images, apply_sigmoid, mask_type, use_graph, text_enhance, views)
        masks = self._mask_views(mdescs, mask_bytes)
        out = (masks, stats.cpu().numpy()) if return_stats else masks
        if return_logits:
            out = (out if return_stats else (out,)) + (self._merged.clone(),)
        return out

    def _tiled_static(self, name: str, need: int, dtype=torch.uint8):
        """the static device buffer `name` of predict_images_tiled holds at least `need` elements; grown geometrically, and the tiled
        graphs captured on the old buffer go with it"""
        buf = getattr(self, name)
        if buf is not None and buf.numel() >= need:
            return
        setattr(self, name, torch.zeros(max(need, 256 if buf is None else 2 * buf.numel()), dtype=dtype, device=self.device))
        self._drop("tiled")

    @torch.no_grad()
    def predict_images_tiled(self, images, overlap: int = 64, apply_sigmoid: bool = False, mask_type: Optional[str] = None,
                             return_logits: bool = False, use_graph: bool = True, tile_batch: Optional[int] = None, tta=None):
        """uint8 (h_i, w_i, C) images of ANY sizes -> a list of uint8 {0,255} device masks, one per image at its own size, predicted at
        NATIVE resolution: instead of resizing an image to IMG_SIZE it is cut into IMG_SIZE x IMG_SIZE tiles that overlap by
        `overlap` pixels (tiling.plan_tiles; an image smaller than a tile is padded by reflection), the tiles of the whole batch go
        through the eval forward `tile_batch` at a time (default PREDICT.BATCH_SIZE), and the tile logits are blended into one plane
        per image with weights that rise from the rim of a tile to its middle (uwm_predict_tiled_u8; the rule: DESIGN.md 8r).  A
        pixel under one tile keeps that tile's logit bit for bit.  The reference has no counterpart: it always resizes.
        One captured graph per (number of images, number of forward chunks) serves every batch with those counts, whatever the
        image sizes; it is re-captured when a staging buffer had to grow or the frozen arena was re-made.  mask_type 'watermark' |
        'text' | 'mixed': every blended mask then goes through the reference's _optimize_mask at its own size
        (uwm_optimize_masks_ragged), in place and inside the same graph.  return_logits: also the list of float32 (h_i, w_i) planes
        of blended logits the masks were thresholded from.  tta (as predict_images): every TILE goes through the forward under each
        view of the set and the tile-logit store holds the merged logits (uwm_predict_tiled_tta_u8); the blend, and so return_logits,
        then work on those."""
        descs, mdescs, areas, mask_bytes = self._run_tiled(images, overlap, apply_sigmoid, mask_type, return_logits, use_graph, tile_batch,
                                                           view_mask(tta))
        masks = self._mask_views(mdescs, mask_bytes)
        if not return_logits:
            return masks
        return masks, ragged_views(self._xlbuf[:mask_bytes].clone(), mdescs)

    def _run_tiled(self, images, overlap: int, apply_sigmoid: bool, mask_type: Optional[str], return_logits: bool, use_graph: bool,
                   tile_batch: Optional[int], views: int = 1):
        """stage `images` and run uwm_predict_tiled_u8 (and, with a mask_type, uwm_optimize_masks_ragged in place) as
        predict_images_tiled describes -> (descs, mask descs, areas, mask bytes); the masks are in _mbuf, the blended logits, when
        asked for, in _xlbuf"""
        from .tiling import check_overlap, plan_batch, table_tensor
        if mask_type is not None:
            mask_type_code(mask_type)
        T = int(self.cfg.DATA.IMG_SIZE)
        batch = int(self.cfg.PREDICT.BATCH_SIZE if tile_batch is None else tile_batch)
        overlap = check_overlap(T, T, overlap)
        n, s, descs, mdescs, areas, mask_bytes = self._stage_images(images)
        tiles, plans = plan_batch(list(zip(descs["h"].tolist(), descs["w"].tolist())), T, T, overlap, batch)
        k = len(tiles)
        self._tiled_static("_xtiles", 16 * k)
        self._tiled_static("_xplans", 16 * n)
        if return_logits and (self._xlbuf is None or self._xlbuf.numel() < self._mbuf.numel()):
            self._xlbuf = None
            self._tiled_static("_xlbuf", self._mbuf.numel(), torch.float32)
        self._xtiles[:16 * k].copy_(table_tensor(tiles))
        self._xplans[:16 * n].copy_(table_tensor(plans))
        caps = () if mask_type is None else (mask_type,) + self._mask_capacities(descs, areas)
        lbuf = self._xlbuf if return_logits else None

        def run(static=None):
            if views != 1:
                self.model.predict_tiled_tta_u8(self._ibuf, self._idesc, self._mdesc, self._mbuf, n, self._xtiles, self._xplans, k, batch,
                                                (T, T), overlap, views, IMAGENET_MEAN, IMAGENET_STD, self.threshold, apply_sigmoid, lbuf)
            else:
                self.model.predict_tiled_u8(self._ibuf, self._idesc, self._mdesc, self._mbuf, n, self._xtiles, self._xplans, k, batch, (T, T),
                                            overlap, IMAGENET_MEAN, IMAGENET_STD, self.threshold, apply_sigmoid, lbuf)
            if mask_type is not None:
                optimize_masks_ragged(self._mbuf, self._mdesc, mask_type, False, out=self._mbuf, n=n, max_pixels=caps[1], rows=caps[2])
        if not use_graph:
            run()
        else:
            # (the counts, the threshold, the capacities and the logit plane's pointer are captured arguments)
            key = (n, k // batch, batch, T, overlap, bool(apply_sigmoid), float(self.threshold), bool(return_logits)) + caps
            if views != 1:
                key += ("tta", views)                 # (a graph of its own per view mask)
            self._captured(("tiled", key), key, (batch, T, T), run, group="tiled").graph.replay()
        return descs, mdescs, areas, mask_bytes

    @torch.no_grad()
    def score_images(self, images, truths, mask_type: Optional[str] = None, text_enhance: bool = False, tile: bool = False,
                     overlap: int = 64, boundary_ratio: float = 0.02, boundary_pixels: Optional[int] = None, return_masks: bool = False,
                     tta=None, surface: bool = False):
        """uint8 (h_i, w_i, C) images of ANY sizes and their ground-truth masks, uint8 (h_i, w_i) grey (binarised as > 127) -> the
        int64 (N, 8) HOST array of scoring.COUNT_FIELDS for the masks that predict_images(images, mask_type=..., text_enhance=...)
        or, with tile, predict_images_tiled(images, overlap, mask_type=...) returns: {tp, fp, fn, tn, |B(P) & B(G)|, |B(P)|, |B(G)|,
        status}, B the Boundary-IoU band of distance boundary_pixels or, by default, scoring.boundary_radius(h_i, w_i,
        boundary_ratio).  The prediction runs as it does there, through the same graphs; the truths are staged into
        a buffer of their own under the same mask descriptors and uwm_score_masks_ragged runs behind the prediction on the same
        stream, reading the predicted masks in place.  One device-to-host copy of 64 N bytes; no mask leaves the device unless
        return_masks, which adds the list of device masks.  scoring.metrics_from_counts / summarize turn the rows into metrics.
        tta: as predict_images / predict_images_tiled take it.  surface: uwm_surface_distances_ragged runs behind the score call on
        the same stream, reading the same two buffers; the return value gains (records, sums), the int64 (N, 10) HOST
        array of scoring.SURFACE_FIELDS and the float64 (N, 2) HOST array of its sums, after the counts (and before the masks)"""
        views = view_mask(tta)
        from .scoring import MAX_RADIUS, boundary_radius, score_masks_ragged, surface_distances_ragged
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("score_images runs only on a HIP device (no CPU fallback)")
        if tile and text_enhance:
            raise ValueError("tile and text_enhance cannot be combined: the tiled path has no text enhancement")
        if boundary_pixels is not None and not 0 <= int(boundary_pixels) <= MAX_RADIUS:
            raise ValueError(f"boundary_pixels must be in 0..{MAX_RADIUS}, got {boundary_pixels!r}")
        if boundary_pixels is None and not float(boundary_ratio) >= 0:
            raise ValueError(f"boundary_ratio must not be negative, got {boundary_ratio!r}")
        images, truths = list(images), [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in truths]
        if len(truths) != len(images):
            raise ValueError(f"{len(images)} images but {len(truths)} truth masks")
        for i, (im, t) in enumerate(zip(images, truths)):
            if t.ndim == 3 and t.shape[2] == 1:
                truths[i] = t = t[:, :, 0]
            if t.ndim != 2 or t.dtype != np.uint8 or tuple(t.shape) != tuple(im.shape[:2]):
                raise ValueError(f"truth {i} is {t.dtype} {tuple(t.shape)}: it must be a uint8 mask of its image's size {tuple(im.shape[:2])}")
        if tile:
            descs, mdescs, areas, mask_bytes = self._run_tiled(images, overlap, False, mask_type, False, True, None, views)
        else:
            if mask_type is not None:
                mask_type_code(mask_type)
            descs, mdescs, areas, mask_bytes, _ = self._run_images(images, False, mask_type, True, text_enhance, views)
        n = len(descs)
        radii = [min(boundary_radius(h, w, boundary_ratio), MAX_RADIUS) if boundary_pixels is None else int(boundary_pixels)
                 for h, w in zip(descs["h"].tolist(), descs["w"].tolist())]
        host = np.zeros(mask_bytes, np.uint8)
        for t, o, a in zip(truths, mdescs["offset"], areas):
            host[int(o): int(o) + int(a)] = t.reshape(-1)
        if self._gtbuf is None or self._gtbuf.numel() != self._mbuf.numel():
            self._gtbuf = torch.zeros_like(self._mbuf)
        self._gtbuf[:mask_bytes].copy_(torch.from_numpy(host))
        counts = score_masks_ragged(self._mbuf, self._gtbuf, self._mdesc, torch.tensor(radii, dtype=torch.int32, device=self.device), n=n,
                                    max_pixels=int(areas.max()), rows=int(descs["h"].astype("int64").sum()))
        if surface:
            records, sums = surface_distances_ragged(self._mbuf, self._gtbuf, self._mdesc, n=n, max_pixels=int(areas.max()),
                                                     rows=int(descs["h"].astype("int64").sum()))
        out = counts.cpu().numpy()
        if surface:
            out = (out, (records.cpu().numpy(), sums.cpu().numpy()))
            return out + (self._mask_views(mdescs, mask_bytes),) if return_masks else out
        return (out, self._mask_views(mdescs, mask_bytes)) if return_masks else out

    @torch.no_grad()
    def remove_watermarks(self, images, mask_type: Optional[str] = "watermark", text_enhance: bool = False, tile: bool = False,
                          overlap: int = 64, tta=None, cycles: Optional[int] = None, return_masks: bool = False,
                          return_stats: bool = False):
        """uint8 (h_i, w_i, C) images of ANY sizes -> the list of uint8 (h_i, w_i, C) device tensors with the predicted watermark
        filled in: the reference's `repair` with the membrane fill of inpaint.py in the place of IOPaint's LaMa.  The masks are those
        predict_images(images, mask_type=..., text_enhance=..., tta=...) or, with tile, predict_images_tiled(images, overlap,
        mask_type=..., tta=...) returns, predicted through the same graphs; uwm_inpaint_ragged then runs behind the prediction on the
        same stream, reading the staged image bytes (the originals, not the text-enhanced ones) and the masks where they are.  Nothing
        crosses to the host between prediction and fill.  An image without a predicted pixel, or predicted all over, comes back as
        it is.  It is a smooth fill: it smears texture.  cycles: V-cycles of the solver (default
        inpaint.DEFAULT_CYCLES).  return_masks: also the list of device masks; return_stats: also the int64 (N, 4) HOST array of
        inpaint.INPAINT_STATS_FIELDS (after the masks)"""
        from .inpaint import DEFAULT_CYCLES, MAX_SIDE, check_cycles, inpaint_buffers
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("remove_watermarks runs only on a HIP device (no CPU fallback)")
        if tile and text_enhance:
            raise ValueError("tile and text_enhance cannot be combined: the tiled path has no text enhancement")
        cycles = check_cycles(DEFAULT_CYCLES if cycles is None else cycles)
        views = view_mask(tta)
        images = list(images)
        if tile:
            descs, mdescs, areas, mask_bytes = self._run_tiled(images, overlap, False, mask_type, False, True, None, views)
        else:
            if mask_type is not None:
                mask_type_code(mask_type)
            descs, mdescs, areas, mask_bytes, _ = self._run_images(images, False, mask_type, True, text_enhance, views)
        n, channels = len(descs), int(images[0].shape[2])
        hs, ws = descs["h"].astype("int64"), descs["w"].astype("int64")
        side = int(max(hs.max(), ws.max()))
        if side > MAX_SIDE or int(areas.max()) > 2 ** 30:
            raise ValueError(f"remove_watermarks: an image with a side above {MAX_SIDE} or more than 2^30 pixels")
        stats = torch.empty((n, 4), dtype=torch.int64, device=self.device) if return_stats else None
        nbytes = int(descs["offset"][-1]) + channels * int(areas[-1])
        out = inpaint_buffers(self._ibuf, self._idesc, self._mbuf, self._mdesc, n, channels, max_pixels=int(areas.max()), rows=int(hs.sum()),
                              max_side=side, cycles=cycles, stats=stats)[:nbytes]
        ret = (ragged_views(out, descs, channels),)
        if return_masks:
            ret += (self._mask_views(mdescs, mask_bytes),)
        if return_stats:
            ret += (stats.cpu().numpy(),)
        return ret[0] if len(ret) == 1 else ret

    @torch.no_grad()
    def mask_stats(self, images, mask_type: str = "watermark", return_masks: bool = False, use_graph: bool = True,
                   text_enhance: bool = False):
        """uint8 (h_i, w_i, C) images of ANY sizes -> the int64 (N, 8) HOST array of postprocess.STATS_FIELDS for the masks
        predict_images(mask_type=...) returns: {components found, largest area, foreground pixels, id of the largest or -1,
        components kept, largest kept area, h_i * w_i, status}.  Entries 2, 4, 5 and 6 are what the reference's model selector
        computes from every mask on the host (src/scripts/model_selector.py:171-197).  One captured call and one device-to-host
        copy of 64 N bytes; no mask leaves the device unless return_masks, which adds the list of device masks.  mask_type may also be
        'none': the thresholded masks as they are.  text_enhance: as predict_images."""
        if mask_type not in RAGGED_TYPES:
            raise ValueError(f"mask_type must be one of 'watermark', 'text', 'mixed', 'none', got {mask_type!r}")
        descs, mdescs, areas, mask_bytes, stats = self._run_images(images, False, mask_type, use_graph, text_enhance)
        host = stats.cpu().numpy()
        return (host, self._mask_views(mdescs, mask_bytes)) if return_masks else host

    @torch.no_grad()
    def watermark_counts(self, images, post_process: Optional[bool] = None, return_masks: bool = False, use_graph: bool = True):
        """uint8 (h_i, w_i, C) images of ANY sizes -> an int64 (N, 2) HOST array {watermark pixels, h_i * w_i} per image: the
        reference's src/scripts/watermark_filter.py (predict_mask + has_watermark's count) in ONE library call
        (uwm_filter_images_u8) — resize + Normalize, eval forward, then at each image's own size sigmoid -> bilinear resize of the
        PROBABILITIES -> > PREDICT.THRESHOLD -> [open, close with the 3 x 3 cross] -> count.  post_process=None reads
        cfg.PREDICT.POST_PROCESS.  The staging and the one-graph-per-(N, IMG_SIZE, threshold, post_process) scheme are
        predict_images'; the result comes back in one device-to-host copy of 16 N bytes, and no mask is written unless
        return_masks, which adds the list of uint8 {0,255} device masks."""
        post = bool(self.cfg.PREDICT.POST_PROCESS if post_process is None else post_process)
        n, s, descs, mdescs, areas, mask_bytes = self._stage_images(images)

        def run(static):
            return self.model.filter_images_u8(self._ibuf, self._idesc, self._mdesc, static["counts"], n, (s, s), IMAGENET_MEAN, IMAGENET_STD,
                                               self.threshold, post, self._mbuf if return_masks else None)

        def statics():
            return {"counts": torch.zeros((n, 2), dtype=torch.int64, device=self.device)}
        if not use_graph:
            counts = run(statics())
        else:
            key = (n, s, s, float(self.threshold), post, bool(return_masks))      # (threshold, post_process and the mask pointer are captured arguments)
            e = self._captured("counts", key, (n, s, s), run, statics)
            e.graph.replay()
            counts = e.static["counts"]
        host = counts.cpu().numpy()
        return (host, self._mask_views(mdescs, mask_bytes)) if return_masks else host
