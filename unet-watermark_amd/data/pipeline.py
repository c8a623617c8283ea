"""The device input path of `main.py train --augment ...`: batches of a raw dataset -> what Trainer.step takes, on the device."""
import numpy as np
import torch

from ..constants import IMAGENET_MEAN, IMAGENET_STD
from .augment import device_augment, device_jpeg, device_preprocess, sample_recipe
from .datasets import DeviceU8Dataset, RawSynthDataset
from .jpegragged import device_jpeg_ragged
from .pairmask import device_pair_mask, stage_clean
from .ragged import device_resize, mask_descs_for, pack_images
from .synth import device_synth
from .synthtext import device_synth_text


class DeviceInputPipeline:
    """Batches of a raw dataset -> what Trainer.step takes, on the device.  Raw folder items (uint8 arrays of any size) are packed
    into persistent pinned buffers (pack_images), uploaded and resized to size x size by uwm_resize_u8 — linear for the image,
    nearest for the mask (the reference's A.Resize); RawPairDataset items (image, mask or None, clean or None) get their missing masks
    from uwm_pair_mask_u8 at the image's own size first; DeviceU8Dataset items are gathered.  Training batches then go through
    device_augment with parameters drawn from `generator`, validation batches through device_preprocess (get_val_transform).
    A recipe that draws JPEG qualities ('transparent_watermark') sends the augmented uint8 images through device_jpeg, which normalises."""

    def __init__(self, size, device, source=None, recipe="basic", mean=IMAGENET_MEAN, std=IMAGENET_STD, mask_threshold=None):
        self.size, self.device, self.source, self.recipe = int(size), torch.device(device), source, recipe
        self.mean, self.std = mean, std
        self.mask_threshold = mask_threshold if mask_threshold is not None else getattr(source, "mask_threshold", None)
        self._pin, self._sent = [None, None, None], [None, None, None]

    def _upload(self, arrays, slot, extra=0):
        """extra: spare bytes behind the packed images in the device tensor"""
        need = sum((a.size + 3) // 4 * 4 for a in arrays)
        buf = self._pin[slot]
        if buf is None or buf.numel() < need:
            buf = self._pin[slot] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, pin_memory=True)
            self._sent[slot] = torch.cuda.Event()
        else:
            self._sent[slot].synchronize()                   # the previous batch's upload has left the buffer
        packed, descs, _ = pack_images(arrays, out=buf)
        dev = torch.empty(packed.numel() + extra, dtype=torch.uint8, device=self.device)
        dev[:packed.numel()].copy_(packed, non_blocking=True)
        self._sent[slot].record(torch.cuda.current_stream(self.device))
        return dev, descs

    def to_u8(self, items):
        """-> (images uint8 (N, S, S, C), masks uint8 (N, S, S)) on the device"""
        if isinstance(self.source, DeviceU8Dataset):
            idx = torch.as_tensor([int(i) for i in items], device=self.device)
            return self.source.images[idx], self.source.masks[idx]
        if isinstance(self.source, RawSynthDataset):
            return self._synth_u8(items)
        imgs = [np.ascontiguousarray(it[0]) for it in items]
        cleans = [(it[2] if it[1] is None else None) if len(it) > 2 else None for it in items]      # (a file mask wins over a clean image)
        # an image without a mask file uploads zeros: they stay where there is no clean image either
        masks = [np.ascontiguousarray(it[1])[..., None] if it[1] is not None else np.zeros(a.shape[:2] + (1,), np.uint8)
                 for it, a in zip(items, imgs)]
        for i, (a, m) in enumerate(zip(imgs, masks)):
            if a.shape[:2] != m.shape[:2]:
                raise ValueError(f"image {i} is {a.shape[:2]}, its mask {m.shape[:2]}")
        generate = any(c is not None for c in cleans)
        if generate and self.mask_threshold is None:
            raise ValueError("items with a clean image and no mask need mask_threshold (DATA.GENERATE_MASK_THRESHOLD)")
        with torch.cuda.device(self.device):
            pi, di = self._upload(imgs, 0)
            pm, dm = self._upload(masks, 1)
            if generate:
                pc, dc = stage_clean(cleans, di, self.device, lambda arrs, extra: self._upload(arrs, 2, extra))
                device_pair_mask(pi, di, pc, dc, self.mask_threshold, True, pm, dm)
            x = device_resize(pi, di, self.size, imgs[0].shape[2], "linear")
            m = device_resize(pm, dm, self.size, 1, "nearest")
        return x, m.view(len(items), self.size, self.size)

    def _synth_u8(self, items):
        """RawSynthDataset items (clean, logos, jobs[, planes, text_jobs]): upload the clean images and the logos the batch uses, paste
        the logos into a copy of the clean batch (uwm_synth_u8), then — only where the dataset makes text or mixed samples — upload the
        coverage planes and paste the texts (uwm_synth_text_u8); take the masks from (synthesized, clean) with uwm_pair_mask_u8 — the
        reference's default flow, gen_data.py writes no masks unless asked — or, mask_source 'alpha', from the pasted alpha planes
        (mixed samples by the script's rule: the logos' plane halved, then the maximum with the text's); then resize as ever.  A
        dataset with both ratios 0 yields three-tuples, and this path then launches exactly what it did without text synthesis.
        A dataset with a jpeg_quality sends every image through uwm_jpeg_ragged_u8 behind the last stage — in front of the masks from
        pairs, so those come from the compressed image as the reference's dataset takes them; masks from the alpha planes stay — and
        the mixed samples of the batch (an enabled logo job and a text) once more between the logos and the text; with quality 0
        neither launch happens."""
        cleans = [np.ascontiguousarray(it[0]) for it in items]
        logos, jobs, planes, text_jobs = [], [], [], []
        for it in items:
            j = np.array(it[2], copy=True)
            j["logo"] += len(logos)                              # item-local logo index -> index into the batch's logos
            logos += [np.ascontiguousarray(a) for a in it[1]]
            jobs.append(j)
            if len(it) > 3:
                t = np.array(it[4], copy=True)
                t["glyph"] += len(planes)
                planes += [np.ascontiguousarray(a)[..., None] for a in it[3]]
                text_jobs.append(t)
        alpha = self.source.mask_source == "alpha"
        quality = int(getattr(self.source, "jpeg_quality", 0))
        mixed = [len(it) > 3 and len(it[3]) > 0 and bool((it[2]["enabled"] != 0).any()) for it in items]
        if not alpha and self.mask_threshold is None:
            raise ValueError("synthesized samples with masks from pairs need mask_threshold (DATA.GENERATE_MASK_THRESHOLD)")
        with torch.cuda.device(self.device):
            pc, dc = self._upload(cleans, 0)
            if logos:
                pl, dl = self._upload(logos, 2)
                synth, pm = device_synth(pc, dc, pl, dl, np.stack(jobs), with_mask=alpha)
            else:                                                # a batch of text samples only
                synth = pc.clone()
                pm = torch.zeros(sum(a.shape[0] * a.shape[1] for a in cleans), dtype=torch.uint8, device=self.device) if alpha else None
            if quality and any(mixed):                           # the temporary file between the logos and the text
                synth = device_jpeg_ragged(synth, dc, np.where(mixed, quality, 0), inplace=True)
            if planes:
                pp, dp = self._upload(planes, 1)
                synth, pm = device_synth_text(synth, dc, pp, dp, np.stack(text_jobs), masks=pm, mask_mode=1, inplace=True)
            if quality:                                          # the save of the finished sample
                synth = device_jpeg_ragged(synth, dc, np.full(len(items), quality), inplace=True)
            if not alpha:
                pm = device_pair_mask(synth, dc, pc, dc, self.mask_threshold)
            x = device_resize(synth, dc, self.size, 3, "linear")
            m = device_resize(pm, mask_descs_for(dc), self.size, 1, "nearest")
        return x, m.view(len(items), self.size, self.size)

    def train_batch(self, items, generator=None):
        x, m = self.to_u8(items)
        params, ext, quality = sample_recipe(self.recipe, x.shape[0], x.shape[1], x.shape[2], generator)
        if quality is None:
            return device_augment(x, m, params, self.mean, self.std, ext=ext)
        _, mo, u8 = device_augment(x, m, params, self.mean, self.std, return_u8=True, ext=ext)
        return device_jpeg(u8, quality, self.mean, self.std), mo

    def val_batch(self, items):
        x, m = self.to_u8(items)
        return device_preprocess(x, m, None, self.mean, self.std)
