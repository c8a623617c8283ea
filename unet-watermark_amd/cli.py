"""`python main.py train|predict|repair|masks|filter|select|synth|extract ...` — counterpart of the reference's CLI for the model path
(/root/reference/src/cli.py:368-395 flag names; train loop order /root/reference/src/train.py:207-499:
epochs of train_epoch + validate (val batch = 2x train batch, :254), Adam | SGD (:265-279), ReduceLROnPlateau on the
val loss | CosineAnnealingLR (:280-296,408-412), best / periodic checkpoints (:428-460), early stopping (:37-66,362-368)).
`repair` predicts the masks and fills them with the weight-free membrane fill of inpaint.py; the reference's IOPaint /
LaMa, OCR, diffusion and video steps and its `auto` mode stay out of scope (SURVEY.md §2 rows 6,9,10: their weights do not ship); the data synthesis runs on the device (`train
--synthesize`, `synth`): logo watermarks and, with --text-watermark-ratio / --mixed-watermark-ratio, text and mixed
ones (§8o; the OCR mask is not served, masks come from pairs or from the pasted alpha planes).
Multi-GPU: launch with torch.distributed.run; every rank trains its shard, gradients are all-reduced."""
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, Subset
from torch.utils.data.distributed import DistributedSampler

from .checkpoint import load_checkpoint, save_checkpoint
from .config import get_cfg_defaults, update_config
from .data import (AUG_RECIPES, AUG_RECIPES_EXT, DeviceInputPipeline, DeviceU8Dataset, FolderDataset, RawFolderDataset, RawPairDataset,
                   RawSynthDataset, SyntheticWatermarkDataset, list_collate)
from .losses import CombinedLoss, FocalLoss, criterion_spec, get_loss_function
from .metrics import logits_metrics
from .model import create_model_from_config
from .predict import WatermarkPredictor
from .train import Trainer


def _loss_weights(cfg):
    name = cfg.LOSS.NAME
    if name == "DiceLoss":
        return 1.0, 0.0
    if name == "BCEWithLogitsLoss":
        return 0.0, 1.0
    if name == "CombinedLoss":
        return float(cfg.LOSS.DICE_WEIGHT), float(cfg.LOSS.BCE_WEIGHT)
    raise ValueError(f"unsupported LOSS.NAME {name!r} (DiceLoss | BCEWithLogitsLoss | CombinedLoss)")


def _criterion(cfg, args=None):
    """The configured loss as a module: get_loss_function(cfg), plus the focal term of --focal-weight config|FLOAT.  The flag is
    served with LOSS.NAME CombinedLoss only (the text-watermark recipe, whose FOCAL_WEIGHT the reference's own trainer ignores):
    'config' takes the weight from LOSS.FOCAL_WEIGHT, a number is the weight; both read LOSS.FOCAL_ALPHA and LOSS.FOCAL_GAMMA."""
    criterion = get_loss_function(cfg)
    fw = getattr(args, "focal_weight", None)
    if fw is None:
        return criterion
    if cfg.LOSS.NAME != "CombinedLoss":
        raise ValueError(f"--focal-weight adds a focal term to LOSS.NAME 'CombinedLoss'; the config names {cfg.LOSS.NAME!r} "
                         "(LOSS.NAME 'FocalLoss' trains on the focal loss alone)")
    if fw == "config":
        if cfg.LOSS.get("FOCAL_WEIGHT", None) is None:
            raise ValueError("--focal-weight config: the config has no LOSS.FOCAL_WEIGHT")
        weight = float(cfg.LOSS.FOCAL_WEIGHT)
    else:
        try:
            weight = float(fw)
        except ValueError:
            raise ValueError(f"--focal-weight {fw!r}: 'config' or a number") from None
    alpha = cfg.LOSS.get("FOCAL_ALPHA", None)
    focal = FocalLoss(mode=getattr(cfg.LOSS, "MODE", "binary"), alpha=None if alpha is None else float(alpha),
                      gamma=float(cfg.LOSS.get("FOCAL_GAMMA", 2.0)))
    return CombinedLoss(criterion.losses + [focal], criterion.weights + [weight])


def _loss_spec(cfg, args=None):
    """The Trainer's loss_spec: None for the losses the Dice / BCE step serves (DiceLoss | BCEWithLogitsLoss | CombinedLoss without
    --focal-weight: the Trainer then takes _loss_weights, as before), else the uwm_loss_spec of _criterion(cfg, args)."""
    if cfg.LOSS.NAME in ("DiceLoss", "BCEWithLogitsLoss", "CombinedLoss") and getattr(args, "focal_weight", None) is None:
        return None
    return criterion_spec(_criterion(cfg, args))


def _served_recipe(augment, cfg, jpeg="refuse"):
    """--augment, DATA.AUGMENTATION_TYPE and --jpeg -> (the recipe the device serves, or 'none'; a note for the 'serving' line).
    'basic' serves the basic recipe whatever the config asks for, and says so; 'config' serves the recipe that DATA.AUGMENTATION_TYPE
    names as the reference chooses it (src/utils/dataset.py:417-427: 'transparent_watermark', 'enhanced', anything else is basic).
    'transparent_watermark' is served only with --jpeg device (its ImageCompression stage is then the baseline libjpeg round trip
    of uwm_jpeg_u8) and refused otherwise."""
    asked = cfg.DATA.get("AUGMENTATION_TYPE", None)
    if jpeg not in ("refuse", "device"):
        raise ValueError(f"--jpeg {jpeg!r}: 'refuse' or 'device'")
    if augment == "none":
        return "none", ""
    if augment == "config":
        if asked == "transparent_watermark":
            if jpeg != "device":
                raise ValueError("--augment config: DATA.AUGMENTATION_TYPE='transparent_watermark' is served only with --jpeg device "
                                 "(its ImageCompression stage then runs as a baseline JPEG round trip on the device); without the flag "
                                 "--augmentation-type enhanced or basic is served")
            return asked, (f" (DATA.AUGMENTATION_TYPE={asked!r}; ImageCompression is the baseline libjpeg round trip (4:2:0, integer "
                           "DCT) on the device, and Affine uses the warp's reflect-101 border and one scale instead of a zero fill)")
        if asked in AUG_RECIPES_EXT:
            return asked, f" (DATA.AUGMENTATION_TYPE={asked!r})"
        return "basic", f" (DATA.AUGMENTATION_TYPE={asked!r} selects the basic recipe, as in the reference)"
    if augment not in AUG_RECIPES:
        raise ValueError(f"--augment {augment!r}: this build serves 'none', 'config' and {AUG_RECIPES}")
    note = "" if asked == augment else f" (DATA.AUGMENTATION_TYPE={asked!r} is not served; its extra stages are NOT applied)"
    return augment, note


def _pair_roots(cfg):
    """DATA.ROOT_DIR + DATA.ADDITIONAL_ROOT_DIRS: the roots of the reference's create_datasets (src/utils/dataset.py:406-414)"""
    return [cfg.DATA.ROOT_DIR] + list(cfg.DATA.get("ADDITIONAL_ROOT_DIRS", None) or [])


def _pair_dataset(cfg):
    """The RawPairDataset of the configured roots when the data needs it — more than one root, or an image without a mask file, whose
    mask is then derived from its clean counterpart — else None: RawFolderDataset serves a single root with every mask as a file."""
    roots = _pair_roots(cfg)
    pair = RawPairDataset(roots, int(cfg.DATA.GENERATE_MASK_THRESHOLD))
    return pair if len(roots) > 1 or pair.missing_masks() else None


def _datasets(cfg, synthetic, device_input=None):
    """device_input: a torch.device = the raw datasets of the device input path (--augment basic) instead of host-prepared tensors"""
    if synthetic or not os.path.isdir(os.path.join(cfg.DATA.ROOT_DIR, "watermarked")):
        full = SyntheticWatermarkDataset(int(synthetic or 256), cfg.DATA.IMG_SIZE, cfg.DATA.SEED)
        if device_input is not None:
            full = DeviceU8Dataset(full, device_input)
    elif device_input is not None:
        full = _pair_dataset(cfg) or RawFolderDataset(cfg.DATA.ROOT_DIR)
    else:
        full = FolderDataset(cfg.DATA.ROOT_DIR, cfg.DATA.IMG_SIZE)
    n = len(full)
    g = torch.Generator().manual_seed(int(cfg.DATA.SEED))
    perm = torch.randperm(n, generator=g).tolist() if cfg.DATA.SHUFFLE else list(range(n))
    ntr = max(1, int(n * float(cfg.DATA.TRAIN_RATIO)))
    return Subset(full, perm[:ntr]), Subset(full, perm[ntr:] or perm[:1])


def _check_synthesize(args, augment):
    """the refusals of `train --synthesize`, before any device work"""
    quality = _check_jpeg_quality(getattr(args, "synth_jpeg_quality", 0), "--synth-jpeg-quality")
    if not getattr(args, "synthesize", False):
        if quality:
            raise ValueError("--synth-jpeg-quality is the JPEG save of the samples that --synthesize makes: give --synthesize as well")
        return
    if args.synthetic:
        raise ValueError("--synthesize and --synthetic exclude each other: --synthetic N trains on a toy generator's images, --synthesize "
                         "pastes real logos onto the images of --clean-dir")
    if augment == "none":
        raise ValueError("--synthesize runs on the device input path (the logos are pasted at each image's own size, in front of the "
                         "device's resize, augmentation and Normalize): give --augment basic or --augment config")
    _check_text_ratios(args)
    if not args.clean_dir or (not args.logos_dir and float(args.text_watermark_ratio) < 1):
        raise ValueError("--synthesize needs --clean-dir (clean photographs) and --logos-dir (logo images; only --text-watermark-ratio 1 "
                         "does without)")


def _check_jpeg_quality(value, flag):
    """-> the quality of a synthesis flag as an int; ValueError, before any device work, unless it is 0 (no round trip) or 1..100"""
    from .data import check_jpeg_quality
    return check_jpeg_quality(value, flag)


_JPEG_QUALITY_HELP = ("send every synthesized image through a baseline 4:2:0 JPEG round trip of this quality on the device (1..100), at "
                      "its own size, bit-equal to Pillow's save and reload; a mixed sample also once between its logos and its text.  The "
                      "reference's value is 95 (gen_data.py saves every sample so); 0 (default) = no round trip, and a command without the "
                      "flag produces byte-identical results")


def _check_text_ratios(args):
    """the refusals that the text and mixed shares bring, before any device work: the ratios' range, and freetype"""
    from .data.datasets import check_synth_ratios
    from .data import require_freetype
    t, m = check_synth_ratios(args.text_watermark_ratio, args.mixed_watermark_ratio)
    if t > 0 or m > 0:
        require_freetype("--text-watermark-ratio / --mixed-watermark-ratio")


def _add_text_arguments(p, prefix):
    p.add_argument("--text-watermark-ratio", type=float, default=0.0,
                   help=f"{prefix}share of samples that carry a text watermark (the text branch of gen_data.py).  The reference's default is "
                        "0.3; 0 here, so that a command without the flag produces byte-identical results")
    p.add_argument("--mixed-watermark-ratio", type=float, default=0.0,
                   help=f"{prefix}share of samples with one or two logos and a text (the reference's default is 0.2; 0 here, as above)")
    p.add_argument("--fonts-dir", type=str, default=None,
                   help=f"{prefix}directory of ttf / otf / ttc fonts for the texts (default: Pillow's embedded scalable font)")
    p.add_argument("--texts-file", type=str, default=None,
                   help=f"{prefix}the texts: one per line, blank lines separate categories (default: a short built-in list)")


def _synth_kinds_note(ds):
    if not ds.with_text:
        return "logo watermarks only"
    return f"text watermarks on {ds.text_ratio:g} of the samples, logos and a text on {ds.mixed_ratio:g}, {len(ds.fonts.paths)} font(s)"


def _synth_datasets(cfg, args):
    """train / validation splits of the clean images, as _datasets splits a folder; the training split draws new samples every epoch
    (set_epoch), the validation split is never told the epoch and so reproduces its samples"""
    kw = dict(seed=int(args.synth_seed), transparent_ratio=float(args.transparent_ratio), multi_watermark_ratio=float(args.multi_watermark_ratio),
              max_watermarks=int(args.synth_max_watermarks), mask_threshold=int(cfg.DATA.GENERATE_MASK_THRESHOLD), mask_source=args.synth_mask,
              text_watermark_ratio=float(args.text_watermark_ratio), mixed_watermark_ratio=float(args.mixed_watermark_ratio),
              fonts_dir=args.fonts_dir, texts_file=args.texts_file, jpeg_quality=int(getattr(args, "synth_jpeg_quality", 0)))
    train, val = RawSynthDataset(args.clean_dir, args.logos_dir, **kw), RawSynthDataset(args.clean_dir, args.logos_dir, **kw)
    n = len(train)
    g = torch.Generator().manual_seed(int(cfg.DATA.SEED))
    perm = torch.randperm(n, generator=g).tolist() if cfg.DATA.SHUFFLE else list(range(n))
    ntr = max(1, int(n * float(cfg.DATA.TRAIN_RATIO)))
    return Subset(train, perm[:ntr]), Subset(val, perm[ntr:] or perm[:1])


@torch.no_grad()
def _validate(model, loader, criterion, device, pipe=None):
    model.eval()
    tot, nb, agg = 0.0, 0, {}
    for batch in loader:
        if pipe is not None:                               # device input path: resize + Normalize, no augmentation
            x, t = pipe.val_batch(batch)
            t = t.long()
        else:
            x, t = batch
            x, t = x.to(device, non_blocking=True), t.to(device, non_blocking=True)
        out = model(x)
        tot += float(criterion(out, t.unsqueeze(1)))
        for k, v in logits_metrics(out, t).items():
            agg[k] = agg.get(k, 0.0) + v
        nb += 1
    nb = max(nb, 1)
    return tot / nb, {k: v / nb for k, v in agg.items()}


class EarlyStopping:
    """/root/reference/src/train.py:37-66 (patience, min_delta, restore_best_weights) with the shallow-copy quirk fixed
    (real clones).  Every rank holds one and feeds it the SAME (all-reduced) validation loss, so the
    stop decision is rank-consistent by construction."""

    def __init__(self, patience=7, min_delta=0.0, restore_best_weights=True):
        self.patience, self.min_delta, self.restore = int(patience), float(min_delta), restore_best_weights
        self.best_loss, self.counter, self.best_weights = None, 0, None

    def __call__(self, val_loss, model) -> bool:
        if self.best_loss is None or val_loss < self.best_loss - self.min_delta:
            if self.best_loss is not None:
                self.counter = 0
            self.best_loss = val_loss
            if self.restore:
                self.best_weights = {k: v.detach().clone() for k, v in model.state_dict().items()}
        else:
            self.counter += 1
        if self.counter >= self.patience:
            if self.restore and self.best_weights is not None:
                model.load_state_dict(self.best_weights)
            return True
        return False


def _rank_mean(value: float, device, world: int) -> float:
    """Mean over ranks of a host scalar (each rank validates with its own BatchNorm running statistics — the reference
    has no SyncBN — so per-rank validation losses differ slightly; every decision below uses this ONE number)."""
    if world <= 1:
        return float(value)
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item()) / world


def _make_scheduler(cfg, opt):
    """/root/reference/src/train.py:280-296"""
    name = cfg.OPTIMIZER.LR_SCHEDULER
    if name == "ReduceLROnPlateau":
        return torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=float(cfg.OPTIMIZER.SCHEDULER_FACTOR),
                                                          patience=int(cfg.OPTIMIZER.SCHEDULER_PATIENCE))
    if name == "CosineAnnealingLR":
        return torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=int(cfg.TRAIN.EPOCHS))
    if name == "CosineAnnealingWarmRestarts":          # the text-watermark trainer (src/text/train_text_watermark.py:85-91)
        o = cfg.OPTIMIZER
        if o.get("SCHEDULER_T_0") is None:
            raise ValueError("OPTIMIZER.LR_SCHEDULER=CosineAnnealingWarmRestarts needs OPTIMIZER.SCHEDULER_T_0")
        return torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(
            opt, T_0=int(o.SCHEDULER_T_0), T_mult=int(o.get("SCHEDULER_T_MULT", 1)), eta_min=float(o.get("SCHEDULER_ETA_MIN", 0.0)))
    return None


def train_command(args):
    cfg = get_cfg_defaults()
    if args.config and os.path.exists(args.config):
        update_config(cfg, args.config)
    for flag, (sec, key) in dict(data_dir=("DATA", "ROOT_DIR"), output_dir=("TRAIN", "OUTPUT_DIR"),
                                 model_save_path=("TRAIN", "MODEL_SAVE_PATH"), batch_size=("TRAIN", "BATCH_SIZE"),
                                 epochs=("TRAIN", "EPOCHS"), lr=("TRAIN", "LR"), img_size=("DATA", "IMG_SIZE"),
                                 early_stopping_patience=("TRAIN", "EARLY_STOPPING_PATIENCE")).items():
        if getattr(args, flag, None) is not None:
            cfg[sec][key] = getattr(args, flag)
    if args.no_early_stopping:
        cfg.TRAIN.USE_EARLY_STOPPING = False
    if args.encoder:
        cfg.MODEL.ENCODER_NAME = args.encoder
    if getattr(args, "model", None):
        cfg.MODEL.NAME = args.model
    if getattr(args, "optimizer", None):
        cfg.OPTIMIZER.NAME = args.optimizer
    if getattr(args, "lr_scheduler", None):
        cfg.OPTIMIZER.LR_SCHEDULER = args.lr_scheduler
    if getattr(args, "augmentation_type", None):
        cfg.DATA.AUGMENTATION_TYPE = args.augmentation_type
    augment, aug_note = _served_recipe(getattr(args, "augment", None) or "none", cfg, getattr(args, "jpeg", None) or "refuse")      # refusals come before any device work
    _check_synthesize(args, augment)
    synthesize = bool(getattr(args, "synthesize", False))
    if getattr(args, "checkpoint_dir", None):
        cfg.TRAIN.CHECKPOINT_DIR = args.checkpoint_dir
    if (getattr(args, "use_blurred_mask", False) and not args.synthetic and not synthesize and os.path.isdir(os.path.join(cfg.DATA.ROOT_DIR, "watermarked"))
            and RawPairDataset(_pair_roots(cfg), int(cfg.DATA.GENERATE_MASK_THRESHOLD)).missing_masks()):
        raise ValueError("--use-blurred-mask: this dataset has images without a mask file, whose masks are derived from their clean "
                         "counterparts, and the reference's blurred variant of that rule (contours, convex hulls, approxPolyDP) is not "
                         "served; drop the flag (exact masks, the reference's default) or provide every mask as a file")
    if cfg.MODEL.NAME not in ("Unet", "UnetPlusPlus"):
        raise ValueError(f"MODEL.NAME={cfg.MODEL.NAME!r}: this build serves 'Unet' and 'UnetPlusPlus'")
    if cfg.OPTIMIZER.NAME not in ("Adam", "AdamW", "SGD"):
        raise ValueError(f"unsupported optimizer: {cfg.OPTIMIZER.NAME}")           # /root/reference/src/train.py:279
    criterion = _criterion(cfg, args)            # (an unserved LOSS.NAME or --focal-weight is refused here, before any device work)
    loss_spec = _loss_spec(cfg, args)
    if cfg.MODEL.ENCODER_WEIGHTS is not None:
        print(f"note: ENCODER_WEIGHTS={cfg.MODEL.ENCODER_WEIGHTS!r} needs a download; training from seeded init")
        cfg.MODEL.ENCODER_WEIGHTS = None

    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("training needs a HIP device (this path has no CPU fallback)")
    ndev = torch.cuda.device_count()
    backend = os.environ.get("UWM_DIST_BACKEND", "nccl")      # tests: "gloo" lets several ranks share one GPU (RCCL refuses that)
    if backend == "gloo":
        local = local % max(1, ndev)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    own_group = False
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend, **({"device_id": device} if backend == "nccl" else {}))
        own_group = True
    torch.manual_seed(int(cfg.DATA.SEED))
    model = create_model_from_config(cfg).to(device)
    wd, wb = (1.0, 0.0) if loss_spec is not None else _loss_weights(cfg)          # (a loss_spec replaces them)
    trainer = Trainer(model, w_dice=wd, w_bce=wb, smooth=float(cfg.LOSS.SMOOTH), lr=float(cfg.TRAIN.LR),
                      weight_decay=float(cfg.TRAIN.WEIGHT_DECAY), optimizer=cfg.OPTIMIZER.NAME,
                      max_grad_norm=(float(cfg.TRAIN.GRADIENT_CLIP) if args.grad_clip else None),
                      global_dice=bool(getattr(args, "global_dice", False)), loss_spec=loss_spec)
    sched = _make_scheduler(cfg, trainer.opt)
    start_epoch, best = 0, float("inf")
    tr_losses, va_losses, tr_hist, va_hist = [], [], [], []
    if args.resume:
        ck = load_checkpoint(args.resume, model, trainer.opt)
        if sched is not None and ck.get("scheduler_state_dict"):
            sched.load_state_dict(ck["scheduler_state_dict"])
        start_epoch = int(ck.get("epoch", 0))            # stored epoch is already +1 (Appendix B.9)
        b = ck.get("best_val_loss", ck.get("val_loss"))
        best = float(b) if b is not None else best
        tr_losses, va_losses = list(ck.get("train_losses", [])), list(ck.get("val_losses", []))
        tr_hist, va_hist = list(ck.get("train_metrics_history", [])), list(ck.get("val_metrics_history", []))
        if world > 1:                                    # every rank read the file; make the replicas bit-identical anyway
            from .train import broadcast_model
            broadcast_model(model, 0)
    stopper = (EarlyStopping(patience=int(cfg.TRAIN.EARLY_STOPPING_PATIENCE), restore_best_weights=True)
               if cfg.TRAIN.USE_EARLY_STOPPING else None)       # /root/reference/src/train.py:362-368
    pipe = None
    tr_set, va_set = _synth_datasets(cfg, args) if synthesize else _datasets(cfg, args.synthetic, device if augment != "none" else None)
    if augment != "none":
        pipe = DeviceInputPipeline(cfg.DATA.IMG_SIZE, device, source=tr_set.dataset, recipe=augment)
        if rank == 0:
            print(f"augmentation: serving the {augment!r} recipe on the device{aug_note}", flush=True)
            if isinstance(tr_set.dataset, RawPairDataset):
                print(f"masks: {len(tr_set.dataset.missing_masks())} of {len(tr_set.dataset)} images have no mask file; theirs are derived on "
                      f"the device from the clean counterpart (DATA.GENERATE_MASK_THRESHOLD={tr_set.dataset.mask_threshold}), zero without "
                      "one; nothing is written (`main.py masks` persists them)", flush=True)
            if synthesize:
                print(f"synthesis: {len(tr_set.dataset)} clean images x {len(tr_set.dataset.logos)} logos, pasted on the device at each image's "
                      f"own size ({_synth_kinds_note(tr_set.dataset)}; masks from "
                      f"{'the pasted alpha planes' if args.synth_mask == 'alpha' else 'synthesized / clean pairs'})",
                      flush=True)
    bs = int(cfg.TRAIN.BATCH_SIZE)
    sampler = DistributedSampler(tr_set, world, rank, shuffle=True, seed=int(cfg.DATA.SEED)) if world > 1 else None
    # the device input path gets raw items from the workers (uint8 arrays of any size, or indices): nothing to stack or pin
    extra = dict(pin_memory=True) if pipe is None else dict(collate_fn=list_collate)
    if isinstance(tr_set.dataset, DeviceU8Dataset):
        extra["num_workers"] = 0                           # items are indices into device tensors
    tr = DataLoader(tr_set, bs, shuffle=sampler is None, sampler=sampler, drop_last=True, **{"num_workers": int(args.workers), **extra})
    va = DataLoader(va_set, bs * 2, shuffle=False, **{"num_workers": int(args.workers), **extra})
    hist = []
    for epoch in range(start_epoch, int(cfg.TRAIN.EPOCHS)):
        if sampler is not None:
            sampler.set_epoch(epoch)
        if synthesize:
            tr_set.dataset.set_epoch(epoch)                   # (the workers of this epoch's loader start after this)
        model.train()
        t0, seen = time.time(), 0
        acc = torch.zeros(3, device=device)
        if pipe is not None:                              # ranks draw different parameters; a rerun reproduces them
            aug_gen = torch.Generator().manual_seed((int(cfg.DATA.SEED) * 1000003 + epoch) * 1009 + rank)
        for batch in tr:
            if pipe is not None:
                x, t = pipe.train_batch(batch, aug_gen)
            else:
                x, t = batch[0].to(device, non_blocking=True), batch[1].to(device, non_blocking=True)
            acc += trainer.step(x, t)
            seen += x.shape[0]
        torch.cuda.synchronize(device)
        dt = time.time() - t0
        tl = _rank_mean(float(acc[0]) / max(1, len(tr)), device, world)
        vl_local, vm = _validate(model, va, criterion, device, pipe)
        # ONE validation loss for every rank: LR schedule, best-model bookkeeping and early stopping all read it, so
        # the replicas take the same decisions and nobody leaves the collective early
        vl = _rank_mean(vl_local, device, world)
        vm = {k: _rank_mean(v, device, world) for k, v in sorted(vm.items())}
        if sched is not None:
            if cfg.OPTIMIZER.LR_SCHEDULER == "ReduceLROnPlateau":
                sched.step(vl)
            else:
                sched.step()
        tr_losses.append(tl); va_losses.append(vl); tr_hist.append({}); va_hist.append(vm)
        rec = dict(epoch=epoch + 1, train_loss=tl, val_loss=vl, val_metrics=vm, lr=trainer.opt.param_groups[0]["lr"],
                   images_per_sec=world * seen / max(dt, 1e-9))
        hist.append(rec)
        improved = vl < best
        if improved:
            best = vl                                       # on EVERY rank
        if rank == 0:                                       # rank 0's BatchNorm buffers are the ones saved
            print(json.dumps(rec), flush=True)
            if improved:
                save_checkpoint(cfg.TRAIN.MODEL_SAVE_PATH, model, epoch + 1, vl, vm, cfg)
            interval = max(5, int(cfg.TRAIN.EPOCHS) // 10)
            if (epoch + 1) % interval == 0 or epoch >= int(cfg.TRAIN.EPOCHS) - 3:
                save_checkpoint(os.path.join(cfg.TRAIN.CHECKPOINT_DIR, f"checkpoint_epoch_{epoch + 1:03d}.pth"), model,
                                epoch + 1, vl, vm, cfg, optimizer=trainer.opt, scheduler=sched, train_loss=tl,
                                train_metrics={}, best_val_loss=best, train_losses=tr_losses, val_losses=va_losses,
                                train_metrics_history=tr_hist, val_metrics_history=va_hist)
        if stopper is not None and stopper(vl, model):
            if rank == 0:
                print(json.dumps({"early_stop": epoch + 1, "best_val_loss": stopper.best_loss}), flush=True)
            break
    # final model (/root/reference/src/train.py:467-485): weights as they stand after the loop — i.e. the RESTORED best weights
    # after an early stop — with the optimizer / scheduler state and is_final=True
    if rank == 0 and hist:
        last = hist[-1]
        save_checkpoint(os.path.join(cfg.TRAIN.CHECKPOINT_DIR, f"final_model_epoch_{last['epoch']:03d}.pth"), model,
                        last["epoch"], last["val_loss"], last["val_metrics"], cfg, optimizer=trainer.opt, scheduler=sched,
                        train_loss=last["train_loss"], train_metrics={}, best_val_loss=best, is_final=True)
    if own_group:
        dist.destroy_process_group()
    return hist


def predict_command(args):
    text_enhance = bool(getattr(args, "text_enhance", False))
    if text_enhance and args.resize != "device":
        raise ValueError("--text-enhance needs --resize device: the reference's text-feature enhancement works on every image at its own "
                         "size, which only the ragged device path serves (--resize host resizes on the host first)")
    tile = bool(getattr(args, "tile", False))
    if tile and args.resize != "device":
        raise ValueError("--tile needs --resize device: tiles are cut from every image at its own size, which only the ragged device "
                         "path serves (--resize host resizes on the host first)")
    if tile and text_enhance:
        raise ValueError("--tile cannot be combined with --text-enhance: enhancing the images before they are cut into tiles is not "
                         "built yet; run one or the other")
    tta = getattr(args, "tta", "none") or "none"
    if tta != "none" and args.resize != "device":
        raise ValueError("--tta needs --resize device: the views are made and their logits merged on the device, inside the ragged device "
                         "path's one call (--resize host runs the plain forward)")
    cfg = get_cfg_defaults()
    if args.config and os.path.exists(args.config):
        update_config(cfg, args.config)
    if args.encoder:
        cfg.MODEL.ENCODER_NAME = args.encoder
    if args.threshold is not None:
        cfg.PREDICT.THRESHOLD = args.threshold
    pred = WatermarkPredictor(args.model, None, cfg, device="cuda")
    from PIL import Image
    import numpy as np
    os.makedirs(args.output, exist_ok=True)
    files = sorted(f for f in os.listdir(args.input) if f.lower().endswith((".png", ".jpg", ".jpeg")))
    s, bs = int(cfg.DATA.IMG_SIZE), int(args.batch_size or cfg.PREDICT.BATCH_SIZE)
    if tta != "none":
        cfg.PREDICT.BATCH_SIZE = bs                            # the views of a batch go through the network --batch-size at a time
    for i in range(0, len(files), bs):
        chunk = files[i:i + bs]
        ims = [Image.open(os.path.join(args.input, f)).convert("RGB") for f in chunk]
        if tile:                                               # native resolution: overlapping IMG_SIZE tiles, blended on the device
            masks = pred.predict_images_tiled([np.asarray(im, dtype=np.uint8) for im in ims], int(args.tile_overlap), args.sigmoid,
                                              args.mask_type, use_graph=len(chunk) == bs, tile_batch=bs, tta=tta)
            for f, m in zip(chunk, masks):
                Image.fromarray(m.cpu().numpy()).save(os.path.join(args.output, os.path.splitext(f)[0] + "_mask.png"))
            continue
        if args.resize == "device":                            # cv2-convention resize on the device, both ways, in one call
            masks = pred.predict_images([np.asarray(im, dtype=np.uint8) for im in ims], args.sigmoid, args.mask_type,
                                        use_graph=len(chunk) == bs, text_enhance=text_enhance, tta=tta)
            for f, m in zip(chunk, masks):
                Image.fromarray(m.cpu().numpy()).save(os.path.join(args.output, os.path.splitext(f)[0] + "_mask.png"))
            continue
        arr = np.stack([np.asarray(im.resize((s, s), Image.BILINEAR), dtype=np.uint8) for im in ims])
        logits = pred.logits(pred.preprocess(torch.from_numpy(arr)), use_graph=len(chunk) == bs)
        from .metrics import resize_threshold
        from .postprocess import optimize_mask
        for k, (f, im) in enumerate(zip(chunk, ims)):          # bilinear resize of the raw logits to the original size, then threshold
            m = resize_threshold(logits[k:k + 1], (im.size[1], im.size[0]), pred.threshold, args.sigmoid)
            if args.mask_type:                                 # the reference's _optimize_mask, per image at its original size
                m = optimize_mask(m, args.mask_type)
            m = m[0].cpu().numpy()
            Image.fromarray(m).save(os.path.join(args.output, os.path.splitext(f)[0] + "_mask.png"))
    print(f"wrote {len(files)} masks to {args.output}")


def masks_command(args):
    """Write masks/<stem>.png, at the image's own size, for every image that has a clean counterpart and no mask file: the masks
    `train --augment basic|config` derives on the fly, persisted where the reference persists them (its first mask directory,
    src/utils/dataset.py:179-190)."""
    import numpy as np
    from PIL import Image
    from .data import device_pair_mask, mask_descs_for, pack_images, stage_clean
    cfg = get_cfg_defaults()
    if args.config and os.path.exists(args.config):
        update_config(cfg, args.config)
    if args.data_dir:
        cfg.DATA.ROOT_DIR = args.data_dir
    thr = int(args.threshold if args.threshold is not None else cfg.DATA.GENERATE_MASK_THRESHOLD)
    ds = RawPairDataset(_pair_roots(cfg), thr)                        # (refuses a threshold outside 0..255)
    if not torch.cuda.is_available():
        raise SystemExit("masks needs a HIP device (this path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    missing = ds.missing_masks()
    out_dir = ds.mask_dirs[0]
    os.makedirs(out_dir, exist_ok=True)
    bs = max(1, int(args.batch_size or 16))
    written = no_clean = 0
    for b in range(0, len(missing), bs):
        pairs = [(i, ds[i]) for i in missing[b:b + bs]]
        no_clean += sum(1 for _, it in pairs if it[2] is None)
        pairs = [(i, it) for i, it in pairs if it[2] is not None]
        if not pairs:
            continue
        packed, descs, _ = pack_images([it[0] for _, it in pairs])
        wm = packed.to(device, non_blocking=True)
        clean, cdescs = stage_clean([it[2] for _, it in pairs], descs, device)
        out = device_pair_mask(wm, descs, clean, cdescs, thr).cpu().numpy()
        for (i, _), d in zip(pairs, mask_descs_for(descs)):
            o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
            stem = os.path.splitext(os.path.basename(ds.files[i]))[0]
            Image.fromarray(out[o:o + h * w].reshape(h, w)).save(os.path.join(out_dir, stem + ".png"))
            written += 1
    res = dict(written=written, skipped=len(ds) - len(missing), no_clean=no_clean, threshold=thr, output=out_dir)
    print(f"wrote {written} masks to {out_dir} (threshold {thr}); skipped {res['skipped']} with a mask file; "
          f"{no_clean} left without a clean image")
    return res


def synth_command(args):
    """The reference's src/scripts/gen_data.py on the device: --count samples into <output-dir>/watermarked (PNG, so the pixels are
    the device's; the reference saves JPEG quality 95, and --jpeg-quality 95 puts exactly that round trip into the pixels on the device:
    the files then hold what `train --synthesize --synth-jpeg-quality 95` sees), a same-named copy of the clean image into <output-dir>/clean — which is what
    lets RawPairDataset derive the masks — and, with --generate-mask, the script's own masks into <output-dir>/masks: the pasted alpha
    planes, for a mixed sample the logos' plane halved and then the maximum with the text's.  (That halved part never survives the
    reference dataset's binarisation at 127 — the script's quirk, kept — which is one reason why masks from pairs are the default
    of `train --synthesize`.)  Text and mixed samples (--text-watermark-ratio, --mixed-watermark-ratio; both 0 by default) carry the
    script's prefixes text_trans_ / text_norm_ / mixed_trans_ / mixed_norm_."""
    import random
    import numpy as np
    from PIL import Image
    from .data import device_jpeg_ragged, device_synth, device_synth_text, mask_descs_for, pack_images
    from .data.datasets import read_u8
    quality = _check_jpeg_quality(getattr(args, "jpeg_quality", 0), "--jpeg-quality")
    if int(args.count) < 1:
        raise ValueError("synth: --count must be >= 1")
    _check_text_ratios(args)
    if not args.logos_dir and float(args.text_watermark_ratio) < 1:
        raise ValueError("synth needs --logos-dir (logo images; only --text-watermark-ratio 1 does without)")
    ds = RawSynthDataset(args.clean_dir, args.logos_dir, seed=int(args.seed), transparent_ratio=float(args.transparent_ratio),
                         multi_watermark_ratio=float(args.multi_watermark_ratio), max_watermarks=int(args.max_watermarks),
                         text_watermark_ratio=float(args.text_watermark_ratio), mixed_watermark_ratio=float(args.mixed_watermark_ratio),
                         fonts_dir=args.fonts_dir, texts_file=args.texts_file)
    if not torch.cuda.is_available():
        raise SystemExit("synth needs a HIP device (this path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    dirs = {k: os.path.join(args.output_dir, k) for k in ("watermarked", "clean") + (("masks",) if args.generate_mask else ())}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    pick = random.Random(f"uwm-synth-pick:{int(args.seed)}")
    bs = max(1, int(args.batch_size or 16))
    written = 0
    for b in range(0, int(args.count), bs):
        idx = list(range(b, min(b + bs, int(args.count))))
        which = [pick.randrange(len(ds)) for _ in idx]       # the script picks a clean image at random for every sample
        cleans, logos, jobs, planes, text_jobs, names, mixed = [], [], [], [], [], [], []
        for n, i in zip(idx, which):
            ds.set_epoch(n)                                   # sample n's draws: a function of (seed, n, clean image)
            clean = read_u8(ds.files[i], "RGB")
            transparent, _, lg, j, kind, pl, tj = ds.draw_sample(i, (clean.shape[1], clean.shape[0]))
            j = np.array(j, copy=True); j["logo"] += len(logos)
            tj = np.array(tj, copy=True); tj["glyph"] += len(planes)
            cleans.append(clean); logos += list(lg); jobs.append(j); planes += [a[..., None] for a in pl]; text_jobs.append(tj)
            mixed.append(len(pl) > 0 and bool((j["enabled"] != 0).any()))
            count = int((j["enabled"] != 0).sum())
            prefix = "multi_" if kind == "logo" and count > 1 else "" if kind == "logo" else kind + "_"
            names.append(f"{prefix}{'trans' if transparent else 'norm'}_{n:06d}")
        pc, dc, _ = pack_images(cleans)
        out, mask = pc.to(device), None
        if logos:
            pl, dl, _ = pack_images(logos)
            out, mask = device_synth(out, dc, pl.to(device), dl, np.stack(jobs), with_mask=bool(args.generate_mask), inplace=True)
        if quality and any(mixed):                            # the temporary file between the logos and the text of a mixed sample
            out = device_jpeg_ragged(out, dc, np.where(mixed, quality, 0), inplace=True)
        if planes:
            pp, dp, _ = pack_images(planes)
            out, mask = device_synth_text(out, dc, pp.to(device), dp, np.stack(text_jobs), inplace=True, mask_mode=1,
                                          masks=(mask if mask is not None else True) if args.generate_mask else None)
        if quality:                                           # the save of the finished sample
            out = device_jpeg_ragged(out, dc, np.full(len(idx), quality), inplace=True)
        out = out.cpu().numpy()
        mask = mask.cpu().numpy() if mask is not None else None
        for name, clean, d, m in zip(names, cleans, dc, mask_descs_for(dc)):
            o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
            Image.fromarray(out[o:o + h * w * 3].reshape(h, w, 3)).save(os.path.join(dirs["watermarked"], name + ".png"))
            Image.fromarray(clean).save(os.path.join(dirs["clean"], name + ".png"))
            if mask is not None:
                mo = int(m["offset"])
                Image.fromarray(mask[mo:mo + h * w].reshape(h, w)).save(os.path.join(dirs["masks"], name + ".png"))
            written += 1
    print(f"wrote {written} samples to {args.output_dir} (watermarked/, clean/{', masks/' if args.generate_mask else ''})")
    return dict(written=written, output=args.output_dir)


def filter_command(args):
    """The reference's src/scripts/watermark_filter.py on the device: one line per kept or moved file, then the stats."""
    from .filter import WatermarkFilter
    if not os.path.isdir(args.input):
        raise SystemExit(f"filter: input directory not found: {args.input}")
    if not os.path.exists(args.model):
        raise SystemExit(f"filter: model file not found: {args.model}")
    if args.config and not os.path.exists(args.config):
        raise SystemExit(f"filter: config file not found: {args.config}")
    if not torch.cuda.is_available():
        raise SystemExit("filter needs a HIP device (this path has no CPU fallback)")
    cfg = get_cfg_defaults()
    if args.config:
        update_config(cfg, args.config)
    if args.encoder:
        cfg.MODEL.ENCODER_NAME = args.encoder
    flt = WatermarkFilter(args.model, None, "cuda", args.threshold, args.batch_size, config=cfg)
    stats = flt.filter_images(args.input, args.no_watermark_dir, args.dry_run, args.delete)
    print("=" * 50)
    print(f"total: {stats['total']}  with watermark: {stats['with_watermark']}  without: {stats['without_watermark']}  "
          f"moved/deleted: {stats['moved']}  errors: {stats['errors']}")
    if args.dry_run:
        print("dry run: no file was touched")
    elif not args.no_watermark_dir and not args.delete:
        print("report only: give --no-watermark-dir DIR to move the images without a watermark, or --delete to delete them")
    return stats


def select_command(args):
    """The reference's src/scripts/model_selector.py on the device: every checkpoint on a seeded sample of images, then the summary."""
    from .select import ModelSelector
    if not os.path.exists(args.input):
        raise SystemExit(f"select: input path not found: {args.input}")
    if not os.path.exists(args.model):
        raise SystemExit(f"select: model path not found: {args.model}")
    if args.config and not os.path.exists(args.config):
        raise SystemExit(f"select: config file not found: {args.config}")
    if not torch.cuda.is_available():
        raise SystemExit("select needs a HIP device (this path has no CPU fallback)")
    cfg = get_cfg_defaults()
    if args.config:
        update_config(cfg, args.config)
    if args.encoder:
        cfg.MODEL.ENCODER_NAME = args.encoder
    sel = ModelSelector(args.input, args.model, args.output, args.num_samples, cfg, args.mask_type, args.batch_size, args.seed, args.save_masks)
    return sel.run_evaluation()


def enhance_masks_command(args):
    """The reference's src/scripts/enhance_masks.py (enhance_mask over a folder) on the device: every .png / .jpg / .jpeg of --mask-dir
    through postprocess.enhance_masks_ragged, --batch-size files per call, written under the same name to --output-dir, or over the
    input with --in-place.  One line per file with the foreground share before and after (from the call's stats)."""
    import numpy as np
    from PIL import Image
    from .data import DESC_DTYPE, mask_descs_for
    from .postprocess import enhance_masks_ragged
    if not os.path.isdir(args.mask_dir):
        raise SystemExit(f"enhance-masks: mask directory not found: {args.mask_dir}")
    out_dir = args.mask_dir if args.in_place else args.output_dir
    if not args.in_place and os.path.realpath(out_dir) == os.path.realpath(args.mask_dir):
        raise SystemExit("enhance-masks: --output-dir is the mask directory: overwriting the masks needs --in-place")
    if not torch.cuda.is_available():
        raise SystemExit("enhance-masks needs a HIP device (this path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    files = sorted(f for f in os.listdir(args.mask_dir) if f.endswith((".png", ".jpg", ".jpeg")))        # the script's filter
    os.makedirs(out_dir, exist_ok=True)
    bs = max(1, int(args.batch_size or 16))
    written = unreadable = 0
    for b in range(0, len(files), bs):
        names, masks = [], []
        for f in files[b:b + bs]:
            try:
                with Image.open(os.path.join(args.mask_dir, f)) as im:
                    masks.append(np.asarray(im if im.mode == "L" else im.convert("L"), dtype=np.uint8))
                names.append(f)
            except Exception as e:                                 # counted and left alone
                unreadable += 1
                print(f"{f}: unreadable ({e.__class__.__name__}), left as it is")
        if not names:
            continue
        descs = np.zeros(len(masks), DESC_DTYPE)
        descs["h"], descs["w"] = [m.shape[0] for m in masks], [m.shape[1] for m in masks]
        descs = mask_descs_for(descs)                              # the masks back to back
        flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in masks])).to(device)
        out, stats = enhance_masks_ragged(flat, descs, args.expand_pixels, args.blur_kernel, args.smooth_iterations, return_stats=True)
        out = out.cpu().numpy()
        for f, d, row in zip(names, descs, stats.cpu().tolist()):
            o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
            Image.fromarray(out[o:o + h * w].reshape(h, w)).save(os.path.join(out_dir, f))
            print(f"{f}: foreground {row[0] / row[2]:.4f} -> {row[1] / row[2]:.4f}")
            written += 1
    print(f"wrote {written} enhanced masks to {out_dir} (expand {args.expand_pixels}, blur {args.blur_kernel}, smooth "
          f"{args.smooth_iterations}); {unreadable} unreadable")
    return dict(written=written, unreadable=unreadable, output=out_dir)


def extract_command(args):
    """The reference's extract_watermarks.py on the device: transparent RGBA cut-outs of the watermark regions of every
    clean / watermarked pair, written where `--logos-dir` of `synth` and `train --synthesize` can read them."""
    from .extract import WatermarkExtractor
    for flag, d in (("--clean-dir", args.clean_dir), ("--watermarked-dir", args.watermarked_dir)):
        if not os.path.isdir(d):
            raise SystemExit(f"extract: {flag} not found: {d}")
    if not torch.cuda.is_available():
        raise SystemExit("extract needs a HIP device (this path has no CPU fallback)")
    ex = WatermarkExtractor(args.clean_dir, args.watermarked_dir, args.output_dir, args.threshold, args.min_area, args.batch_size)
    res = ex.process_all_images(args.limit, args.seed)
    print(f"processed {res['processed']} pairs: {res['extracted']} yielded cut-outs, {res['written']} files written to {args.output_dir}, "
          f"{res['errors']} errors")
    return res


def _evaluate_dirs(args):
    """the two input forms of `evaluate`: --input with --masks, or --data-dir D for D/watermarked and D/masks"""
    pair = args.input is not None or args.masks is not None
    if pair and args.data_dir is not None:
        raise SystemExit("evaluate: give --input with --masks, or --data-dir, not both")
    if not pair and args.data_dir is None:
        raise SystemExit("evaluate: give --input with --masks, or --data-dir")
    if pair and (args.input is None or args.masks is None):
        raise SystemExit("evaluate: --input and --masks go together")
    if pair:
        return args.input, args.masks
    return os.path.join(args.data_dir, "watermarked"), os.path.join(args.data_dir, "masks")


def evaluate_command(args):
    """Score the masks a checkpoint predicts for a labelled folder at each image's own size: the reference's five metrics and Boundary
    IoU, micro (counts summed) and image-wise (values averaged); evaluate.py, DESIGN.md 8s.  Every refusal comes before anything is
    created."""
    from .evaluate import Evaluator, check_settings, format_summary, write_json
    input_dir, masks_dir = _evaluate_dirs(args)
    try:
        check_settings(args.mask_type, args.text_enhance, args.tile, args.tile_overlap,
                       0.02 if args.boundary_ratio is None and args.boundary_pixels is None else args.boundary_ratio, args.boundary_pixels,
                       args.batch_size, args.limit, args.tta)
    except ValueError as e:
        raise SystemExit(f"evaluate: {e}")
    for flag, d in (("the image directory", input_dir), ("the mask directory", masks_dir)):
        if not os.path.isdir(d):
            raise SystemExit(f"evaluate: {flag} not found: {d}")
    if not os.path.exists(args.model):
        raise SystemExit(f"evaluate: model file not found: {args.model}")
    if args.config and not os.path.exists(args.config):
        raise SystemExit(f"evaluate: config file not found: {args.config}")
    if not torch.cuda.is_available():
        raise SystemExit("evaluate needs a HIP device (this path has no CPU fallback)")
    cfg = get_cfg_defaults()
    if args.config:
        update_config(cfg, args.config)
    ev = Evaluator(input_dir, masks_dir, args.model, None, args.mask_type, args.text_enhance, args.tile, args.tile_overlap, args.boundary_ratio,
                   args.boundary_pixels, args.batch_size, args.limit, args.seed, config=cfg, tta=args.tta, surface=args.surface_distance)
    ev.settings["config"] = args.config
    res = ev.run(per_image=args.per_image)
    print(format_summary(res))
    if args.output:
        write_json(res, args.output)
        print(f"wrote {args.output}")
    return res


def repair_command(args):
    """Predict the watermark mask of every image of a folder and fill it on the device (or fill given masks): repair.py, DESIGN.md 8v.
    Every refusal comes before anything is created."""
    from .repair import check_settings, format_counts, repair_folder
    try:
        check_settings(args.model, args.masks, args.mask_type, args.text_enhance, args.tile, args.tile_overlap, args.tta, args.cycles,
                       args.batch_size, args.limit)
    except ValueError as e:
        raise SystemExit(f"repair: {e}")
    for what, d in (("the image directory", args.input), ("the mask directory", args.masks)):
        if d is not None and not os.path.isdir(d):
            raise SystemExit(f"repair: {what} not found: {d}")
    if args.model is not None and not os.path.exists(args.model):
        raise SystemExit(f"repair: model file not found: {args.model}")
    if args.config and not os.path.exists(args.config):
        raise SystemExit(f"repair: config file not found: {args.config}")
    if not torch.cuda.is_available():
        raise SystemExit("repair needs a HIP device (this path has no CPU fallback)")
    pred = None
    if args.model is not None:
        cfg = get_cfg_defaults()
        if args.config:
            update_config(cfg, args.config)
        cfg.PREDICT.BATCH_SIZE = int(args.batch_size)
        pred = WatermarkPredictor(args.model, None, cfg, device="cuda")
    res = repair_folder(args.input, args.output, pred, args.masks, args.mask_type, args.text_enhance, args.tile, args.tile_overlap, args.tta,
                        args.cycles, args.save_masks, args.limit, args.seed, args.batch_size)
    print(format_counts(res))
    return res


def build_parser():
    ap = argparse.ArgumentParser(description="MI355X-native U-Net watermark segmentation (train | masks | enhance-masks | extract | filter | select | evaluate | predict)")
    sub = ap.add_subparsers(dest="command")
    tp = sub.add_parser("train")
    tp.add_argument("--config", type=str, default=None)
    tp.add_argument("--device", type=str, default="auto")
    tp.add_argument("--data-dir", type=str); tp.add_argument("--output-dir", type=str)
    tp.add_argument("--model-save-path", type=str); tp.add_argument("--batch-size", type=int)
    tp.add_argument("--epochs", type=int); tp.add_argument("--lr", type=float)
    tp.add_argument("--no-early-stopping", action="store_true")
    tp.add_argument("--early-stopping-patience", type=int)
    tp.add_argument("--resume", type=str)
    tp.add_argument("--use-blurred-mask", action="store_true",
                    help="accepted for compatibility where every mask is a file (it only concerns generated masks); refused on a dataset "
                         "that needs masks derived from watermarked / clean pairs: only the reference's exact rule is served")
    tp.add_argument("--encoder", type=str); tp.add_argument("--img-size", type=int)
    tp.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images instead of DATA.ROOT_DIR")
    tp.add_argument("--workers", type=int, default=2)
    tp.add_argument("--augment", choices=["none", "basic", "config"], default="none",
                    help="'basic' = the device input path: workers only decode, the device resizes (cv2's rule), augments with the "
                         "reference's basic recipe (flips, rot90, ShiftScaleRotate, RandomBrightnessContrast, HueSaturationValue) and "
                         "normalises; validation is resized and normalised only.  'config' = the same path with the recipe that "
                         "DATA.AUGMENTATION_TYPE names: 'enhanced' adds CLAHE / gamma, Gaussian noise and motion / Gaussian blur; "
                         "'transparent_watermark' (the config's default) adds a sheared Affine, noise, blur and ImageCompression and is "
                         "served only with --jpeg device.  'none' (default) = host-prepared tensors, no augmentation")
    tp.add_argument("--jpeg", choices=["refuse", "device"], default="refuse",
                    help="ImageCompression of the 'transparent_watermark' recipe (read by --augment config): 'device' = a baseline "
                         "libjpeg round trip (4:2:0, integer DCT, no entropy coding) on the device, bit-equal to Pillow / OpenCV; "
                         "'refuse' (default) = that recipe is refused")
    tp.add_argument("--augmentation-type", choices=["basic", "enhanced", "transparent_watermark"], default=None,
                    help="DATA.AUGMENTATION_TYPE (read by --augment config)")
    tp.add_argument("--model", choices=["Unet", "UnetPlusPlus"], default=None, help="MODEL.NAME (reference default: UnetPlusPlus)")
    tp.add_argument("--grad-clip", action="store_true", help="honour TRAIN.GRADIENT_CLIP (the reference defines but never applies it)")
    tp.add_argument("--optimizer", choices=["Adam", "AdamW", "SGD"], default=None, help="OPTIMIZER.NAME")
    tp.add_argument("--global-dice", action="store_true",
                    help="data-parallel runs: Dice of the GLOBAL batch (loss sums all-reduced) instead of the mean of per-rank Dice losses")
    tp.add_argument("--focal-weight", type=str, default=None, metavar="config|FLOAT",
                    help="LOSS.NAME CombinedLoss: add a focal term (smp's FocalLoss with LOSS.FOCAL_ALPHA / LOSS.FOCAL_GAMMA) to the BCE + Dice "
                         "sum, weighted by LOSS.FOCAL_WEIGHT ('config') or by the number given; absent (default) = no focal term, as in the "
                         "reference's trainer")
    tp.add_argument("--lr-scheduler", choices=["ReduceLROnPlateau", "CosineAnnealingLR", "CosineAnnealingWarmRestarts", "none"],
                    default=None, help="OPTIMIZER.LR_SCHEDULER")
    tp.add_argument("--checkpoint-dir", type=str, default=None, help="TRAIN.CHECKPOINT_DIR")
    tp.add_argument("--synthesize", action="store_true",
                    help="make the training pairs on the device: paste logos of --logos-dir onto the images of --clean-dir with the logo "
                         "branch of the reference's gen_data.py (resize, rotate, stretch, shear, blur, defects, colour, opacity), new samples "
                         "every epoch; needs --augment basic|config")
    tp.add_argument("--clean-dir", type=str, default=None, help="--synthesize: directory of clean images")
    tp.add_argument("--logos-dir", type=str, default=None,
                    help="--synthesize: directory of logos, with combined/, independent/ and car_logo/ as in the reference, or flat")
    tp.add_argument("--transparent-ratio", type=float, default=0.6, help="--synthesize: share of samples with low-opacity logos")
    tp.add_argument("--multi-watermark-ratio", type=float, default=0.4, help="--synthesize: share of samples with several logos")
    tp.add_argument("--synth-max-watermarks", type=int, default=3, help="--synthesize: most logos on one image (1..3)")
    tp.add_argument("--synth-mask", choices=["pair", "alpha"], default="pair",
                    help="--synthesize: 'pair' (default) derives the mask from (synthesized, clean) as the reference's dataset does; 'alpha' "
                         "takes the pasted alpha planes, which the reference binarises at 127, so low-opacity samples get nearly empty masks")
    tp.add_argument("--synth-seed", type=int, default=42, help="--synthesize: seed of the draws")
    _add_text_arguments(tp, "--synthesize: ")
    tp.add_argument("--synth-jpeg-quality", type=int, default=0, help="--synthesize: " + _JPEG_QUALITY_HELP)
    sp = sub.add_parser("synth", help="write logo-, text- and mixed-watermarked samples (the reference's scripts/gen_data.py) made on the device")
    sp.add_argument("--clean-dir", type=str, required=True)
    sp.add_argument("--logos-dir", type=str, default=None, help="directory of logos (required unless --text-watermark-ratio 1)")
    sp.add_argument("--output-dir", type=str, required=True); sp.add_argument("--count", type=int, required=True)
    sp.add_argument("--generate-mask", action="store_true", help="also write the pasted alpha planes to masks/ (a mixed sample: the logos' plane halved, then the maximum with the text's)")
    sp.add_argument("--seed", type=int, default=42)
    sp.add_argument("--transparent-ratio", type=float, default=0.6); sp.add_argument("--multi-watermark-ratio", type=float, default=0.4)
    sp.add_argument("--max-watermarks", type=int, default=3); sp.add_argument("--batch-size", type=int, default=None)
    _add_text_arguments(sp, "")
    sp.add_argument("--jpeg-quality", type=int, default=0, help=_JPEG_QUALITY_HELP + "; the files stay PNG, so they hold exactly these pixels")
    mp = sub.add_parser("masks", help="derive masks/<stem>.png from watermarked / clean pairs on the device, for every pair without one")
    mp.add_argument("--data-dir", type=str, default=None, help="DATA.ROOT_DIR: the directory with watermarked/, clean/ and masks/")
    mp.add_argument("--config", type=str, default=None)
    mp.add_argument("--threshold", type=int, default=None, help="DATA.GENERATE_MASK_THRESHOLD (0..255)")
    mp.add_argument("--batch-size", type=int, default=None, help="pairs per launch (default 16)")
    ep = sub.add_parser("enhance-masks", help="round and enlarge the masks of a folder (the reference's scripts/enhance_masks.py) on the device",
                        description="enhance_mask of the reference's script for every .png / .jpg / .jpeg of --mask-dir: grey close, dilate "
                                    "by --expand-pixels, Gaussian blur, threshold, smoothing; each result is written under the same name.  "
                                    "The defaults are the function's (10 / 15 / 2); the script's main() uses 15 / 21 and overwrites "
                                    "data/train/masks, which here needs --in-place.  Single-channel 8-bit files are read exactly; a colour "
                                    "file is converted by Pillow's 'L' rule, not by OpenCV's.  An unreadable file is counted and left alone.")
    ep.add_argument("--mask-dir", type=str, required=True, help="the folder of masks")
    dst = ep.add_mutually_exclusive_group(required=True)
    dst.add_argument("--output-dir", type=str, default=None, help="where the enhanced masks go")
    dst.add_argument("--in-place", action="store_true", help="overwrite the masks of --mask-dir (never done without this flag)")
    ep.add_argument("--expand-pixels", type=int, default=10, help="radius of the dilation, 0..31")
    ep.add_argument("--blur-kernel", type=int, default=15, help="side of the Gaussian, 0..63 (0: no blur; an even value is raised by one)")
    ep.add_argument("--smooth-iterations", type=int, default=2, help="open / close E(5,5) rounds, 0..8")
    ep.add_argument("--batch-size", type=int, default=16, help="masks per call")
    xp = sub.add_parser("extract", help="cut the watermarks out of clean / watermarked pairs as transparent PNGs (the reference's extract_watermarks.py)",
                        description="Compare every pair of --clean-dir and --watermarked-dir on the device, find the watermark regions "
                                    "(difference, threshold, closing and opening, filled outer contours, area above --min-area), and write "
                                    "each cluster of regions as an enhanced RGBA cut-out: <stem>_watermark.png, or <stem>_watermark_partK.png "
                                    "where the regions lie further apart than a quarter of the diagonal.  Departures from the reference's "
                                    "script: pairs are matched by stem over jpg, jpeg, png, bmp, tiff and tif (the script globs *.jpg); "
                                    "--limit draws its sample from --seed; a pair that cannot be read counts under errors and stops "
                                    "nothing; parts are numbered in ascending order of their first pixel, not in OpenCV's contour order.")
    xp.add_argument("--clean-dir", type=str, required=True); xp.add_argument("--watermarked-dir", type=str, required=True)
    xp.add_argument("--output-dir", type=str, required=True)
    xp.add_argument("--threshold", type=int, default=30, help="least grey difference that counts as watermark (0..255)")
    xp.add_argument("--min-area", type=int, default=100, help="a region is kept when its contour area exceeds this")
    xp.add_argument("--limit", type=int, default=None, help="process a seeded random sample of this many pairs")
    xp.add_argument("--seed", type=int, default=0, help="seed of the --limit sample")
    xp.add_argument("--batch-size", type=int, default=16, help="pairs per device call")
    fp = sub.add_parser("filter", help="sort a folder by predicted watermark area (the reference's scripts/watermark_filter.py)",
                        description="Predict every image's watermark mask on the device and move away (or delete) the images whose mask "
                                    "covers less than --threshold of the image.  Two deliberate departures from the reference's script: "
                                    "an image that cannot be read counts under 'errors' and stays where it is (the reference treats it "
                                    "as 'no watermark' and moves or deletes it), and files are deleted only with --delete (the reference "
                                    "deletes whenever no target directory is given); with neither --no-watermark-dir nor --delete the "
                                    "run only reports.")
    fp.add_argument("--input", type=str, required=True, help="the folder of images (jpg, jpeg, png, bmp, tiff, tif; either letter case)")
    fp.add_argument("--model", type=str, required=True); fp.add_argument("--config", type=str, default=None)
    fp.add_argument("--encoder", type=str)
    fp.add_argument("--threshold", type=float, default=0.0001, help="least share of watermark pixels that keeps an image (the script's default)")
    act = fp.add_mutually_exclusive_group()
    act.add_argument("--no-watermark-dir", type=str, default=None, help="move the images without a watermark here")
    act.add_argument("--delete", action="store_true", help="delete the images without a watermark (never done without this flag)")
    fp.add_argument("--dry-run", action="store_true", help="report what would be moved or deleted; touch nothing")
    fp.add_argument("--batch-size", type=int, default=None, help="images per captured call (default PREDICT.BATCH_SIZE)")
    lp = sub.add_parser("select", help="rank checkpoints on a seeded sample of images (the reference's scripts/model_selector.py)",
                        description="Run every .pth under --model on a seeded sample of the images under --input and write "
                                    "model_evaluation_results.json (the reference's keys) to --output: per image the watermark ratio and "
                                    "the component statistics of the post-processed mask, per model the detection rate (share of ratios "
                                    "above 0.001), and the model with the highest.  A batch is one captured call on the device and 64 bytes "
                                    "back per image.  Deliberate departures from the reference's script: masks are written only with "
                                    "--save-masks (the reference writes one PNG per image and model); an image that cannot be read is a "
                                    "failed prediction of every model, not fatal; a model is keyed by its path relative to --model (the "
                                    "reference keys by file name, so same-named files of different sub-directories overwrite each other); "
                                    "one process and one device, no worker processes.")
    lp.add_argument("--input", type=str, required=True, help="the folder of images (png, jpg, jpeg, bmp, tiff), or one image")
    lp.add_argument("--model", type=str, required=True, help="a directory searched recursively for .pth files, or one .pth file")
    lp.add_argument("--output", type=str, required=True, help="where model_evaluation_results.json (and the masks) go")
    lp.add_argument("--num-samples", type=int, default=100, help="images drawn with random.sample (the script's default)")
    lp.add_argument("--seed", type=int, default=42); lp.add_argument("--config", type=str, default=None)
    lp.add_argument("--encoder", type=str)
    lp.add_argument("--mask-type", choices=["watermark", "text", "mixed"], default="watermark",
                    help="the _optimize_mask type every mask goes through (predict_mask's default: watermark)")
    lp.add_argument("--batch-size", type=int, default=None, help="images per captured call (default PREDICT.BATCH_SIZE)")
    lp.add_argument("--save-masks", action="store_true", help="also write <image>_<model>_mask.png for every image and model")
    vp = sub.add_parser("evaluate", help="score the masks a checkpoint predicts against ground-truth masks, every image at its own size",
                        description="Predict the mask of every image of --input (or DATA-DIR/watermarked) on the device-resize path, with "
                                    "the post-processing, text enhancement or native-resolution tiling asked for, and count it against the "
                                    "mask of the same stem in --masks (or DATA-DIR/masks; > 127 is foreground) on the device.  Prints the "
                                    "reference's IoU, F1, accuracy, recall and precision (its get_metrics formulas; 0 / 0 gives 1) and "
                                    "Boundary IoU (Cheng et al., CVPR 2021), micro (counts summed over the images) and image-wise (values "
                                    "averaged).  An unreadable file, an image without a mask and a mask of another size count under "
                                    "'errors' and stop nothing.  The reference has no such command.")
    vp.add_argument("--input", type=str, default=None, help="the folder of images (jpg, jpeg, png, bmp, tiff, tif); with --masks")
    vp.add_argument("--masks", type=str, default=None, help="the folder of ground-truth masks, paired with the images by file stem")
    vp.add_argument("--data-dir", type=str, default=None, help="instead of --input and --masks: DIR/watermarked and DIR/masks")
    vp.add_argument("--model", type=str, required=True); vp.add_argument("--config", type=str, default=None)
    vp.add_argument("--mask-type", choices=["watermark", "text", "mixed"], default=None,
                    help="post-process every mask as the reference's _optimize_mask does for this type before it is scored (absent: raw "
                         "thresholded masks)")
    vp.add_argument("--text-enhance", action="store_true", help="the reference's _enhance_text_features in front of the network, as predict's")
    vp.add_argument("--tile", action="store_true", help="predict at native resolution from overlapping IMG_SIZE tiles, as predict's; not with --text-enhance")
    vp.add_argument("--tile-overlap", type=int, default=64, help="pixels neighbouring tiles share, 0 .. IMG_SIZE / 2 (with --tile)")
    vp.add_argument("--tta", choices=["none", "hflip", "flips", "d4"], default="none",
                    help="test-time augmentation as predict's --tta; the choice is recorded in the output JSON")
    vp.add_argument("--boundary-ratio", type=float, default=None,
                    help="Boundary IoU's distance as a share of the image diagonal, at least one pixel (default 0.02, the paper's)")
    vp.add_argument("--boundary-pixels", type=int, default=None, help="the same distance in pixels for every image, 0..32767 (0: no Boundary IoU); not with --boundary-ratio")
    vp.add_argument("--surface-distance", action="store_true",
                    help="also measure, in pixels, the Hausdorff distance, its 95th percentile (HD95), the average symmetric surface "
                         "distance and the covering radius (how far the predicted mask must be dilated by a Euclidean disc to cover "
                         "the truth) from exact distance transforms on the device; adds 'surface' to the output")
    vp.add_argument("--batch-size", type=int, default=16, help="pairs per device call")
    vp.add_argument("--limit", type=int, default=None, help="score a seeded random sample of this many pairs")
    vp.add_argument("--seed", type=int, default=0, help="seed of the --limit sample")
    vp.add_argument("--output", type=str, default=None, help="write settings, images, errors, micro and imagewise as JSON to this file")
    vp.add_argument("--per-image", action="store_true", help="add per_image to the JSON: path, size, radius, the eight counts, the six metrics")
    rp = sub.add_parser("repair", help="remove the watermarks of a folder: predict every mask and fill it on the device (the reference's repair)",
                        description="Predict the watermark mask of every image of --input as predict's device path does and fill it with "
                                    "the membrane (harmonic) interpolant on the device, or fill the masks of --masks (paired with the "
                                    "images by file stem; a byte != 0 is filled).  A smooth fill: it removes a logo from sky, wall, paper or "
                                    "skin and it smears texture; the reference's IOPaint / LaMa, OCR, diffusion and video steps are not "
                                    "served.  Results are written as <stem>.png.  An unreadable file, an image without a mask and a mask "
                                    "of another size count under 'errors' and stop nothing.")
    rp.add_argument("--input", type=str, required=True); rp.add_argument("--output", type=str, required=True)
    rp.add_argument("--model", type=str, default=None, help="the checkpoint that predicts the masks; or --masks")
    rp.add_argument("--masks", type=str, default=None, help="instead of --model: a folder of masks, paired with the images by file stem")
    rp.add_argument("--config", type=str, default=None)
    rp.add_argument("--mask-type", choices=["watermark", "text", "mixed"], default="watermark",
                    help="post-process every predicted mask as the reference's _optimize_mask does for this type (default watermark)")
    rp.add_argument("--text-enhance", action="store_true", help="the reference's _enhance_text_features in front of the network, as predict's")
    rp.add_argument("--tile", action="store_true", help="predict at native resolution from overlapping IMG_SIZE tiles, as predict's; not with --text-enhance")
    rp.add_argument("--tile-overlap", type=int, default=64, help="pixels neighbouring tiles share, 0 .. IMG_SIZE / 2 (with --tile)")
    rp.add_argument("--tta", choices=["none", "hflip", "flips", "d4"], default="none", help="test-time augmentation as predict's --tta")
    rp.add_argument("--cycles", type=int, default=None, help="V-cycles of the fill's multigrid solver, 0..32 (default 7: within half a grey level of the exact membrane)")
    rp.add_argument("--save-masks", type=str, default=None, help="also write the masks that were filled as DIR/<stem>.png")
    rp.add_argument("--limit", type=int, default=None, help="repair a seeded random sample of this many images")
    rp.add_argument("--seed", type=int, default=0, help="seed of the --limit sample")
    rp.add_argument("--batch-size", type=int, default=16, help="images per device call")
    pp = sub.add_parser("predict")
    pp.add_argument("--input", type=str, required=True); pp.add_argument("--output", type=str, required=True)
    pp.add_argument("--model", type=str, required=True); pp.add_argument("--config", type=str, default=None)
    pp.add_argument("--encoder", type=str); pp.add_argument("--threshold", type=float)
    pp.add_argument("--batch-size", type=int); pp.add_argument("--sigmoid", action="store_true")
    pp.add_argument("--mask-type", choices=["watermark", "text", "mixed"], default=None,
                    help="post-process every mask as the reference's _optimize_mask does for this watermark type (absent: raw thresholded masks)")
    pp.add_argument("--resize", choices=["host", "device"], default="host",
                    help="where images are resized to IMG_SIZE: 'device' = the reference's rule (cv2.resize INTER_LINEAR as A.Resize "
                         "does, restated in HIP; images of any size in one captured graph); 'host' (default) = PIL BILINEAR, which "
                         "widens its support on a downscale and so does NOT give the reference's pixels")
    pp.add_argument("--text-enhance", action="store_true",
                    help="run the reference's _enhance_text_features (CLAHE, Canny, dilate, x 1.2 on the edges, sharpen) on every image on "
                         "the device before the network sees it; needs --resize device.  Independent of --mask-type: the reference's "
                         "predict_text_watermark_mask is --mask-type text --text-enhance")
    pp.add_argument("--tile", action="store_true",
                    help="predict at native resolution: cut every image into overlapping IMG_SIZE x IMG_SIZE tiles on the device, run them "
                         "through the network --batch-size at a time and blend the tile logits into one mask at the image's own size "
                         "(no counterpart in the reference, which always resizes); needs --resize device, not with --text-enhance")
    pp.add_argument("--tile-overlap", type=int, default=64, help="pixels neighbouring tiles share, 0 .. IMG_SIZE / 2 (with --tile)")
    pp.add_argument("--tta", choices=["none", "hflip", "flips", "d4"], default="none",
                    help="test-time augmentation: the network sees every image (with --tile: every tile) under the views of the set -- "
                         "hflip: identity + horizontal flip; flips: + vertical flip and half turn; d4: all 8 flips and quarter turns -- "
                         "and the logit planes are mapped back and averaged on the device before the threshold (the mean of the logits, "
                         "not of the probabilities); k forwards per image; needs --resize device; composes with --tile, --mask-type and "
                         "--text-enhance where those compose")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.command == "train":
        return train_command(args)
    if args.command == "predict":
        return predict_command(args)
    if args.command == "masks":
        return masks_command(args)
    if args.command == "filter":
        return filter_command(args)
    if args.command == "synth":
        return synth_command(args)
    if args.command == "select":
        return select_command(args)
    if args.command == "enhance-masks":
        return enhance_masks_command(args)
    if args.command == "extract":
        return extract_command(args)
    if args.command == "evaluate":
        return evaluate_command(args)
    if args.command == "repair":
        return repair_command(args)
    ap.print_help()
