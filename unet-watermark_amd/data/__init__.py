"""Minimal data side of the boundary: tensors with the contract of the reference's dataset
(/root/reference/src/utils/dataset.py:113-122,332-333,389-395) — image fp32 NCHW normalised with the
ImageNet mean/std, mask int64 {0,1} (H,W).  A synthetic generator and a plain PIL folder reader are provided (datasets); the
reference's basic and enhanced albumentations recipes run on the device (augment: device_augment; pipeline: DeviceInputPipeline;
`main.py train --augment basic` / `--augment config`), and so does the transparent_watermark recipe, whose ImageCompression is a
baseline JPEG round trip on the device (device_jpeg, sample_transparent_recipe; `--augment config --jpeg device`).
Images of any size travel as one packed buffer (ragged).  An image without a mask file gets the mask the reference derives from its
clean counterpart, also on the device (pairmask: device_pair_mask; RawPairDataset), and logo-watermarked samples are
synthesized there (synth: device_synth; RawSynthDataset), as are text and mixed ones (synthtext: device_synth_text;
DESIGN.md §8o); the JPEG save the reference ends its synthesis with runs there at each image's own size (jpegragged:
device_jpeg_ragged).
Every name is used as data.NAME; the modules below say where it lives."""
from __future__ import annotations

import os  # noqa: F401
from functools import partial as _partial

import numpy as np  # noqa: F401
import torch  # noqa: F401
from torch.utils.data import Dataset  # noqa: F401

from ..constants import IMAGENET_MEAN, IMAGENET_STD  # noqa: F401
from .._device import _WORKSPACE, workspace  # noqa: F401
from .ragged import DESC_DTYPE, INTERP, descs_tensor, device_resize, mask_descs_for, pack_images  # noqa: F401
from .augment import (AUG_DESC_DTYPE, AUG_EXT_DTYPE, AUG_HFLIP, AUG_RECIPES, AUG_RECIPES_EXT, AUG_VFLIP, BLUR_GAUSS, BLUR_MOTION,  # noqa: F401
                      BLUR_NONE, IDENTITY_MINV, JPEG_QUALITY_RANGE, NOISE_SIGMA_MAX, RECIPES, TONE_CLAHE, TONE_NONE, TONE_TABLE,
                      _AUG_COORD_LIMIT, _check_aug_ext_params, _check_aug_params, affine_inverse, aug_flags, brightness_contrast_lut,
                      clahe_clip_limit, device_augment, device_jpeg, device_preprocess, gamma_lut, identity_aug_ext_params,
                      identity_aug_params, motion_kernel, random_aug_flags, sample_aug_params, sample_aug_recipe, sample_recipe,
                      sample_transparent_recipe)
from .pairmask import device_pair_mask, stage_clean  # noqa: F401
from .jpegragged import SYNTH_JPEG_QUALITY, check_jpeg_quality, device_jpeg_ragged  # noqa: F401
from .synth import (SYNTH_JOB_DTYPE, SYNTH_MAX_SIDE, SYNTH_MAX_SLOTS, SYNTH_SLOTS, _overlap_area, _plain_job, _sample_effects,  # noqa: F401
                    device_synth, empty_synth_jobs, sample_synth_choice, sample_synth_jobs, synth_blur_params, synth_job_needs,
                    synth_opacity_lut, synth_rotate_setup, synth_shear_inverse)
from .synthtext import (DEFAULT_TEXTS, SYNTH_KINDS, TEXT_INKS, TEXT_JOB_DTYPE, TEXT_MARGIN, FontSet, device_synth_text,  # noqa: F401
                        empty_text_jobs, has_cjk, load_texts, render_text_plane, require_freetype, sample_font_size, sample_synth_kind,
                        sample_text, sample_text_item, sample_text_job, text_job_final_size, text_job_needs)
from .datasets import (LOGO_EXTENSIONS, LOGO_SUBDIRS, PAIR_IMAGE_EXTENSIONS, DeviceU8Dataset, FolderDataset, RawFolderDataset,  # noqa: F401
                       RawPairDataset, RawSynthDataset, SyntheticWatermarkDataset, list_collate, list_logos)
from .pipeline import DeviceInputPipeline  # noqa: F401

# the per-feature cache names of the single-file module: the three caches are the one dict of _device, keyed by (name, device)
_EXT_WORKSPACE = _JPEG_WORKSPACE = _SYNTH_WORKSPACE = _WORKSPACE
_ext_workspace, _jpeg_workspace = _partial(workspace, "augment_ext"), _partial(workspace, "jpeg")
