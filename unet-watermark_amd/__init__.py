"""unet-watermark_amd — MI355X-native U-Net watermark-segmentation hot path.

Python host layer over libuwm.so (hand-written HIP for gfx950, C ABI in include/uwm.h):
`Unet` / `UnetPlusPlus` (smp drop-ins), Dice/BCE/Jaccard/Tversky/Focal/Combined losses, binary metrics, trainer / predictor.
Import name: `unet_watermark_amd` (alias package next to this directory).
"""
from . import _lib  # noqa: F401
from .model import Unet, UnetPlusPlus, create_model, create_model_from_config, SUPPORTED_MODELS  # noqa: F401
from .losses import DiceLoss, BCEWithLogitsLoss, CombinedLoss, get_loss_function  # noqa: F401
from .losses import JaccardLoss, TverskyLoss, FocalLoss, make_loss_spec, criterion_spec  # noqa: F401
from .metrics import (get_metrics, get_stats, micro_scores, logits_metrics, threshold_mask, resize_threshold,  # noqa: F401
                      dice_coef, iou_score)

__version__ = "0.1.0"

from .postprocess import optimize_mask, morphology, connected_components, structuring_element  # noqa: F401,E402
from .data import device_preprocess, aug_flags, random_aug_flags, pack_images, device_resize  # noqa: F401,E402
from .data import (device_augment, sample_aug_params, identity_aug_params, affine_inverse, brightness_contrast_lut,  # noqa: F401,E402
                   AUG_DESC_DTYPE)
from .data import (sample_aug_recipe, identity_aug_ext_params, gamma_lut, motion_kernel, clahe_clip_limit,  # noqa: F401,E402
                   AUG_EXT_DTYPE)
from .data import device_pair_mask, stage_clean, mask_descs_for, RawPairDataset  # noqa: F401,E402
from .data import device_synth, sample_synth_jobs, sample_synth_choice, RawSynthDataset, SYNTH_JOB_DTYPE  # noqa: F401,E402
from .data import device_synth_text, render_text_plane, sample_text_job, sample_synth_kind, TEXT_JOB_DTYPE  # noqa: F401,E402
from .filter import WatermarkFilter, filter_folder, batch_ratios, list_images  # noqa: F401,E402
from .postprocess import optimize_masks_ragged  # noqa: F401,E402
from .select import ModelSelector, run_selection  # noqa: F401,E402
from .extract import WatermarkExtractor, extract_regions, plan_cutouts, extract_cutouts  # noqa: F401,E402
from .textenh import enhance_text_features, text_enhance_ragged  # noqa: F401,E402
from .train import FusedAdam, FusedAdamW  # noqa: F401,E402
from .tiling import plan_tiles, plan_batch  # noqa: F401,E402
from .scoring import score_masks_ragged, boundary_radius, metrics_from_counts, summarize  # noqa: F401,E402
from .scoring import distance_transform_ragged, surface_distances_ragged, surface_from_record, summarize_surface  # noqa: F401,E402
from .evaluate import Evaluator  # noqa: F401,E402
from .inpaint import inpaint, inpaint_ragged, INPAINT_STATS_FIELDS  # noqa: F401,E402
from .tta import view_mask, view_codes, apply_view, invert_view, plan_slots, merge_views  # noqa: F401,E402
