"""The draws of the augmentation recipes and of the logo-synthesis sampler, pinned to what they were when data.py was one file: the
other tests only check that one seed gives the same bytes twice, which a sampler with two columns swapped would still pass.

tests/golden/recipe_draws.npz holds the raw structured arrays, recorded at the commit before the data package with:

    import random, numpy as np, torch
    from unet_watermark_amd import data as D
    g = lambda s: torch.Generator().manual_seed(s)
    enh_p, enh_e = D.sample_aug_recipe(16, 48, 40, g(2), "enhanced")          # non-square, so rot90 is masked
    tw_p, tw_e, tw_q = D.sample_transparent_recipe(16, 48, 48, g(3))
    rng = random.Random("x")
    synth = np.stack([D.sample_synth_jobs(rng, (640, 480), [(100, 50), (30, 80)]) for _ in range(8)])
    np.savez_compressed("tests/golden/recipe_draws.npz", basic=D.sample_aug_params(16, 48, 48, g(1)), enhanced_params=enh_p,
                        enhanced_ext=enh_e, transparent_params=tw_p, transparent_ext=tw_e, transparent_quality=tw_q, synth=synth)

Every field is compared exactly, except the two groups whose values pass through libm's cos / sin / tan / pow and so may differ in
the last bit between two numpy builds: `minv` and `rot` to 1e-12 (the ulp effects of a dozen float64 operations are about 1e-15; a
wrong column or limit moves an entry by more than 1e-3), `lut2` to one count (a wrong gamma moves mid-table entries by several)."""
import os
import random

import numpy as np
import pytest
import torch

from unet_watermark_amd import data as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recipe_draws.npz")
CLOSE = ("minv", "rot")                   # np.allclose(rtol=1e-12, atol=1e-12)
WITHIN_ONE = ("lut2",)                    # max abs difference <= 1

# dir(data) without the dunder names, at the commit before the package
NAMES = ['AUG_DESC_DTYPE', 'AUG_EXT_DTYPE', 'AUG_HFLIP', 'AUG_RECIPES', 'AUG_RECIPES_EXT', 'AUG_VFLIP', 'BLUR_GAUSS', 'BLUR_MOTION',
         'BLUR_NONE', 'DESC_DTYPE', 'Dataset', 'DeviceInputPipeline', 'DeviceU8Dataset', 'FolderDataset', 'IDENTITY_MINV',
         'IMAGENET_MEAN', 'IMAGENET_STD', 'INTERP', 'JPEG_QUALITY_RANGE', 'LOGO_EXTENSIONS', 'LOGO_SUBDIRS', 'NOISE_SIGMA_MAX',
         'PAIR_IMAGE_EXTENSIONS', 'RawFolderDataset', 'RawPairDataset', 'RawSynthDataset', 'SYNTH_JOB_DTYPE', 'SYNTH_MAX_SIDE',
         'SYNTH_MAX_SLOTS', 'SYNTH_SLOTS', 'SyntheticWatermarkDataset', 'TONE_CLAHE', 'TONE_NONE', 'TONE_TABLE', '_AUG_COORD_LIMIT',
         '_EXT_WORKSPACE', '_JPEG_WORKSPACE', '_SYNTH_WORKSPACE', '_check_aug_ext_params', '_check_aug_params', '_ext_workspace',
         '_jpeg_workspace', '_overlap_area', '_plain_job', '_sample_effects', 'affine_inverse', 'annotations', 'aug_flags',
         'brightness_contrast_lut', 'clahe_clip_limit', 'descs_tensor', 'device_augment', 'device_jpeg', 'device_pair_mask',
         'device_preprocess', 'device_resize', 'device_synth', 'empty_synth_jobs', 'gamma_lut', 'identity_aug_ext_params',
         'identity_aug_params', 'list_collate', 'list_logos', 'mask_descs_for', 'motion_kernel', 'np', 'os', 'pack_images',
         'random_aug_flags', 'sample_aug_params', 'sample_aug_recipe', 'sample_synth_choice', 'sample_synth_jobs',
         'sample_transparent_recipe', 'stage_clean', 'synth_blur_params', 'synth_job_needs', 'synth_opacity_lut', 'synth_rotate_setup',
         'synth_shear_inverse', 'torch']


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _same_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype.names is None:
        assert np.array_equal(got, want), what
        return
    for name in want.dtype.names:
        g, w = got[name], want[name]
        if name in CLOSE:
            assert np.allclose(g, w, rtol=1e-12, atol=1e-12), f"{what}.{name}"
        elif name in WITHIN_ONE:
            assert int(np.abs(g.astype(np.int64) - w.astype(np.int64)).max()) <= 1, f"{what}.{name}"
        else:
            assert np.array_equal(g, w), f"{what}.{name}"


def test_basic_draws_are_the_recorded_ones(golden):
    _same_records(D.sample_aug_params(16, 48, 48, _gen(1)), golden["basic"], "basic")


def test_enhanced_draws_are_the_recorded_ones(golden):
    params, ext = D.sample_aug_recipe(16, 48, 40, _gen(2), "enhanced")
    _same_records(params, golden["enhanced_params"], "enhanced params")
    _same_records(ext, golden["enhanced_ext"], "enhanced ext")
    assert not ((params["flags"] >> 2) & 3).any()                  # non-square: rot90 is masked


def test_transparent_watermark_draws_are_the_recorded_ones(golden):
    params, ext, quality = D.sample_transparent_recipe(16, 48, 48, _gen(3))
    _same_records(params, golden["transparent_params"], "transparent_watermark params")
    _same_records(ext, golden["transparent_ext"], "transparent_watermark ext")
    _same_records(quality, golden["transparent_quality"], "transparent_watermark quality")
    assert quality.dtype == np.int32


def test_synth_job_draws_are_the_recorded_ones(golden):
    rng = random.Random("x")
    jobs = np.stack([D.sample_synth_jobs(rng, (640, 480), [(100, 50), (30, 80)]) for _ in range(8)])
    _same_records(jobs, golden["synth"], "synth jobs")


def test_the_recorded_draws_exercise_every_stage(golden):
    """a fixture in which a stage never fired would pin nothing about it"""
    e, t = golden["enhanced_ext"], golden["transparent_ext"]
    assert (e["tone"] == D.TONE_CLAHE).any() and (e["tone"] == D.TONE_TABLE).any()
    for ext in (e, t):
        assert (ext["noise_sigma"] > 0).any() and (ext["blur"] == D.BLUR_MOTION).any() and (ext["blur"] == D.BLUR_GAUSS).any()
    assert (golden["transparent_quality"] > 0).any() and (golden["transparent_quality"] == 0).any()
    for p in (golden["basic"], golden["enhanced_params"], golden["transparent_params"]):
        assert (p["minv"] != D.IDENTITY_MINV).any() and (p["lut"] != np.arange(256)).any() and (p["hue"] != 0).any()
    assert golden["synth"]["enabled"].any() and golden["synth"]["rotate"].any() and golden["synth"]["shear"].any()


def test_basic_through_sample_aug_recipe_is_sample_aug_params():
    params, ext = D.sample_aug_recipe(16, 48, 48, _gen(1), "basic")
    assert ext is None and params.tobytes() == D.sample_aug_params(16, 48, 48, _gen(1)).tobytes()


def test_sample_aug_recipe_still_refuses_what_it_refused():
    with pytest.raises(ValueError, match="draw it with sample_transparent_recipe"):
        D.sample_aug_recipe(2, 16, 16, _gen(0), "transparent_watermark")
    with pytest.raises(ValueError, match=r"unknown augmentation recipe 'x' \(served: basic, enhanced\)"):
        D.sample_aug_recipe(2, 16, 16, _gen(0), "x")
    with pytest.raises(ValueError, match=r"unknown augmentation recipe 'enhanced' \(served: basic\)"):
        D.sample_aug_params(2, 16, 16, _gen(0), "enhanced")


def test_every_name_of_the_single_file_module_is_still_there():
    assert len(NAMES) == 81
    missing = [n for n in NAMES if not hasattr(D, n)]
    assert not missing, missing
