"""The Jaccard / Tversky / Focal losses, the part that needs no device: the closed-form gradients csrc/loss_ext.hip evaluates,
restated here in fp64 and held against autograd of the definitions (tests/loss_ext_ref.py); the new symbols of libuwm.so and their
argument checks, which fail before any launch; get_loss_function, CombinedLoss folding and the command line's loss selection."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ext_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_YAML = os.path.join(ROOT, "tests", "golden", "unet_text_watermark.yaml")
NEW = ("uwm_loss_ext", "uwm_loss_ext_sums", "uwm_loss_ext_apply")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


# ------------------------------------------------------------------------------------------------ the closed forms
def closed_form(x, t, q, npix_total=None, sums=None):
    """loss_ext.hip's arithmetic in fp64: ({term: value}, dtotal/dx).  Every region loss's gradient is s_i (ct t_i + c0)."""
    x, t = x.double(), t.double()
    p = torch.sigmoid(x)
    s = p * (1 - p)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    n = float(npix_total or x.numel())
    I, P, T = sums[:3] if sums is not None else (float((p * t).sum()), float(p.sum()), float(t.sum()))
    on = T > 0
    ct = c0 = 0.0
    out = {}
    # Dice
    sm, eps = q["dice_smooth"], q["dice_eps"]
    den = P + T + sm; denc = max(den, eps)
    out["dice"] = 1 - (2 * I + sm) / denc if on else 0.0
    if on:
        ct -= q["w_dice"] * 2 / denc; c0 += q["w_dice"] * ((2 * I + sm) / denc ** 2 if den > eps else 0.0)
    # Jaccard: g_i = -(A t_i - B (1 - t_i)) s_i
    sm, eps = q["jaccard_smooth"], q["jaccard_eps"]
    den = P + T - I + sm; denc = max(den, eps)
    out["jaccard"] = 1 - (I + sm) / denc if on else 0.0
    if on:
        A, B = 1 / denc, ((I + sm) / denc ** 2 if den > eps else 0.0)
        ct -= q["w_jaccard"] * (A + B); c0 += q["w_jaccard"] * B
    # Tversky: dscore_i = (t_i s_i denc - (I + sm) dden_i) / denc^2, dden_i = s_i (t_i + a (1 - t_i) - b t_i) or 0 when clamped
    sm, eps, a, b, g = (q[k] for k in ("tversky_smooth", "tversky_eps", "tversky_alpha", "tversky_beta", "tversky_gamma"))
    den = I + a * (P - I) + b * (T - I) + sm; denc = max(den, eps)
    base = max(1 - (I + sm) / denc, 0.0) if on else 0.0
    out["tversky"] = base ** g
    K = (1.0 if on else 0.0) if g == 1.0 else (g * base ** (g - 1) if base > 0 else 0.0)
    A, B = 1 / denc, ((I + sm) / denc ** 2 if den > eps else 0.0)
    ct -= q["w_tversky"] * K * (A - B * (1 - a - b)); c0 += q["w_tversky"] * K * B * a
    grad = s * (ct * t + c0) + q["w_bce"] / n * (p - t)
    out["bce"] = float(bce.sum()) / n if sums is None else sums[3] / n
    # Focal: (p - t) (1 - pt)^(g - 1) (g pt bce + (1 - pt)), evaluated as (p - t) (1 - pt)^g (g pt r + 1), r = bce / (1 - pt) -> 1
    fa, fg = q["focal_alpha"], q["focal_gamma"]
    om = -torch.expm1(-bce); pt = torch.exp(-bce)
    r = torch.where(om > 0, bce / torch.where(om > 0, om, torch.ones_like(om)), torch.ones_like(om))
    aw = fa * t + (1 - fa) * (1 - t) if fa is not None else torch.ones_like(t)
    out["focal"] = float((aw * om ** fg * bce).sum()) / n if sums is None else sums[4] / n
    grad = grad + q["w_focal"] / n * aw * (p - t) * om ** fg * (fg * pt * r + 1)
    out["total"] = sum(q["w_" + k] * out[k] for k in ("dice", "bce", "jaccard", "tversky", "focal"))
    return out, grad


SPECS = {
    "jaccard-smooth0": R.full_spec(w_jaccard=1.0),
    "jaccard-smooth1e-5": R.full_spec(w_jaccard=1.0, jaccard_smooth=1e-5),
    "tversky-default": R.full_spec(w_tversky=1.0),
    "tversky-0.3-0.7-1.5": R.full_spec(w_tversky=1.0, tversky_alpha=0.3, tversky_beta=0.7, tversky_gamma=1.5, tversky_smooth=1e-5),
    "focal-none-2": R.full_spec(w_focal=1.0),
    "focal-0.25-2.5": R.full_spec(w_focal=1.0, focal_alpha=0.25, focal_gamma=2.5),
    "focal-none-0.5": R.full_spec(w_focal=1.0, focal_gamma=0.5),
    "all-five": R.full_spec(w_dice=0.3, w_bce=0.2, w_jaccard=0.15, w_tversky=0.25, w_focal=0.4, dice_smooth=1e-5, jaccard_smooth=1e-5,
                            tversky_smooth=1e-5, tversky_alpha=0.3, tversky_beta=0.7, tversky_gamma=1.5, focal_alpha=0.25, focal_gamma=2.5),
}


def _inputs(seed=0, shape=(2, 1, 8, 8), density=0.2):
    g = torch.Generator().manual_seed(seed)
    x = 4.0 * torch.randn(shape, generator=g, dtype=torch.float64)
    t = (torch.rand(shape, generator=g) < density).double()
    return x, t


@pytest.mark.parametrize("name", sorted(SPECS))
def test_closed_form_gradients_match_autograd_of_the_definitions(name):
    q = SPECS[name]
    x, t = _inputs()
    ref, gref = R.loss_and_grad(x, t, q)
    got, g = closed_form(x, t, q)
    for k in R.TERMS:
        assert abs(got[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (k, got[k], ref[k])
    assert float((g - gref).abs().max()) <= 1e-12 * float(gref.abs().max()), name


@pytest.mark.parametrize("name", ["jaccard-smooth0", "tversky-0.3-0.7-1.5", "all-five"])
def test_an_empty_target_zeroes_the_region_losses_and_their_gradients(name):
    q = SPECS[name]
    x, _ = _inputs(1)
    t = torch.zeros_like(x)
    ref, gref = R.loss_and_grad(x, t, q)
    got, g = closed_form(x, t, q)
    assert ref["dice"] == ref["jaccard"] == ref["tversky"] == 0.0 and got["dice"] == got["jaccard"] == got["tversky"] == 0.0
    if q["w_bce"] == 0.0 and q["w_focal"] == 0.0:
        assert float(gref.abs().max()) == 0.0 and float(g.abs().max()) == 0.0 and ref["total"] == got["total"] == 0.0
    else:
        assert float((g - gref).abs().max()) <= 1e-12 * float(gref.abs().max())


def test_the_eps_clamp_drops_the_denominators_derivative():
    """a target that is 1e-9 at one pixel (logit -17), logits of -100 elsewhere and smooth = 0: T > 0 while every denominator sits
    under eps"""
    x = torch.full((1, 1, 5, 7), -100.0, dtype=torch.float64)
    t = torch.zeros_like(x); t[0, 0, 2, 3] = 1e-9; x[0, 0, 2, 3] = -17.0
    for name in ("jaccard-smooth0", "tversky-default"):
        q = SPECS[name]
        ref, gref = R.loss_and_grad(x, t, q)
        got, g = closed_form(x, t, q)
        assert abs(got["total"] - ref["total"]) <= 1e-12 and 0.99 < ref["total"] <= 1.0
        assert float((g - gref).abs().max()) <= 1e-12 * float(gref.abs().max()) and float(gref.abs().max()) > 0


def test_focal_gradient_stays_finite_where_one_minus_pt_vanishes():
    x = torch.tensor([100.0, -100.0, 30.0, -30.0, 800.0, -800.0, 100.0, -100.0], dtype=torch.float64).reshape(1, 1, 2, 4)
    t = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0], dtype=torch.float64).reshape(1, 1, 2, 4)
    for name in ("focal-none-0.5", "focal-0.25-2.5"):
        got, g = closed_form(x, t, SPECS[name])
        assert torch.isfinite(g).all() and all(v == v and abs(v) != float("inf") for v in got.values())
    # confident and right, confident and wrong, at the logits the device tests force: the reference itself stays finite there (its
    # BCE keeps softplus(-100) = 3.7e-44) and the closed form follows it
    x = torch.tensor([100.0, -100.0, 30.0, -30.0, 100.0, -100.0, 30.0, -30.0], dtype=torch.float64).reshape(1, 1, 2, 4)
    for name in ("focal-none-0.5", "focal-0.25-2.5", "all-five"):
        ref, gref = R.loss_and_grad(x, t, SPECS[name])
        got, g = closed_form(x, t, SPECS[name])
        assert torch.isfinite(gref).all() and float((g - gref).abs().max()) <= 1e-12 * float(gref.abs().max())
        assert abs(got["total"] - ref["total"]) <= 1e-12 * abs(ref["total"])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_new_symbols_are_exported_and_declared(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "uwm.h")).read()
    for name in NEW:
        assert name in L.SIGNATURES and getattr(lib, name) is not None
        assert name + "(" in header
    assert "typedef struct uwm_loss_spec" in header
    assert "loss_ext.hip" in L.SOURCES
    assert [f for f, _ in L.uwm_loss_spec._fields_] == list(R.SPEC_DEFAULTS) and C.sizeof(L.uwm_loss_spec) == 64


def _host_block():
    buf = (C.c_uint8 * 4096)()
    return buf, C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)


def _spec(L, **fields):
    from unet_watermark_amd.losses import make_loss_spec
    return make_loss_spec(w_jaccard=1.0, **fields)


BAD = [("logits", None), ("target", None), ("spec", None), ("scratch", None), ("loss_out", None), ("npix", 0), ("npix", -5),
       ("ld", 0), ("ldd", 0), ("tdt", 4), ("tdt", -1), ("tversky_gamma", 0.0), ("tversky_gamma", -1.0), ("tversky_gamma", float("nan")),
       ("focal_gamma", -0.5), ("focal_gamma", float("nan")), ("focal_alpha", 1.5), ("npix_total", 15)]


@pytest.mark.parametrize("what,value", BAD, ids=[f"{w}={v}" for w, v in BAD])
def test_argument_checks_return_an_error_before_any_launch(L, what, value):
    """every pointer here is host memory: a call that got as far as a launch would not return an error code with the entry
    point's own message"""
    lib = L.lib()
    keep, p = _host_block()
    a = dict(logits=p, ld=1, target=p, tdt=0, npix=16, npix_total=16, scratch=p, loss_out=p, dlogits=p, ldd=4, gs=1.0)
    fields = {}
    if what in a:
        a[what] = value
    elif what != "spec":
        fields[what] = value
    spec = None if what == "spec" else C.byref(_spec(L, **fields))
    calls = {
        "uwm_loss_ext": lambda: lib.uwm_loss_ext(a["logits"], a["ld"], a["target"], a["tdt"], a["npix"], spec, a["scratch"], a["loss_out"],
                                                 a["dlogits"], a["ldd"], a["gs"], None),
        "uwm_loss_ext_sums": lambda: lib.uwm_loss_ext_sums(a["logits"], a["ld"], a["target"], a["tdt"], a["npix"], spec, a["scratch"], None),
        "uwm_loss_ext_apply": lambda: lib.uwm_loss_ext_apply(a["logits"], a["ld"], a["target"], a["tdt"], a["npix"], a["npix_total"], spec,
                                                             a["scratch"], a["loss_out"], a["dlogits"], a["ldd"], a["gs"], None),
    }
    applies = {"loss_out": ("uwm_loss_ext", "uwm_loss_ext_apply"), "ldd": ("uwm_loss_ext", "uwm_loss_ext_apply"),
               "npix_total": ("uwm_loss_ext_apply",)}.get(what, NEW)
    for name in applies:
        assert calls[name]() != 0, name
        assert lib.uwm_last_error().decode().startswith(name + ":"), (name, lib.uwm_last_error().decode())


# ------------------------------------------------------------------------------------------------ the Python layer
def _cfg(name=None, yaml=None):
    from unet_watermark_amd.config import get_cfg_defaults, update_config
    cfg = get_cfg_defaults()
    if yaml:
        update_config(cfg, yaml)
    if name:
        cfg.LOSS.NAME = name
    return cfg


def test_get_loss_function_serves_the_references_names(L):
    import unet_watermark_amd as U
    cfg = _cfg("JaccardLoss"); cfg.LOSS.SMOOTH = 3e-4
    j = U.get_loss_function(cfg)
    assert type(j) is U.JaccardLoss and (j.mode, j.smooth, j.eps) == ("binary", 3e-4, 1e-7)
    cfg.LOSS.NAME = "TverskyLoss"
    t = U.get_loss_function(cfg)
    assert type(t) is U.TverskyLoss and (t.smooth, t.eps, t.alpha, t.beta, t.gamma) == (3e-4, 1e-7, 0.5, 0.5, 1.0)
    cfg.LOSS.NAME = "FocalLoss"; cfg.LOSS.FOCAL_ALPHA = 0.25; cfg.LOSS.FOCAL_GAMMA = 2.5
    f = U.get_loss_function(cfg)
    assert type(f) is U.FocalLoss and (f.alpha, f.gamma) == (None, 2.0)          # the reference passes mode alone
    cfg.LOSS.NAME = "LovaszLoss"
    with pytest.raises(ValueError, match="LovaszLoss"):
        U.get_loss_function(cfg)
    cfg.LOSS.NAME = "HingeLoss"
    with pytest.raises(ValueError):
        U.get_loss_function(cfg)


def test_unsupported_constructor_options_raise(L):
    import unet_watermark_amd as U
    for cls, kw in [(U.JaccardLoss, dict(mode="multiclass")), (U.JaccardLoss, dict(log_loss=True)), (U.JaccardLoss, dict(from_logits=False)),
                    (U.JaccardLoss, dict(classes=[0])), (U.TverskyLoss, dict(mode="multilabel")), (U.TverskyLoss, dict(ignore_index=255)),
                    (U.TverskyLoss, dict(log_loss=True)), (U.TverskyLoss, dict(gamma=0.0)), (U.FocalLoss, dict(mode="multiclass")),
                    (U.FocalLoss, dict(normalized=True)), (U.FocalLoss, dict(reduced_threshold=0.5)), (U.FocalLoss, dict(reduction="sum")),
                    (U.FocalLoss, dict(ignore_index=0)), (U.FocalLoss, dict(gamma=-1.0)), (U.FocalLoss, dict(alpha=1.5))]:
        with pytest.raises(ValueError):
            cls(**kw)
    assert U.TverskyLoss("binary", alpha=0.3, beta=0.7, gamma=1.5).spec_fields(2.0)["tversky_beta"] == 0.7
    with pytest.raises(RuntimeError, match="HIP device"):
        U.FocalLoss()(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))              # no CPU fallback


def test_combined_loss_folds_the_five_kinds_into_one_spec(L):
    import unet_watermark_amd as U
    from unet_watermark_amd.losses import spec_needs_ext
    second = U.JaccardLoss(smooth=1.0)
    crit = U.CombinedLoss([U.BCEWithLogitsLoss(), U.DiceLoss(smooth=1e-5), U.JaccardLoss(smooth=2e-5), U.TverskyLoss(alpha=0.3, beta=0.7, gamma=1.5),
                           U.FocalLoss(alpha=0.25, gamma=2.5), U.BCEWithLogitsLoss(), second], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7])
    fields, rest = crit.fold()
    assert rest == [(second, 0.7)]
    assert fields == dict(w_dice=0.2, w_bce=0.7, dice_smooth=1e-5, dice_eps=1e-7, w_jaccard=0.3, jaccard_smooth=2e-5, jaccard_eps=1e-7,
                          w_tversky=0.4, tversky_smooth=0.0, tversky_eps=1e-7, tversky_alpha=0.3, tversky_beta=0.7, tversky_gamma=1.5,
                          w_focal=0.5, focal_alpha=0.25, focal_gamma=2.5)
    with pytest.raises(ValueError, match="second"):
        U.criterion_spec(crit)
    spec = U.criterion_spec(U.CombinedLoss(crit.losses[:6], crit.weights[:6]))
    assert spec_needs_ext(spec) and abs(spec.w_bce - 0.7) < 1e-7 and abs(spec.focal_gamma - 2.5) < 1e-7
    plain = U.criterion_spec(U.CombinedLoss([U.BCEWithLogitsLoss(), U.DiceLoss(smooth=1e-5)], [0.5, 0.5]))
    assert not spec_needs_ext(plain) and U.make_loss_spec(w_focal=1.0).focal_alpha == -1.0
    with pytest.raises(ValueError, match="unknown"):
        U.make_loss_spec(w_lovasz=1.0)


def test_the_command_line_selects_the_loss(L):
    from unet_watermark_amd import cli
    ap = cli.build_parser()
    plain = ap.parse_args(["train"])
    assert plain.focal_weight is None
    # the three names served before: no spec, the same weights as ever
    for name, weights in [("DiceLoss", (1.0, 0.0)), ("BCEWithLogitsLoss", (0.0, 1.0)), ("CombinedLoss", (0.5, 0.5))]:
        cfg = _cfg(name)
        assert cli._loss_spec(cfg, plain) is None and cli._loss_weights(cfg) == weights
    text = _cfg(yaml=TEXT_YAML)
    assert cli._loss_weights(text) == (0.5, 0.3) and cli._loss_spec(text, plain) is None
    with pytest.raises(ValueError, match="unsupported LOSS.NAME"):
        cli._loss_weights(_cfg("JaccardLoss"))
    # the three new names
    for name, field in [("JaccardLoss", "w_jaccard"), ("TverskyLoss", "w_tversky"), ("FocalLoss", "w_focal")]:
        spec = cli._loss_spec(_cfg(name), plain)
        assert getattr(spec, field) == 1.0 and sum(getattr(spec, w) for w in ("w_dice", "w_bce", "w_jaccard", "w_tversky", "w_focal")) == 1.0
    assert abs(cli._loss_spec(_cfg("JaccardLoss"), plain).jaccard_smooth - 1e-5) < 1e-12
    with pytest.raises(ValueError, match="LovaszLoss"):
        cli._loss_spec(_cfg("LovaszLoss"), plain)
    # --focal-weight config: the text-watermark recipe's 0.2 / 0.25 / 2.5
    spec = cli._loss_spec(text, ap.parse_args(["train", "--focal-weight", "config"]))
    got = [spec.w_dice, spec.w_bce, spec.w_focal, spec.focal_alpha, spec.focal_gamma, spec.dice_smooth, spec.w_jaccard, spec.w_tversky]
    assert got == pytest.approx([0.5, 0.3, 0.2, 0.25, 2.5, 1e-6, 0.0, 0.0], rel=1e-6)
    crit = cli._criterion(text, ap.parse_args(["train", "--focal-weight", "0.35"]))
    assert [type(m).__name__ for m in crit.losses] == ["BCEWithLogitsLoss", "DiceLoss", "FocalLoss"] and crit.weights == [0.3, 0.5, 0.35]
    with pytest.raises(ValueError, match="FOCAL_WEIGHT"):
        cli._loss_spec(_cfg("CombinedLoss"), ap.parse_args(["train", "--focal-weight", "config"]))
    with pytest.raises(ValueError, match="CombinedLoss"):
        cli._loss_spec(_cfg("DiceLoss"), ap.parse_args(["train", "--focal-weight", "0.2"]))
    with pytest.raises(ValueError, match="number"):
        cli._loss_spec(text, ap.parse_args(["train", "--focal-weight", "lots"]))
