"""Dice / BCE-with-logits / Jaccard / Tversky / Focal / CombinedLoss on libuwm's fused HIP loss kernels.

Counterparts of /root/reference/src/utils/losses.py:11-52 and of the smp.losses.DiceLoss /
nn.BCEWithLogitsLoss objects it constructs (SURVEY.md §8 a12,a13, Appendix A.5).  The call protocol
is the reference's: `criterion(outputs (N,1,H,W) float, masks (N,1,H,W) int64|uint8|float) -> 0-d
tensor`, then `.backward()` / `.item()` (/root/reference/src/train.py:94-107).

Dice and BCE (and their CombinedLoss) run on `uwm_loss`; Jaccard, Tversky and Focal, alone or in any weighted mix with the
other two, run on `uwm_loss_ext` (csrc/loss_ext.hip): one spec, one fused call.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from . import model as _model


def _logit_plane(logits: torch.Tensor):
    """(N,1,H,W) or (N,H,W) logits -> (tensor kept alive, data_ptr, element stride ld)."""
    if logits.dim() == 4:
        if logits.shape[1] != 1:
            raise ValueError(f"binary losses take (N,1,H,W) logits, got {tuple(logits.shape)}")
        x = logits[:, 0]
    elif logits.dim() == 3:
        x = logits
    else:
        raise ValueError(f"bad logits shape {tuple(logits.shape)}")
    n, h, w = x.shape
    s = x.stride()
    ld = s[2] if w > 1 else 1
    if not (ld >= 1 and s[1] == w * ld and s[0] == h * w * ld):
        x = x.contiguous()
        ld = 1
    return x, x.data_ptr(), int(ld)


def _target_plane(target: torch.Tensor, n: int, hw: int):
    if target.numel() != n * hw:
        raise ValueError(f"target has {target.numel()} elements, logits have {n * hw}")
    t = target.contiguous()
    return t, t.data_ptr(), L.target_dtype_code(t)


class _DiceBCEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, w_dice, w_bce, smooth, eps):
        if logits.device.type != "cuda":
            raise RuntimeError("uwm losses run only on a HIP device (no CPU fallback)")
        if logits.dtype != torch.float32:
            raise TypeError(f"uwm losses take float32 logits, got {logits.dtype}")
        x, xp, ld = _logit_plane(logits.detach())
        n, h, w = x.shape
        t, tp, tdt = _target_plane(target, n, h * w)
        npix = n * h * w
        scratch = torch.empty(8, dtype=torch.float64, device=x.device)
        out = torch.empty(3, dtype=torch.float32, device=x.device)
        need_grad = logits.requires_grad
        cp = 4
        dl = torch.empty((n, h, w, cp), dtype=torch.float32, device=x.device) if need_grad else None
        with L.on_device(x):
            L.check(L.lib().uwm_loss(C.c_void_p(xp), ld, C.c_void_p(tp), tdt, npix, float(w_dice), float(w_bce),
                                     float(smooth), float(eps), C.c_void_p(scratch.data_ptr()),
                                     C.c_void_p(out.data_ptr()), C.c_void_p(dl.data_ptr() if need_grad else 0), cp, 1.0,
                                     C.c_void_p(L.stream_ptr(x.device))))
        ctx.dl = dl
        ctx.in_shape = tuple(logits.shape)
        return out[0].clone()

    @staticmethod
    def backward(ctx, gout):
        dl = ctx.dl
        if dl is None:
            return (None,) * 6
        n, h, w, cp = dl.shape
        g = dl[..., :1].permute(0, 3, 1, 2)          # (N,1,H,W) view of the padded buffer
        if not (gout.numel() == 1 and float(gout) == 1.0):
            g = g * gout
        else:
            _model._PADDED_PTRS.clear()
            _model._PADDED_PTRS.add(dl.data_ptr())
        if len(ctx.in_shape) == 3:
            g = g[:, 0]
        return g, None, None, None, None, None


def _fused(logits, target, w_dice, w_bce, smooth, eps):
    return _DiceBCEFunction.apply(logits, target, w_dice, w_bce, smooth, eps)


# defaults of uwm_loss_spec (include/uwm.h): every weight 0, smp's constructor defaults for the parameters
SPEC_DEFAULTS = dict(w_dice=0.0, w_bce=0.0, w_jaccard=0.0, w_tversky=0.0, w_focal=0.0, dice_smooth=0.0, dice_eps=1e-7,
                     jaccard_smooth=0.0, jaccard_eps=1e-7, tversky_smooth=0.0, tversky_eps=1e-7, tversky_alpha=0.5, tversky_beta=0.5,
                     tversky_gamma=1.0, focal_alpha=-1.0, focal_gamma=2.0)
NEW_WEIGHTS = ("w_jaccard", "w_tversky", "w_focal")


def make_loss_spec(spec=None, **fields):
    """A `uwm_loss_spec` from a mapping and / or keyword fields over SPEC_DEFAULTS (focal_alpha None or negative: no alpha);
    a `uwm_loss_spec` passes through."""
    if isinstance(spec, L.uwm_loss_spec) and not fields:
        return spec
    vals = dict(SPEC_DEFAULTS)
    if isinstance(spec, L.uwm_loss_spec):
        vals.update({n: getattr(spec, n) for n in SPEC_DEFAULTS})
    elif spec is not None:
        vals.update(spec)
    vals.update(fields)
    unknown = set(vals) - set(SPEC_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown loss spec fields {sorted(unknown)} (known: {sorted(SPEC_DEFAULTS)})")
    if vals["focal_alpha"] is None:
        vals["focal_alpha"] = -1.0
    return L.uwm_loss_spec(**{k: float(v) for k, v in vals.items()})


def spec_needs_ext(spec) -> bool:
    """True when the spec asks for Jaccard, Tversky or Focal, i.e. for uwm_loss_ext instead of uwm_loss"""
    return any(getattr(spec, n) != 0.0 for n in NEW_WEIGHTS)


class _ExtLossFunction(torch.autograd.Function):
    """uwm_loss_ext: returns (total, the eight terms {total, dice, bce, jaccard, tversky, focal, 0, 0})"""

    @staticmethod
    def forward(ctx, logits, target, spec):
        if logits.device.type != "cuda":
            raise RuntimeError("uwm losses run only on a HIP device (no CPU fallback)")
        if logits.dtype != torch.float32:
            raise TypeError(f"uwm losses take float32 logits, got {logits.dtype}")
        x, xp, ld = _logit_plane(logits.detach())
        n, h, w = x.shape
        t, tp, tdt = _target_plane(target, n, h * w)
        scratch = torch.empty(8, dtype=torch.float64, device=x.device)
        out = torch.empty(8, dtype=torch.float32, device=x.device)
        need_grad = logits.requires_grad
        cp = 4
        dl = torch.empty((n, h, w, cp), dtype=torch.float32, device=x.device) if need_grad else None
        with L.on_device(x):
            L.check(L.lib().uwm_loss_ext(C.c_void_p(xp), ld, C.c_void_p(tp), tdt, n * h * w, C.byref(spec),
                                         C.c_void_p(scratch.data_ptr()), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(dl.data_ptr() if need_grad else 0), cp, 1.0, C.c_void_p(L.stream_ptr(x.device))))
        ctx.dl = dl
        ctx.in_shape = tuple(logits.shape)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, gout, _gterms):
        dl = ctx.dl
        if dl is None:
            return None, None, None
        g = dl[..., :1].permute(0, 3, 1, 2)          # (N,1,H,W) view of the padded buffer
        if not (gout.numel() == 1 and float(gout) == 1.0):
            g = g * gout
        else:
            _model._PADDED_PTRS.clear()
            _model._PADDED_PTRS.add(dl.data_ptr())
        if len(ctx.in_shape) == 3:
            g = g[:, 0]
        return g, None, None


def _fused_ext(module, logits, target, spec):
    total, terms = _ExtLossFunction.apply(logits, target, spec)
    module.last_terms = terms                        # device tensor, no host sync
    return total


def _only(name, mode, **unsupported):
    if mode != "binary":
        raise ValueError(f"{name} mode={mode!r} is not supported (binary only)")
    bad = [k for k, (v, ok) in unsupported.items() if v != ok and not (v is None and ok is None)]
    if bad:
        raise ValueError(f"{name}: {', '.join(bad)} not supported (only " + ", ".join(f"{k}={ok!r}" for k, (_, ok) in unsupported.items()) + ")")


class JaccardLoss(nn.Module):
    """smp.losses.JaccardLoss(mode='binary', smooth, from_logits=True, log_loss=False, eps=1e-7)."""

    def __init__(self, mode: str = "binary", classes=None, log_loss: bool = False, from_logits: bool = True, smooth: float = 0.0,
                 eps: float = 1e-7):
        super().__init__()
        _only("JaccardLoss", mode, classes=(classes, None), log_loss=(bool(log_loss), False), from_logits=(bool(from_logits), True))
        self.mode, self.smooth, self.eps = mode, float(smooth), float(eps)

    def spec_fields(self, w):
        return dict(w_jaccard=w, jaccard_smooth=self.smooth, jaccard_eps=self.eps)

    def forward(self, y_pred, y_true):
        return _fused_ext(self, y_pred, y_true, make_loss_spec(self.spec_fields(1.0)))


class TverskyLoss(nn.Module):
    """smp.losses.TverskyLoss(mode='binary', smooth, eps=1e-7, alpha=0.5, beta=0.5, gamma=1.0): alpha weighs the false
    positives, beta the false negatives, the loss is (1 - score) ** gamma."""

    def __init__(self, mode: str = "binary", classes=None, log_loss: bool = False, from_logits: bool = True, smooth: float = 0.0,
                 ignore_index=None, eps: float = 1e-7, alpha: float = 0.5, beta: float = 0.5, gamma: float = 1.0):
        super().__init__()
        _only("TverskyLoss", mode, classes=(classes, None), log_loss=(bool(log_loss), False), from_logits=(bool(from_logits), True),
              ignore_index=(ignore_index, None))
        if not float(gamma) > 0.0:
            raise ValueError(f"TverskyLoss: gamma={gamma!r} must be positive")
        self.mode, self.smooth, self.eps = mode, float(smooth), float(eps)
        self.alpha, self.beta, self.gamma = float(alpha), float(beta), float(gamma)

    def spec_fields(self, w):
        return dict(w_tversky=w, tversky_smooth=self.smooth, tversky_eps=self.eps, tversky_alpha=self.alpha, tversky_beta=self.beta,
                    tversky_gamma=self.gamma)

    def forward(self, y_pred, y_true):
        return _fused_ext(self, y_pred, y_true, make_loss_spec(self.spec_fields(1.0)))


class FocalLoss(nn.Module):
    """smp.losses.FocalLoss(mode='binary', alpha=None, gamma=2.0, reduction='mean')."""

    def __init__(self, mode: str = "binary", alpha=None, gamma: float = 2.0, ignore_index=None, reduction: str = "mean",
                 normalized: bool = False, reduced_threshold=None):
        super().__init__()
        _only("FocalLoss", mode, ignore_index=(ignore_index, None), reduction=(reduction, "mean"), normalized=(bool(normalized), False),
              reduced_threshold=(reduced_threshold, None))
        gamma = 2.0 if gamma is None else gamma
        if not float(gamma) >= 0.0:
            raise ValueError(f"FocalLoss: gamma={gamma!r} must not be negative")
        if alpha is not None and not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"FocalLoss: alpha={alpha!r} must lie in [0, 1] (or None)")
        self.mode, self.alpha, self.gamma = mode, (None if alpha is None else float(alpha)), float(gamma)

    def spec_fields(self, w):
        return dict(w_focal=w, focal_alpha=self.alpha, focal_gamma=self.gamma)

    def forward(self, y_pred, y_true):
        return _fused_ext(self, y_pred, y_true, make_loss_spec(self.spec_fields(1.0)))


class DiceLoss(nn.Module):
    """smp.losses.DiceLoss(mode='binary', smooth, from_logits=True, log_loss=False, eps=1e-7)."""

    def __init__(self, mode: str = "binary", classes=None, log_loss: bool = False, from_logits: bool = True,
                 smooth: float = 0.0, ignore_index=None, eps: float = 1e-7):
        super().__init__()
        if mode != "binary":
            raise ValueError(f"DiceLoss mode={mode!r} is not supported (binary only)")
        if log_loss or not from_logits or ignore_index is not None or classes is not None:
            raise ValueError("DiceLoss: only from_logits=True, log_loss=False, no ignore_index/classes")
        self.mode, self.smooth, self.eps = mode, float(smooth), float(eps)

    def forward(self, y_pred, y_true):
        return _fused(y_pred, y_true, 1.0, 0.0, self.smooth, self.eps)


class BCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss() (mean reduction); integer masks are cast, as SURVEY.md a13 notes."""

    def __init__(self, weight=None, reduction: str = "mean", pos_weight=None):
        super().__init__()
        if weight is not None or pos_weight is not None or reduction != "mean":
            raise ValueError("BCEWithLogitsLoss: only the default (unweighted, mean) form is supported")

    def forward(self, y_pred, y_true):
        return _fused(y_pred, y_true, 0.0, 1.0, 0.0, 1e-7)


class CombinedLoss(nn.Module):
    """/root/reference/src/utils/losses.py:33-52 — sum_i weights[i] * losses[i](pred, target).
    Dice, BCE, Jaccard, Tversky and Focal members are evaluated by ONE fused kernel pass: the first instance of each kind (every
    BCE) folds into one spec; anything else, a second instance of a kind included, is called on its own and added.  A
    combination of Dice and BCE alone stays on `uwm_loss`."""

    def __init__(self, losses, weights=None):
        super().__init__()
        self.losses = list(losses)
        self.weights = list(weights) if weights else [1.0] * len(self.losses)

    def fold(self):
        """(spec fields of the members the fused pass serves, [(member, weight)] left to their own calls)"""
        fields = dict(w_dice=0.0, w_bce=0.0)
        rest, seen = [], set()
        for fn, w in zip(self.losses, self.weights):
            if isinstance(fn, BCEWithLogitsLoss):
                fields["w_bce"] += w
            elif isinstance(fn, DiceLoss) and DiceLoss not in seen:
                fields.update(w_dice=w, dice_smooth=fn.smooth, dice_eps=fn.eps); seen.add(DiceLoss)
            elif isinstance(fn, (JaccardLoss, TverskyLoss, FocalLoss)) and type(fn) not in seen:
                fields.update(fn.spec_fields(w)); seen.add(type(fn))
            else:
                rest.append((fn, w))
        return fields, rest

    def forward(self, pred, target):
        fields, rest = self.fold()
        if any(fields.get(n, 0.0) != 0.0 for n in NEW_WEIGHTS):
            total = _fused_ext(self, pred, target, make_loss_spec(fields))
        elif fields["w_dice"] != 0.0 or fields["w_bce"] != 0.0:
            total = _fused(pred, target, fields["w_dice"], fields["w_bce"], fields.get("dice_smooth", 0.0), fields.get("dice_eps", 1e-7))
        else:
            total = 0
        for fn, w in rest:
            total = total + w * fn(pred, target)
        return total


def criterion_spec(criterion):
    """The `uwm_loss_spec` that evaluates `criterion` (one of this module's losses, or a CombinedLoss of them) in one fused
    call — what Trainer(loss_spec=...) takes, so that the train step and the validation loss are the same function.
    ValueError when a member is not served by the fused pass."""
    if isinstance(criterion, CombinedLoss):
        fields, rest = criterion.fold()
        if rest:
            raise ValueError(f"criterion_spec: {type(rest[0][0]).__name__} is not served by the fused loss pass (or is a second "
                             "instance of its kind)")
        return make_loss_spec(fields)
    if isinstance(criterion, DiceLoss):
        return make_loss_spec(w_dice=1.0, dice_smooth=criterion.smooth, dice_eps=criterion.eps)
    if isinstance(criterion, BCEWithLogitsLoss):
        return make_loss_spec(w_bce=1.0)
    if isinstance(criterion, (JaccardLoss, TverskyLoss, FocalLoss)):
        return make_loss_spec(criterion.spec_fields(1.0))
    raise ValueError(f"criterion_spec: {type(criterion).__name__} is not served by the fused loss pass")


def get_loss_function(cfg):
    """Counterpart of get_loss_function (/root/reference/src/utils/losses.py:11-31).  `CombinedLoss`
    (named by the reference's text-watermark YAML but unhandled there) is wired to
    LOSS.BCE_WEIGHT / LOSS.DICE_WEIGHT (/root/reference/src/configs/config.py:61-62)."""
    name = cfg.LOSS.NAME
    mode = getattr(cfg.LOSS, "MODE", "binary")
    smooth = getattr(cfg.LOSS, "SMOOTH", getattr(cfg.LOSS, "DICE_SMOOTH", 1e-5))
    if name == "DiceLoss":
        return DiceLoss(mode=mode, smooth=smooth)
    if name == "BCEWithLogitsLoss":
        return BCEWithLogitsLoss()
    if name == "CombinedLoss":
        return CombinedLoss([BCEWithLogitsLoss(), DiceLoss(mode=mode, smooth=smooth)],
                            [float(getattr(cfg.LOSS, "BCE_WEIGHT", 0.5)), float(getattr(cfg.LOSS, "DICE_WEIGHT", 0.5))])
    if name == "JaccardLoss":
        return JaccardLoss(mode=mode, smooth=smooth)
    if name == "FocalLoss":                      # (the reference passes neither LOSS.FOCAL_ALPHA nor LOSS.FOCAL_GAMMA: smp's None / 2.0)
        return FocalLoss(mode=mode)
    if name == "TverskyLoss":
        return TverskyLoss(mode=mode, smooth=smooth)
    if name == "LovaszLoss":
        raise ValueError("LOSS.NAME 'LovaszLoss' is not served: it sorts the per-pixel errors of the batch, which this build has no "
                         "device kernel for (DiceLoss | BCEWithLogitsLoss | CombinedLoss | JaccardLoss | TverskyLoss | FocalLoss)")
    raise ValueError(f"不支持的损失函数: {name}")
