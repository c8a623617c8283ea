"""fp64 reference of the losses `uwm_loss_ext` serves, written from the definitions with autograd (no closed-form gradient):
smp's DiceLoss, JaccardLoss, TverskyLoss and FocalLoss in mode='binary' with from_logits=True, log_loss=False, normalized=False,
reduced_threshold=None, reduction='mean', torch's BCEWithLogitsLoss, and their weighted sum (the reference's CombinedLoss).

`spec` everywhere is a plain dict over SPEC_DEFAULTS — the fields of `uwm_loss_spec`, focal_alpha None for "no alpha"."""
import torch

SPEC_DEFAULTS = dict(w_dice=0.0, w_bce=0.0, w_jaccard=0.0, w_tversky=0.0, w_focal=0.0, dice_smooth=0.0, dice_eps=1e-7,
                     jaccard_smooth=0.0, jaccard_eps=1e-7, tversky_smooth=0.0, tversky_eps=1e-7, tversky_alpha=0.5, tversky_beta=0.5,
                     tversky_gamma=1.0, focal_alpha=None, focal_gamma=2.0)
TERMS = ("total", "dice", "bce", "jaccard", "tversky", "focal")


def full_spec(**fields):
    assert set(fields) <= set(SPEC_DEFAULTS), sorted(set(fields) - set(SPEC_DEFAULTS))
    return {**SPEC_DEFAULTS, **fields}


def _sums(x, t):
    p = torch.sigmoid(x)
    return (p * t).sum(), p.sum(), t.sum()


def dice_loss(x, t, smooth=0.0, eps=1e-7):
    i, p, tt = _sums(x, t)
    score = (2.0 * i + smooth) / (p + tt + smooth).clamp_min(eps)
    return (1.0 - score) * (tt > 0).to(x.dtype)


def jaccard_loss(x, t, smooth=0.0, eps=1e-7):
    i, p, tt = _sums(x, t)
    score = (i + smooth) / (p + tt - i + smooth).clamp_min(eps)
    return (1.0 - score) * (tt > 0).to(x.dtype)


def tversky_loss(x, t, smooth=0.0, eps=1e-7, alpha=0.5, beta=0.5, gamma=1.0):
    i, p, tt = _sums(x, t)
    fp, fn = p - i, tt - i                       # sum p (1-t), sum (1-p) t
    score = (i + smooth) / (i + alpha * fp + beta * fn + smooth).clamp_min(eps)
    loss = (1.0 - score) * (tt > 0).to(x.dtype)
    return loss if gamma == 1.0 else loss ** gamma


def bce_terms(x, t):
    """per-pixel BCE with logits as max(x, 0) - x t + softplus(-|x|).  torch's own kernel forms the last term as log(1 + exp(-|x|)),
    which is exactly 0 from |x| = 37 on in fp64; 1 - pt is then 0 and autograd of its gamma < 1 power is 0 * inf.  With log1p the term
    stays positive and the focal gradient finite at every logit the tests use."""
    return torch.clamp(x, min=0.0) - x * t + torch.log1p(torch.exp(-x.abs()))


def focal_loss(x, t, alpha=None, gamma=2.0):
    logpt = bce_terms(x, t)
    one_minus_pt = -torch.expm1(-logpt)          # 1 - exp(-logpt), as the issue states it: no cancellation at confident pixels
    loss = one_minus_pt ** gamma * logpt
    if alpha is not None:
        loss = loss * (alpha * t + (1.0 - alpha) * (1.0 - t))
    return loss.mean()


def terms(x, t, spec):
    """the six loss values as 0-d fp64 tensors (attached to x): total, dice, bce, jaccard, tversky, focal"""
    q = spec
    out = dict(dice=dice_loss(x, t, q["dice_smooth"], q["dice_eps"]), bce=bce_terms(x, t).mean(),
               jaccard=jaccard_loss(x, t, q["jaccard_smooth"], q["jaccard_eps"]),
               tversky=tversky_loss(x, t, q["tversky_smooth"], q["tversky_eps"], q["tversky_alpha"], q["tversky_beta"], q["tversky_gamma"]),
               focal=focal_loss(x, t, q["focal_alpha"], q["focal_gamma"]))
    out["total"] = sum(q["w_" + k] * out[k] for k in ("dice", "bce", "jaccard", "tversky", "focal") if q["w_" + k] != 0.0)
    return out


def loss_and_grad(logits, target, spec):
    """logits, target: any shape / dtype -> ({term: float}, dtotal/dlogits as an fp64 tensor of logits' shape)"""
    x = logits.detach().double().cpu().clone().requires_grad_(True)
    t = target.detach().double().cpu().reshape(x.shape)
    out = terms(x, t, spec)
    total = out["total"]
    if not torch.is_tensor(total) or not total.requires_grad:           # every weight 0, or nothing depends on x
        grad = torch.zeros_like(x)
    else:
        (grad,) = torch.autograd.grad(total, x)
    return {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in out.items()}, grad
