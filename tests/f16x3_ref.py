"""CPU reference of the fp16x3 split arithmetic of conv_f16x3.hip / conv_f16x3v2.hip, and the operands of their op-level tests.

The kernels split every fp32 operand once into two fp16 halves and add up to three fp16 x fp16 products per term in fp32:

    hi(v) = v rounded to fp16 (round to nearest even)          lo(v) = (v - hi(v)) rounded to fp16
    W = a filter element times the power of two of its row     X = an activation (a dgrad's dY times the power of two xs)
    nprod 1: hi(W) hi(X)      nprod 2: + lo(W) hi(X)      nprod 3: + hi(W) lo(X)

`conv_emu` / `dgrad_emu` evaluate exactly these products, accumulated in fp64 and un-scaled at the end; `nprod=0` is the fp64 truth
(the same pipeline, F.conv2d in float64, nothing split).  Around them sits what the kernels fuse: the lazy input transform
x * scale + shift (one fp32 rounding, as the kernels' fused multiply-add; ReLU only where the source asks for it), zero padding AFTER
that transform, nearest x2 up-sampling of source 0, the channel concat with source 1, the bias, and a dgrad's (dx + addend) masked by
(mask * mscale + mshift) > 0.

Row scale: the kernels put a row's largest |element| into [2^13, 2^14) (`top=14`).  tests/test_f16x3_ref.py shows that the result
does not depend on that choice (top=11 gives the same numbers to 1e-3 of the GPU bar), so no test has to copy the rule.  xs puts
max|dY| into [2^13, 2^14) (uwm_launch.inc, "The max|dY| contract").

`wgrad_emu` is the same for wgrad_f16x3.hip's weight gradient (further down: there the two split operands are X, unscaled, and dY
times xs).

Everything is NCHW / OIHW on the CPU; tests/test_f16x3v2_ops_gpu.py and tests/test_wgrad_f16x3_ops_gpu.py pack it for the library.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

BAR = 2e-5            # GPU output bar: BAR * max(1, output range) — _conv_case's fp32-accumulation bar (tests/test_ops_gpu.py)


def hi(v):
    """fp64 tensor of fp32 values -> their fp16 roundings (as fp64)"""
    return v.float().half().double()


def lo(v):
    return (v - hi(v)).float().half().double()


def pow2_scale(mx, top=14):
    """per element of mx (> 0): the power of two s with mx * s in [2^(top-1), 2^top); 1 where mx == 0"""
    _, e = torch.frexp(mx.double())                  # mx = m * 2^e, m in [0.5, 1)
    s = torch.ldexp(torch.ones_like(mx, dtype=torch.float64), top - e)
    return torch.where(mx > 0, s, torch.ones_like(s))


def staged(sources, exact=False):
    """cat over the sources of up(relu?(x * scale + shift)) as fp64 NCHW.  A source = dict(x, scale, shift, relu, up) (scale /
    shift None = plain).  exact: the transform stays in fp64 (the truth); else it is rounded once to fp32 (the kernels' fma)."""
    parts = []
    for s in sources:
        v = s["x"].double()
        if s.get("scale") is not None:
            v = v * s["scale"].double()[None, :, None, None] + s["shift"].double()[None, :, None, None]
            if not exact:
                v = v.float().double()
            if s.get("relu"):
                v = torch.relu(v)
        if s.get("up"):
            v = v.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        parts.append(v)
    return torch.cat(parts, 1)


def _split_conv(X, w, nprod, top, xs):
    """3x3 / pad 1 of fp64 X with fp32 filters w [rows][chans][3][3] on nprod split products (0: plain fp64)"""
    wd = w.double()
    if nprod == 0:
        return F.conv2d(X, wd, None, 1, 1)
    s = pow2_scale(wd.flatten(1).abs().amax(1), top)
    W = wd * s[:, None, None, None]
    Xs = (X * xs).clamp(-65504.0, 65504.0)
    Wh, Xh = hi(W), hi(Xs)
    acc = F.conv2d(Xh, Wh, None, 1, 1)
    if nprod >= 2:
        acc = acc + F.conv2d(Xh, lo(W), None, 1, 1)
    if nprod >= 3:
        acc = acc + F.conv2d(lo(Xs), Wh, None, 1, 1)
    return acc / (s[None, :, None, None] * xs)


def conv_emu(sources, w, nprod, bias=None, top=14):
    """forward conv of the staged sources; nprod 0 = fp64 truth"""
    y = _split_conv(staged(sources, exact=nprod == 0), w, nprod, top, 1.0)
    if bias is not None:
        y = y + bias.double()[None, :, None, None]
    return y


def dgrad_filters(w):
    """forward OIHW weights -> the dgrad's filters [Cin][Cout][3][3], taps mirrored (bank job mode 2)"""
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


def dgrad_emu(dy, w, nprod, addend=None, mask=None, mscale=None, mshift=None, top=14):
    """input gradient of a 3x3 / stride-1 / pad-1 conv with forward weights w, epilogue included; nprod 0 = fp64 truth"""
    mx = dy.abs().max()
    xs = float(pow2_scale(mx.reshape(1), 14)[0])
    v = _split_conv(dy.double(), dgrad_filters(w), nprod, top, xs)
    if addend is not None:
        v = v + addend.double()
    if mask is not None:
        v = torch.where(mask_sign(mask, mscale, mshift) > 0, v, torch.zeros_like(v))
    return v


def mask_sign(mask, mscale, mshift):
    m = mask.double()
    if mscale is not None:
        m = m * mscale.double()[None, :, None, None] + mshift.double()[None, :, None, None]
    return m


# ---------------------------------------------------------------------------------------------------------------- operands
# Forward shapes, each for one branch of conv_f16x3v2.hip's chunk walk / tile walk: name -> (Cin, Cout, N, H, W)
FWD_SHAPES = {
    "32to32": (32, 32, 3, 8, 32),        # two chunks: tail only; 3 workgroups (< 8 XCDs); one tile per image: every halo is padding
    "64to32": (64, 32, 1, 16, 64),       # exactly one four-chunk trip; 2 x 2 tiles: halos from neighbouring tiles
    "96to96": (96, 96, 1, 16, 64),       # trip + tail; 12 workgroups (q8 = 1, r8 = 4); rows % 64 == 32: code 600 takes the second form
    "128to160": (128, 160, 2, 8, 32),    # two trips, five channel tiles; code 600 takes the second form
    "256to256": (256, 256, 1, 8, 32),    # 8 * 256 * 36 * 32 bytes of filters > UWM_V2_COSLOW_BYTES: channel tile slowest
}
FWD_FORMS = ("plain", "lazy")                                  # every shape
FWD_FORMS_96 = ("plain", "lazy", "lazy_norelu", "bias")      # 96 -> 96 only
CAT_CASES = {                                                  # cat(nearest x2 of source 0, source 1) -> 32 channels at 1 x 16 x 64: (C0, C1, source 1 lazy)
    "cat32+32": (32, 32, False),
    "cat16+48": (16, 48, False),         # the concat boundary inside the first chunk pair
    "cat48+16": (48, 16, False),         # ... inside the second
    "cat32+32lazy": (32, 32, True),
}
DGRAD_SHAPES = {                                               # name -> (Cin, Cout, N, H, W): dx [N][Cin][H][W] from dy [N][Cout][H][W]
    "32from64": (32, 64, 1, 16, 64),
    "96from32": (96, 32, 3, 8, 32),
    "160from128": (160, 128, 2, 8, 32),
}
DGRAD_FORMS = ("plain", "addmask", "addmask_affine")
DY_SMALL, DY_LARGE = 1e-6, 1e3


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _lazy(g, c):
    scale = torch.rand(c, generator=g) + 0.5
    scale[::3] *= -1
    return scale, torch.randn(c, generator=g) * 0.3


def _source(g, n, c, h, w, lazy=False, relu=True, up=0):
    s = {"x": torch.randn(n, c, h, w, generator=g), "scale": None, "shift": None, "relu": 0, "up": up}
    if lazy:
        s["scale"], s["shift"] = _lazy(g, c)
        s["relu"] = 1 if relu else 0
    return s


@functools.lru_cache(maxsize=None)
def fwd_case(shape, form):
    """operands of a forward case: dict(sources, w, bias, n, h, w_, cout)"""
    g = _gen(f"fwd/{shape}/{form}")
    if shape in CAT_CASES:
        c0, c1, lazy1 = CAT_CASES[shape]
        cin, cout, n, h, w = c0 + c1, 32, 1, 16, 64
        sources = [_source(g, n, c0, h // 2, w // 2, lazy=True, up=1), _source(g, n, c1, h, w, lazy=lazy1)]
    else:
        cin, cout, n, h, w = FWD_SHAPES[shape]
        sources = [_source(g, n, cin, h, w, lazy=form.startswith("lazy"), relu=form != "lazy_norelu")]
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (cin * 9) ** 0.5)
    bias = torch.randn(cout, generator=g) * 0.25 if form == "bias" else None      # (a unit-variance bias widens the output range until one product sits within 10 bars of the truth: test_f16x3_ref.py, check 2)
    return {"sources": sources, "w": wt, "bias": bias, "n": n, "h": h, "w_": w, "cin": cin, "cout": cout}


def fwd_cases():
    out = [(s, f) for s in FWD_SHAPES for f in (FWD_FORMS_96 if s == "96to96" else FWD_FORMS)]
    return out + [(s, "cat") for s in CAT_CASES]


@functools.lru_cache(maxsize=None)
def fwd_ref(shape, form, nprod, top=14):
    c = fwd_case(shape, form)
    return conv_emu(c["sources"], c["w"], nprod, c["bias"], top)


@functools.lru_cache(maxsize=None)
def dgrad_case(shape, form, mag=DY_SMALL):
    """operands of a dgrad case: dict(dy, w, addend, mask, mscale, mshift, y, mean, rstd, ...); addend / mask in units of mag.
    The mask is kept 1e-3 away from its threshold, so that fp32 and fp64 agree on every sign."""
    g = _gen(f"dgrad/{shape}")                      # dy and w are the layer's: every form of a layer multiplies the same operands
    cin, cout, n, h, w = DGRAD_SHAPES[shape]
    c = {"n": n, "h": h, "w_": w, "cin": cin, "cout": cout, "mag": mag, "addend": None, "mask": None, "mscale": None, "mshift": None}
    c["dy"] = torch.randn(n, cout, h, w, generator=g) * mag
    c["w"] = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (cout * 9) ** 0.5)      # (dx of unit variance, in units of mag)
    g = _gen(f"dgrad/{shape}/{form}")
    if form != "plain":
        c["addend"] = torch.randn(n, cin, h, w, generator=g) * (0.25 * mag)      # (a larger addend widens the range until one product sits within 10 bars of the truth: test_f16x3_ref.py, check 2)
        mask = torch.randn(n, cin, h, w, generator=g)
        if form == "addmask_affine":
            c["mscale"], c["mshift"] = _lazy(g, cin)
            near = mask_sign(mask, c["mscale"], c["mshift"]).abs() < 1e-3
            mask = torch.where(near, mask + 0.01 / c["mscale"][None, :, None, None], mask)
        else:
            mask = torch.where(mask.abs() < 1e-3, torch.full_like(mask, 0.01), mask)
        c["mask"] = mask
    # a BatchNorm's raw input other than the mask tensor (bnb_y), and the statistics the fused sums normalise with
    c["y"] = torch.randn(n, cin, h, w, generator=g)
    c["mean"] = torch.randn(cin, generator=g) * 0.2
    c["rstd"] = torch.rand(cin, generator=g) + 0.5
    return c


@functools.lru_cache(maxsize=None)
def dgrad_ref(shape, form, nprod, mag=DY_SMALL, top=14):
    c = dgrad_case(shape, form, mag)
    return dgrad_emu(c["dy"], c["w"], nprod, c["addend"], c["mask"], c["mscale"], c["mshift"], top)


def out_range(ref):
    return float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- weight gradient
# wgrad_f16x3.hip: dW[co][ci][tap] = sum over pixels of dY[p][co] * X[p + tap][ci].  X = the staged sources, clamped to +-65504 and
# NOT scaled; D = dY times the power of two xs that puts max|dY| into [2^13, 2^14) (1 when dY is all zero).  dW is bilinear in
# (X, D), so with G(X, D) = the fp64 weight gradient of F.conv2d(X, w, None, 1, 1):
#     nprod 1: G(hi X, hi D)      nprod 2: + G(lo X, hi D)      nprod 3: + G(hi X, lo D)           all divided by xs
WGRAD_BAR = 3e-5      # GPU bar: WGRAD_BAR * range of the true gradient — test_wgrad_f16x3_direct's (tests/test_ops_gpu.py)


def wgrad64(X, D):
    """fp64 autograd weight gradient [Cout][Cin][3][3] of the 3x3 / stride-1 / pad-1 conv of X [N][Cin][H][W] with output gradient D"""
    w = torch.zeros(D.shape[1], X.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.conv2d(X, w, None, 1, 1), w, D)[0]


def wgrad_emu(sources, dy, nprod, top=14):
    """weight gradient of the staged sources on nprod split products; nprod 0 = fp64 truth (nothing rounded, clamped or split)"""
    X, D = staged(sources, exact=nprod == 0), dy.double()
    if nprod == 0:
        return wgrad64(X, D)
    X = X.clamp(-65504.0, 65504.0)
    xs = float(pow2_scale(D.abs().max().reshape(1), top)[0])
    D = D * xs
    Xh, Dh = hi(X), hi(D)
    acc = wgrad64(Xh, Dh)
    if nprod >= 2:
        acc = acc + wgrad64(lo(X), Dh)
    if nprod >= 3:
        acc = acc + wgrad64(Xh, lo(D))
    return acc / xs


def wgrad_splits(pairs, nstages, cus):
    """the launcher's pixel split (launch_wgrad_f16x3; cu_share 0, scratch not binding) -> (nsplit, stages per split)"""
    nsplit = max(1, min(-(-cus // pairs), nstages // 4))
    sps = -(-nstages // nsplit)
    return -(-nstages // sps), sps


def wgrad_geometry(cin, wrows, h, w, n):
    """(stage width, (64-row, 32-channel) tile pairs, stages of 128 pixels) of a layer; None where the kernel does not take the image"""
    wx = 32 if w % 32 == 0 and h % 4 == 0 else 16 if w % 16 == 0 and h % 8 == 0 else 0
    if not wx:
        return None
    return wx, -(-wrows // 64) * (cin // 32), n * (h // (128 // wx)) * (w // wx)


# One shape per branch of the kernel's stage walk, tile walk and grid: name -> (Cin, wrows, dY channels, N, H, W), the smallest that
# reaches it.  WGRAD_CLAIMS: (stage width, workgroups, splits, stages per split) of each, on any card of 64 CUs or more
# (tests/test_f16x3_ref.py::test_wgrad_case_table).
WGRAD_SHAPES = {
    "one_stage": (32, 32, 32, 1, 4, 32),      # 1 stage, no split: += straight into dW; a half-empty 64-row tile; 1 workgroup
    "two_stage": (32, 64, 64, 2, 4, 32),      # 2 stages: the even tail of the two-buffer walk
    "three_stage": (64, 64, 64, 3, 4, 32),    # 3 stages: the odd tail; two input-channel tiles share dY
    "seven": (32, 32, 32, 1, 28, 32),         # 7 stages in one workgroup: steady state, prefetch index clamped at the end
    "uneven": (32, 96, 96, 1, 36, 32),        # 9 stages -> splits of 5 + 4 (the shorter last split); rows 64..95 in a second, half-empty tile; partial images + reduce
    "halo": (96, 40, 40, 1, 8, 64),           # 2 x 2 stage tiles: halo rows and columns from neighbours; 40 rows overhang; 3 workgroups
    "xcd12": (96, 40, 40, 4, 8, 64),          # 16 stages -> 4 splits; 12 workgroups (q8 = 1, r8 = 4)
    "xcd8": (128, 64, 64, 2, 16, 32),         # 8 stages -> 2 splits; 8 workgroups (q8 = 1, r8 = 0)
    "padrows": (32, 38, 40, 2, 4, 32),        # wrows < Cout: dY padded to whole channel quads, dW with fewer rows
    "wx16_one": (64, 32, 32, 1, 8, 16),       # 8 x 16-pixel stages: 1 stage
    "wx16_split": (32, 64, 64, 5, 16, 16),    # ... 10 stages -> 2 x 5, two tile rows per image
    "wx16_w48": (32, 32, 32, 1, 8, 48),       # ... on a width that is no multiple of 32: 3 stages
}
WGRAD_CLAIMS = {
    "one_stage": (32, 1, 1, 1), "two_stage": (32, 1, 1, 2), "three_stage": (32, 2, 1, 3), "seven": (32, 1, 1, 7), "uneven": (32, 4, 2, 5),
    "halo": (32, 3, 1, 4), "xcd12": (32, 12, 4, 4), "xcd8": (32, 8, 2, 4), "padrows": (32, 1, 1, 2), "wx16_one": (16, 2, 1, 1),
    "wx16_split": (16, 2, 2, 5), "wx16_w48": (16, 1, 1, 3),
    "cat1x8x32/upcat": (32, 2, 1, 2), "cat1x8x32/upcat_plain_skip": (32, 3, 1, 2),
    "cat2x8x64/upcat": (32, 4, 2, 4), "cat2x8x64/upcat_plain_skip": (32, 6, 2, 4),
}
WGRAD_FORMS = ("plain", "lazy")                                # every shape
WGRAD_FORMS_MORE = {"three_stage": ("lazy_norelu",), "wx16_w48": ("lazy_norelu",)}
WGRAD_CAT_SHAPES = {"cat1x8x32": (1, 8, 32), "cat2x8x64": (2, 8, 64)}      # cat(nearest x2 of source 0, source 1) -> 64 rows at N, H, W
WGRAD_CAT_FORMS = {                                            # (C0, C1, source 1 lazy): source 0 always lazy + ReLU at half resolution
    "upcat": (32, 32, True),                  # the concat boundary on the first 32-channel tile; source 1 with its own scale, shift and ReLU
    "upcat_plain_skip": (64, 32, False),
}
WGRAD_RANGES = (                                               # (shape, form, dY magnitude, X magnitude) of test_wgrad_ranges
    ("halo", "lazy", DY_LARGE, 1.0),
    ("halo", "lazy", DY_SMALL, 300.0),
    ("halo", "lazy", DY_SMALL, 1e-3),
)


def wgrad_cases():
    out = [(s, f) for s in WGRAD_SHAPES for f in WGRAD_FORMS + WGRAD_FORMS_MORE.get(s, ())]
    return out + [(s, f) for s in WGRAD_CAT_SHAPES for f in WGRAD_CAT_FORMS]


def wgrad_dims(shape, form):
    """(Cin in total, wrows, dY channels, N, H, W)"""
    if shape in WGRAD_CAT_SHAPES:
        c0, c1, _ = WGRAD_CAT_FORMS[form]
        return (c0 + c1, 64, 64) + WGRAD_CAT_SHAPES[shape]
    return WGRAD_SHAPES[shape]


@functools.lru_cache(maxsize=None)
def wgrad_case(shape, form, mag=DY_SMALL, xmag=1.0):
    """operands of a weight-gradient case: dict(sources, dy [N][wrows][H][W], cin, wrows, coutp, n, h, w_).  dY ~ mag with the left
    half of the image a further 1e-3 smaller (mag 0: all zero); X ~ xmag (a lazy shift scaled along).  The unit operands of a
    (shape, form) are the same at every magnitude."""
    g = _gen(f"wgrad/{shape}/{form}")
    cin, wrows, coutp, n, h, w = wgrad_dims(shape, form)
    if shape in WGRAD_CAT_SHAPES:
        c0, c1, lazy1 = WGRAD_CAT_FORMS[form]
        sources = [_source(g, n, c0, h // 2, w // 2, lazy=True, up=1), _source(g, n, c1, h, w, lazy=lazy1)]
    else:
        sources = [_source(g, n, cin, h, w, lazy=form.startswith("lazy"), relu=form != "lazy_norelu")]
    for s in sources:
        s["x"] = s["x"] * xmag
        if s["shift"] is not None:
            s["shift"] = s["shift"] * xmag
    dy = torch.randn(n, wrows, h, w, generator=g) * mag
    dy[:, :, :, : w // 2] *= 1e-3
    return {"sources": sources, "dy": dy, "cin": cin, "wrows": wrows, "coutp": coutp, "n": n, "h": h, "w_": w}


@functools.lru_cache(maxsize=None)
def wgrad_ref(shape, form, nprod, mag=DY_SMALL, xmag=1.0, top=14):
    c = wgrad_case(shape, form, mag, xmag)
    return wgrad_emu(c["sources"], c["dy"], nprod, top)
