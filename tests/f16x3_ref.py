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

Everything is NCHW / OIHW on the CPU; tests/test_f16x3v2_ops_gpu.py packs it for the library.
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
