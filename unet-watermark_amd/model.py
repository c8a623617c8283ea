"""`Unet` — drop-in for `smp.Unet(...)` as the reference constructs it
(/root/reference/src/models/unet_model.py:64-71,93-120), executing on libuwm's HIP kernels.

* same constructor keywords as smp.Unet; unsupported values raise ValueError
  (mirroring unet_model.py:55-59's explicit rejection).
* parameters / BatchNorm buffers are real torch tensors that alias ONE flat device arena whose
  layout libuwm defines; `state_dict()` keys and logical OIHW shapes are smp-compatible
  (SURVEY.md Appendix A.2), so checkpoints interchange with the reference.
* forward/backward run only on a HIP device; there is no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from ._device import norm_arrays, ptr


class _Node(nn.Module):
    """Plain container used to reproduce smp's module tree (names only)."""


def _get_node(root: nn.Module, path: Sequence[str]) -> nn.Module:
    cur = root
    for name in path:
        nxt = cur._modules.get(name)
        if nxt is None:
            nxt = _Node()
            cur.add_module(name, nxt)
        cur = nxt
    return cur


class SegmentationModelError(RuntimeError):
    pass


class _UnetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, *params):
        logits = module._forward_raw(x, training=True)
        ctx.module = module
        ctx.gen = module._fwd_gen
        return module._logits_view(logits)

    @staticmethod
    def backward(ctx, grad_out):
        m = ctx.module
        if ctx.gen != m._fwd_gen:
            raise RuntimeError("uwm: backward called after another forward overwrote the workspace "
                               "(one forward/backward pair at a time per model)")
        dl = m._as_padded_dlogits(grad_out)
        m._backward_raw(dl)
        if m._arena_grads_only:         # a fused flat optimizer consumes the arena itself (train.py): no per-parameter copies
            return (None, None) + (None,) * len(m._plist)
        grads = tuple(m._grad_views[i] if p.requires_grad else None for i, p in enumerate(m._plist))
        return (None, None) + grads


class Unet(nn.Module):
    """MI355X-native U-Net (ResNet-18/34/50 or EfficientNet-b4 encoder, smp UnetDecoder, 3x3 segmentation head)."""

    SUPPORTED_ENCODERS = tuple(L.ENC)
    _ARCH = "Unet"

    def __init__(self, encoder_name: str = "resnet34", encoder_depth: int = 5,
                 encoder_weights: Optional[str] = None, decoder_use_batchnorm: bool = True,
                 decoder_channels: Sequence[int] = (256, 128, 64, 32, 16),
                 decoder_attention_type: Optional[str] = None, in_channels: int = 3, classes: int = 1,
                 activation=None, aux_params: Optional[dict] = None):
        super().__init__()
        if encoder_name not in L.ENC:
            raise ValueError(f"Unsupported encoder: {encoder_name}. Supported encoders: {list(L.ENC)}")
        if encoder_depth != 5:
            raise ValueError(f"encoder_depth={encoder_depth} is not supported (only 5)")
        decoder_channels = tuple(int(c) for c in decoder_channels)
        if len(decoder_channels) != encoder_depth:
            raise ValueError(
                f"Model depth is {encoder_depth}, but you provide `decoder_channels` for {len(decoder_channels)} blocks.")
        if encoder_weights is not None:
            raise ValueError(
                f"encoder_weights={encoder_weights!r} needs a network download, which this build cannot do; "
                f"pass encoder_weights=None and load a local state_dict instead")
        if decoder_use_batchnorm is not True:
            raise ValueError("decoder_use_batchnorm must be True")
        if decoder_attention_type is not None:
            raise ValueError(f"decoder_attention_type={decoder_attention_type!r} is not supported")
        if activation is not None:
            raise ValueError(f"activation={activation!r} is not supported (the reference passes None)")
        if aux_params is not None:
            raise ValueError("aux_params (classification head) is not supported")

        self.encoder_name, self.in_channels, self.classes = encoder_name, int(in_channels), int(classes)
        self.decoder_channels = decoder_channels
        lib = L.lib()
        desc = L.uwm_unet_desc(L.ENC[encoder_name], self.in_channels, self.classes,
                               (C.c_int * 5)(*decoder_channels), 1e-5, 0.1, L.ARCH[self._ARCH])
        h = C.c_void_p()
        L.check(lib.uwm_create(C.byref(desc), C.byref(h)), ValueError)
        self._h = h
        self._cp = lib.uwm_logits_channels(h)
        self._n_param = lib.uwm_param_arena_floats(h)
        self._n_buf = lib.uwm_buffer_arena_floats(h)
        self._infos = []
        for i in range(lib.uwm_num_tensors(h)):
            ti = L.uwm_tensor_info()
            L.check(lib.uwm_tensor_info_get(h, i, C.byref(ti)))
            self._infos.append((ti.name.decode(), ti.kind, ti.arena, int(ti.offset),
                                tuple(ti.shape[: ti.ndim]), tuple(ti.stride[: ti.ndim])))
        self.stages = []
        for s in range(lib.uwm_num_stages(h)):
            b, e = C.c_longlong(), C.c_longlong()
            L.check(lib.uwm_stage_range(h, s, C.byref(b), C.byref(e)))
            self.stages.append((int(b.value), int(e.value)))

        self._param_arena = torch.zeros(self._n_param, dtype=torch.float32)
        self._buffer_arena = torch.zeros(self._n_buf, dtype=torch.float32)
        self._grad_arena = None
        self._plist, self._pinfo, self._binfo = [], [], []
        for name, kind, arena, off, shape, stride in self._infos:
            *path, leaf = name.split(".")
            node = _get_node(self, path)
            if arena == L.ARENA_PARAM:
                p = nn.Parameter(self._param_arena.as_strided(shape, stride, off))
                node.register_parameter(leaf, p)
                self._plist.append(p)
                self._pinfo.append((off, shape, stride))
            else:
                node.register_buffer(leaf, self._buffer_arena.as_strided(shape, stride, off))
                self._binfo.append((node, leaf, off, shape, stride))
                if kind == L.KIND_BN_VAR:
                    self._nbt = getattr(self, "_nbt", [])
                    self._nbt.append(node)
        # all num_batches_tracked counters alias one int64 arena: ONE increment kernel per training forward
        self._nbt_arena = torch.zeros(len(self._nbt), dtype=torch.long)
        for i, node in enumerate(self._nbt):
            node.register_buffer("num_batches_tracked", self._nbt_arena[i])
        self._grad_views = []
        self._ws = None
        self._ws_key = None
        self._fwd_gen = 0
        self._bound = None
        # EfficientNet encoders: stochastic depth of the MBConv blocks (efficientnet_pytorch drop_connect_rate 0.2)
        self._n_mb = lib.uwm_num_mbconv_blocks(h)
        self._mb_drop = [float(lib.uwm_mbconv_drop_rate(h, i)) for i in range(self._n_mb)]
        self.drop_connect = self._n_mb > 0
        self.precision = {v: k for k, v in L.PREC.items()}[lib.uwm_get_precision(h)]       # the process default (UWM_PRECISION) or "f32"
        self._fused_opt_ref = None        # weakref to the fused flat optimizer that consumes the gradient arena itself (train.py)
        self._keep_override = None        # tests: {0,1} keep masks [n_blocks, N] instead of a random draw
        self._rowscale = None
        self._frozen = False              # freeze(): eval forwards read the frozen arena
        self._fz_arena = None             # the arena tensor (uint8), owned here
        self.reset_parameters()

    # ------------------------------------------------------------------ init
    @torch.no_grad()
    def reset_parameters(self):
        pi = 0
        for name, kind, arena, off, shape, stride in self._infos:
            if arena == L.ARENA_PARAM:
                p = self._plist[pi]; pi += 1
                if kind == L.KIND_CONV_W:
                    w = torch.empty(shape, dtype=torch.float32)
                    fan_in = shape[1] * shape[2] * shape[3]
                    if name.startswith("encoder._"):        # efficientnet_pytorch keeps torch's default Conv2d init
                        nn.init.kaiming_uniform_(w, a=5 ** 0.5)
                    elif name.startswith("encoder."):
                        nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
                    elif name.startswith("decoder."):
                        nn.init.kaiming_uniform_(w, mode="fan_in", nonlinearity="relu")
                    else:
                        nn.init.xavier_uniform_(w)
                    p.copy_(w.to(p.device))
                elif kind == L.KIND_BN_GAMMA:
                    p.fill_(1.0)
                elif kind == L.KIND_BIAS and name.startswith("encoder._"):   # default Conv2d bias init (SE layers)
                    bound = 1.0 / fan_in ** 0.5
                    p.copy_(torch.empty(shape, dtype=torch.float32).uniform_(-bound, bound).to(p.device))
                else:
                    p.zero_()
        for node, leaf, off, shape, stride in self._binfo:
            getattr(node, leaf).fill_(1.0 if leaf == "running_var" else 0.0)
        self._nbt_arena.zero_()

    # ------------------------------------------------------------------ device movement keeps the arena aliasing
    def _apply(self, fn, recurse=True):
        self.unfreeze()
        new_p = fn(self._param_arena)
        new_b = fn(self._buffer_arena)
        if new_p.dtype != torch.float32 or new_b.dtype != torch.float32:
            raise TypeError("uwm.Unet parameters are fp32 only (half()/bfloat16() are not supported)")
        self._param_arena, self._buffer_arena = new_p.contiguous(), new_b.contiguous()
        self._grad_arena = None
        self._grad_views = []
        for p, (off, shape, stride) in zip(self._plist, self._pinfo):
            p.data = self._param_arena.as_strided(shape, stride, off)
            p.grad = None
        for node, leaf, off, shape, stride in self._binfo:
            node._buffers[leaf] = self._buffer_arena.as_strided(shape, stride, off)
        self._nbt_arena = fn(self._nbt_arena)
        for i, node in enumerate(self._nbt):
            node._buffers["num_batches_tracked"] = self._nbt_arena[i]
        self._ws = None
        self._ws_key = None
        self._bound = None
        return self

    @property
    def device(self):
        return self._param_arena.device

    @property
    def _arena_grads_only(self) -> bool:
        """True while a LIVE fused flat optimizer (train.py) owns the gradient arena: backward() then leaves `p.grad` unset.
        The flag dies with that optimizer (or its close()), so a torch.optim optimizer, clip_grad_norm_ or a gradient
        check used on the same model afterwards sees populated `p.grad` again."""
        ref = self._fused_opt_ref
        return ref is not None and ref() is not None

    def flat_parameters(self) -> torch.Tensor:
        """The flat fp32 parameter arena (padding included; padding is always zero)."""
        return self._param_arena

    def flat_grads(self) -> torch.Tensor:
        self._ensure_bound()
        return self._grad_arena

    def num_parameters(self) -> int:
        return int(L.lib().uwm_param_count(self._h))

    def set_precision(self, mode: str = "f32", min_workgroups: Optional[int] = None, routing_batch: Optional[int] = None):
        """Arithmetic of the convolution products, per model (uwm_set_precision): "f32" (default: exact fp32 matrix
        instructions); "bf16x3" (opt-in: the backward data-gradient convolutions take each product as a_hi*b_hi + a_hi*b_lo +
        a_lo*b_hi over bf16 halves of the fp32 operands, fp32 accumulation — the forward, hence every logit, is unchanged);
        "bf16x3_all" (forward products too: 1.6e-3 logit error on resnet34, outside the 1e-3 bar on deep encoders);
        "f16x3" / "f16x3_all" (3x3 stride-1 convolutions — forward / forward, data and weight gradients — in direct form on
        gfx950's v_mfma_f32_16x16x32_f16 with every fp32 operand split into two fp16 halves: 22-bit operands, fp32 accumulation,
        power-of-two range scaling; fp32-class accuracy: the fp32 mode's parity bars hold, logit error 1.0e-4 either way).
        Parameters, activations, gradients and optimizer state stay fp32.  The reference's GPU path is reduced precision
        as well (fp16 autocast + GradScaler, /root/reference/src/train.py:75,89-98)."""
        if mode not in L.PREC:
            raise ValueError(f"unsupported precision {mode!r} (supported: {list(L.PREC)})")
        self.unfreeze()                      # the bank forms follow the precision mode and the routing: freeze again afterwards
        L.check(L.lib().uwm_set_precision(self._h, L.PREC[mode]), ValueError)
        if min_workgroups is not None:       # fp16x3 modes: smallest launch the fp16x3 kernels take (default: one workgroup per two CUs)
            L.check(L.lib().uwm_set_precision_fill(self._h, int(min_workgroups)), ValueError)
        if routing_batch is not None:        # choose kernels as if the batch were this many images (0: the real batch) — uwm_set_routing_batch
            L.check(L.lib().uwm_set_routing_batch(self._h, int(routing_batch)), ValueError)
        self.precision = mode
        return self

    # ------------------------------------------------------------------ frozen-weight inference
    @property
    def frozen(self) -> bool:
        return bool(getattr(self, "_frozen", False))

    def freeze(self, batch_shape: Optional[Sequence[int]] = None):
        """Freeze the weights for inference (uwm_freeze): everything the eval forward derives from parameters and buffers alone —
        every BatchNorm's scale / shift, every forward filter bank, the stem bank — is computed ONCE into an arena this model owns,
        and eval forwards then launch no weight-preparation kernel.  Logits stay bit-identical to the unfrozen eval forward.

        Needs eval mode and a HIP device.  `batch_shape` = (N, H, W) fixes the bank forms now; with None the first eval forward
        after freeze() fixes them for its own shape.  A later forward whose shape selects other forms still gives the same
        logits, through the unfrozen path, without touching the arena (call freeze(batch_shape=...) again to serve it from the
        arena; `frozen_serves` tells).  With the routing pinned (set_precision(..., min_workgroups=1) or a routing batch)
        the forms do not depend on the batch size.

        train(True), load_state_dict, .to() / .float() (`_apply`) and set_precision (precision, min_workgroups, routing_batch)
        unfreeze: call freeze() again afterwards.  Parameters or buffers changed in any OTHER way (an optimizer step on a
        model left in eval mode, in-place writes) are not seen: unfreeze() / freeze() by hand then.  unfreeze() releases the
        arena, so a hipGraph captured from a frozen forward must not be replayed after it."""
        if self.training:
            raise RuntimeError("freeze() needs eval mode (call .eval() first): a training forward moves the running statistics")
        self._require_gpu()
        L.check(L.lib().uwm_unfreeze(self._h))
        self._frozen = True
        if batch_shape is not None:
            n, h, w = (int(v) for v in batch_shape)
            self._ensure_bound()
            self._freeze_now(n, h, w)
        return self

    def unfreeze(self):
        if getattr(self, "_h", None) is not None and getattr(self, "_frozen", False):
            L.check(L.lib().uwm_unfreeze(self._h))
        self._frozen = False
        self._fz_arena = None
        return self

    def _freeze_now(self, n: int, h: int, w: int):
        need = int(L.lib().uwm_frozen_bytes(self._h))
        if self._fz_arena is None or self._fz_arena.numel() < need or self._fz_arena.device != self.device:
            self._fz_arena = torch.empty(need, dtype=torch.uint8, device=self.device)
        with L.on_device(self._fz_arena):
            L.check(L.lib().uwm_freeze(self._h, C.c_void_p(self._fz_arena.data_ptr()), self._fz_arena.numel(), n, h, w,
                                       C.c_void_p(L.stream_ptr(self.device))), SegmentationModelError)

    def frozen_serves(self, n: int, h: int, w: int) -> bool:
        """True when an eval forward of (n, h, w) would read the frozen arena right now (uwm_frozen_serves)."""
        return bool(self.frozen and L.lib().uwm_frozen_serves(self._h, int(n), int(h), int(w)))

    def prep_launches(self) -> int:
        """Weight-preparation launches enqueued by this model so far (uwm_prep_launches): stands still across frozen forwards."""
        return int(L.lib().uwm_prep_launches(self._h))

    def train(self, mode: bool = True):
        if mode:
            self.unfreeze()
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self.unfreeze()
        return super().load_state_dict(*args, **kwargs)

    def routing(self, enable: Optional[bool] = None, clear: bool = True):
        """Routing record of the library (uwm_routing_enable / uwm_routing_dump): with `enable` switch the record on / off; otherwise
        return the list of (pass, layer, kernel) of every convolution-class launch since the last call — which HIP kernel each
        layer's forward / dgrad / wgrad ran on (tests and bench.py assert it for the benched precision mode)."""
        if enable is not None:
            L.check(L.lib().uwm_routing_enable(self._h, int(bool(enable))))
            return self
        need = int(L.lib().uwm_routing_dump(self._h, None, 0, 0))
        buf = C.create_string_buffer(max(1, need))
        L.lib().uwm_routing_dump(self._h, buf, need, int(clear))
        out = []
        for line in buf.value.decode().splitlines():
            if line:
                pas, layer, kern = line.split(" ", 2)
                out.append((pas, layer, kern.strip("()")))       # (a templated kernel is written "(name<args>)" at its launch site)
        return out

    def conv_flops(self, h: int, w: int):
        """Algorithmic conv FLOPs per image at h x w: (forward, forward+backward) — SURVEY.md 8(d)."""
        f, fb = C.c_double(), C.c_double()
        L.check(L.lib().uwm_conv_flops(self._h, int(h), int(w), C.byref(f), C.byref(fb)))
        return f.value, fb.value

    # ------------------------------------------------------------------ raw entry points
    def _require_gpu(self, x: Optional[torch.Tensor] = None):
        if self._param_arena.device.type != "cuda":
            raise RuntimeError("uwm.Unet runs only on a HIP device (no CPU fallback): call .to('cuda') first")
        if x is not None and x.device != self._param_arena.device:
            raise RuntimeError(f"input is on {x.device} but the model is on {self._param_arena.device}")

    def _ensure_bound(self):
        self._require_gpu()
        if self._grad_arena is None:
            self._grad_arena = torch.zeros_like(self._param_arena)
            self._grad_views = [self._grad_arena.as_strided(shape, stride, off) for off, shape, stride in self._pinfo]
            self._bound = None
        key = (self._param_arena.data_ptr(), self._grad_arena.data_ptr(), self._buffer_arena.data_ptr())
        if self._bound != key:
            L.check(L.lib().uwm_bind(self._h, C.c_void_p(key[0]), C.c_void_p(key[1]), C.c_void_p(key[2])))
            self._bound = key

    def _workspace(self, need, key):
        """the model's one workspace with at least `need` bytes, what a uwm_*_workspace_bytes query of this handle answered (0: its
        refusal), for the plan `key` = (forward batch, h, w, training); grown when it is too small.  A captured graph's owner keeps
        its own reference."""
        if need == 0:
            raise SegmentationModelError(L.lib().uwm_last_error().decode())
        if self._ws is None or self._ws.numel() < need or self._ws.device != self.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._ws_key = key
        return self._ws

    def _eval_call_setup(self, name: str, flat, n: int, batch: int, size, query, mean, std):
        """what the eval entry points share: eval mode, the checks of their flat tensors (packed bytes, descriptors in and out first: n
        images need 16 n bytes of each), the input size, the bound / frozen state for the forward batch, the workspace of `query`(h, w)
        bytes, the forward generation and drop-connect -> (h, w, workspace, bytes, mean array, std array)"""
        if self.training:
            raise RuntimeError(f"{name} is an eval-mode path: call .eval() first")
        for t in flat:
            self._require_gpu(t)
            if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
                raise RuntimeError(f"{name} takes flat contiguous uint8 tensors (data.pack_images / data.descs_tensor / tiling.table_tensor)")
        if flat and (n < 1 or flat[1].numel() < 16 * n or flat[2].numel() < 16 * n):
            raise RuntimeError(f"{name}: {n} images need {16 * n} descriptor bytes each way")
        if batch < 1:
            raise RuntimeError(f"{name}: the forward batch must be >= 1 (got {batch})")
        h, w = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        self.check_input_shape(torch.empty((0, self.in_channels, h, w)))
        self._ensure_bound()
        if self._frozen and not L.lib().uwm_is_frozen(self._h):
            self._freeze_now(batch, h, w)
        need = query(h, w)
        ws = self._workspace(need, (batch, h, w, False))
        self._fwd_gen += 1
        if self._n_mb:
            self._set_drop_connect(batch, False, self.device)
        return (h, w, ws, need) + norm_arrays(mean, std, self.in_channels)

    def _predict_bytes(self, n, return_logits):
        """the workspace query of the calls around ONE eval forward of n images: the eval plan [+ the logits behind it]"""
        return lambda h, w: L.lib().uwm_predict_workspace_bytes(self._h, n, h, w, int(not return_logits))

    def check_input_shape(self, x):
        h, w = x.shape[-2:]
        if h % 32 != 0 or w % 32 != 0:
            nh = (h // 32 + 1) * 32 if h % 32 else h
            nw = (w // 32 + 1) * 32 if w % 32 else w
            raise RuntimeError(
                f"Wrong input shape height={h}, width={w}. Expected image height and width divisible by 32. "
                f"Consider pad your images to shape ({nh}, {nw}).")

    def _forward_raw(self, x: torch.Tensor, training: bool) -> torch.Tensor:
        """x [N,Cin,H,W] fp32 on the HIP device -> padded logits [N,H,W,CP]."""
        self._require_gpu(x)
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"expected input of shape (N,{self.in_channels},H,W), got {tuple(x.shape)}")
        self.check_input_shape(x)
        if x.dtype != torch.float32:
            raise TypeError(f"uwm.Unet takes float32 images, got {x.dtype}")
        x = x.contiguous()
        n, _, h, w = x.shape
        self._ensure_bound()
        if self._frozen and not training and not L.lib().uwm_is_frozen(self._h):
            self._freeze_now(n, h, w)        # freeze(batch_shape=None): this forward fixes the forms (also after a re-bind)
        ws = self._workspace(L.lib().uwm_workspace_bytes(self._h, n, h, w, int(training)), (n, h, w, bool(training)))
        logits = torch.empty((n, h, w, self._cp), dtype=torch.float32, device=x.device)
        self._fwd_gen += 1
        if self._n_mb:
            self._set_drop_connect(n, training, x.device)
        L.check(L.lib().uwm_forward(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(logits.data_ptr()),
                                    C.c_void_p(ws.data_ptr()), ws.numel(), n, h, w, int(training),
                                    C.c_void_p(L.stream_ptr(x.device))), SegmentationModelError)
        if training:
            self._nbt_arena += 1
        return logits

    @torch.no_grad()
    def predict_u8(self, images_u8: torch.Tensor, mean, std, threshold: float = 0.5, apply_sigmoid: bool = False,
                   out_size=None, return_logits: bool = False):
        """uint8 (N,H,W,C) images on the HIP device -> uint8 {0,255} masks (N,out_h,out_w) in ONE library call (uwm_predict_u8):
        Normalize(mean, std) of x/255 written straight into the forward's input layout, eval forward (frozen or not), bilinear
        resize to `out_size` (default: the input size) + threshold.  Bit-identical to device_preprocess -> forward ->
        resize_threshold.  return_logits: also the logits (N,classes,H,W)."""
        self._require_gpu(images_u8)
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != self.in_channels:
            raise RuntimeError(f"expected uint8 images of shape (N,H,W,{self.in_channels}), got {images_u8.dtype} {tuple(images_u8.shape)}")
        x = images_u8.contiguous()
        n = x.shape[0]
        h, w, ws, _, mean_c, std_c = self._eval_call_setup("predict_u8", (), n, n, x.shape[1:3], self._predict_bytes(n, return_logits), mean, std)
        oh, ow = (h, w) if out_size is None else (int(out_size[0]), int(out_size[1]))
        mask = torch.empty((n, oh, ow), dtype=torch.uint8, device=x.device)
        logits = torch.empty((n, h, w, self._cp), dtype=torch.float32, device=x.device) if return_logits else None
        with L.on_device(x):
            L.check(L.lib().uwm_predict_u8(self._h, ptr(x), mean_c, std_c, float(threshold), int(apply_sigmoid), oh, ow, ptr(mask), ptr(logits),
                                           ptr(ws), ws.numel(), n, h, w, C.c_void_p(L.stream_ptr(x.device))), SegmentationModelError)
        return (mask, self._logits_view(logits)) if return_logits else mask

    @torch.no_grad()
    def predict_images_u8(self, packed: torch.Tensor, in_descs: torch.Tensor, out_descs: torch.Tensor, mask: torch.Tensor, n: int,
                          size, mean, std, threshold: float = 0.5, apply_sigmoid: bool = False, return_logits: bool = False):
        """A packed ragged batch of n uint8 images of any sizes (data.pack_images; `packed` flat uint8, `in_descs` / `out_descs` the
        bytes of the uwm_image_desc arrays, all on the HIP device) -> every image's uint8 {0,255} mask at its own size, written into
        the flat uint8 buffer `mask` at out_descs' offsets, in ONE library call (uwm_predict_images_u8): cv2-convention resize to
        `size` = (H, W) + Normalize into the forward's input, eval forward (frozen or not), resize back + threshold.  Nothing in the
        call depends on the image sizes, so a graph captured around it serves every batch of n images.  Returns `mask`
        [, logits (n,classes,H,W)]."""
        n = int(n)
        h, w, ws, _, mean_c, std_c = self._eval_call_setup("predict_images_u8", (packed, in_descs, out_descs, mask), n, n, size,
                                                           self._predict_bytes(n, return_logits), mean, std)
        logits = torch.empty((n, h, w, self._cp), dtype=torch.float32, device=packed.device) if return_logits else None
        with L.on_device(packed):
            L.check(L.lib().uwm_predict_images_u8(self._h, ptr(packed), packed.numel(), ptr(in_descs), mean_c, std_c, float(threshold),
                                                  int(apply_sigmoid), ptr(out_descs), ptr(mask), mask.numel(), ptr(logits), ptr(ws), ws.numel(),
                                                  n, h, w, C.c_void_p(L.stream_ptr(packed.device))), SegmentationModelError)
        return (mask, self._logits_view(logits)) if return_logits else mask

    @torch.no_grad()
    def predict_tiled_u8(self, packed: torch.Tensor, in_descs: torch.Tensor, out_descs: torch.Tensor, mask: torch.Tensor, n: int,
                         tiles: torch.Tensor, plans: torch.Tensor, k: int, batch: int, size, overlap: int, mean, std,
                         threshold: float = 0.5, apply_sigmoid: bool = False, logits_out: Optional[torch.Tensor] = None):
        """A packed ragged batch of n uint8 images (as predict_images_u8 takes it) at NATIVE resolution, in ONE library call
        (uwm_predict_tiled_u8): `tiles` / `plans` are the bytes of tiling.plan_batch's tables on the HIP device, `k` the number of
        tile entries (a multiple of the forward batch `batch`), `size` = (T_h, T_w) the tile = the model's input size.  Per chunk of
        `batch` tiles: gather + Normalize into the forward's input, eval forward (frozen or not), the logit planes into the tile-logit
        store; then one blend into `mask` at out_descs' offsets and, where given, into the float32 tensor `logits_out` (mask.numel()
        floats, the same offsets).  Nothing in the call depends on the image sizes beyond k, so a graph captured around it serves every
        batch of n images with k tile entries.  Returns `mask`; the store [k][T_h][T_w] of the call stays readable as
        `self._tile_store` (a view of the workspace's tail)."""
        n, k, batch = int(n), int(k), int(batch)
        if plans.numel() < 16 * n:
            raise RuntimeError(f"predict_tiled_u8: {n} images need {16 * n} plan bytes")
        if k < 1 or batch < 1 or k % batch or tiles.numel() < 16 * k:
            raise RuntimeError(f"predict_tiled_u8: k = {k} tile entries must be a multiple of the batch {batch} and need {16 * k} table bytes")
        self._check_logits_out("predict_tiled_u8", logits_out, mask)
        h, w, ws, need, mean_c, std_c = self._eval_call_setup(
            "predict_tiled_u8", (packed, in_descs, out_descs, mask, tiles, plans), n, batch, size,
            lambda h, w: L.lib().uwm_predict_tiled_workspace_bytes(self._h, batch, k, h, w), mean, std)
        self._tile_store = ws[need - 4 * k * h * w: need].view(torch.float32).view(k, h, w)
        with L.on_device(packed):
            L.check(L.lib().uwm_predict_tiled_u8(self._h, ptr(packed), packed.numel(), ptr(in_descs), n, ptr(tiles), k, ptr(plans), h, w,
                                                 int(overlap), mean_c, std_c, float(threshold), int(apply_sigmoid), ptr(out_descs), ptr(mask),
                                                 mask.numel(), ptr(logits_out), ptr(ws), need, batch, C.c_void_p(L.stream_ptr(packed.device))),
                    SegmentationModelError)
        return mask

    def _check_logits_out(self, name: str, logits_out, mask):
        if logits_out is not None:
            self._require_gpu(logits_out)
            if logits_out.dtype != torch.float32 or not logits_out.is_contiguous() or logits_out.numel() < mask.numel():
                raise RuntimeError(f"{name}: logits_out must be a contiguous float32 tensor of at least {mask.numel()} elements")

    @torch.no_grad()
    def predict_images_tta_u8(self, packed: torch.Tensor, in_descs: torch.Tensor, out_descs: torch.Tensor, mask: torch.Tensor, n: int,
                              batch: int, size, views: int, mean, std, threshold: float = 0.5, apply_sigmoid: bool = False):
        """predict_images_u8 with test-time augmentation, in ONE library call (uwm_predict_images_tta_u8): every image goes through the
        eval forward under each view of the bitmask `views` (tta.view_mask), `batch` slots at a time, and the logit planes are mapped
        back and averaged (the mean of the logits, summed in ascending view order) before the resize back + threshold.  Nothing in
        the call depends on the image sizes, so a graph captured around it serves every batch of n images.  Returns `mask`; the
        merged planes (n, H, W) of the call stay readable as `self._merged_store` (a view of the workspace's tail)."""
        n, batch, views = int(n), int(batch), int(views)
        h, w, ws, need, mean_c, std_c = self._eval_call_setup(
            "predict_images_tta_u8", (packed, in_descs, out_descs, mask), n, batch, size,
            lambda h, w: L.lib().uwm_predict_images_tta_workspace_bytes(self._h, batch, h, w, n, views), mean, std)
        self._merged_store = ws[need - 4 * n * h * w: need].view(torch.float32).view(n, h, w)
        with L.on_device(packed):
            L.check(L.lib().uwm_predict_images_tta_u8(self._h, ptr(packed), packed.numel(), ptr(in_descs), n, views, mean_c, std_c, float(threshold),
                                                      int(apply_sigmoid), ptr(out_descs), ptr(mask), mask.numel(), ptr(None), ptr(ws), need, batch, h, w,
                                                      C.c_void_p(L.stream_ptr(packed.device))), SegmentationModelError)
        return mask

    @torch.no_grad()
    def predict_tiled_tta_u8(self, packed: torch.Tensor, in_descs: torch.Tensor, out_descs: torch.Tensor, mask: torch.Tensor, n: int,
                             tiles: torch.Tensor, plans: torch.Tensor, k: int, batch: int, size, overlap: int, views: int, mean, std,
                             threshold: float = 0.5, apply_sigmoid: bool = False, logits_out: Optional[torch.Tensor] = None):
        """predict_tiled_u8 with test-time augmentation, in ONE library call (uwm_predict_tiled_tta_u8): every tile goes through the
        eval forward under each view of the bitmask `views`, `batch` slots at a time; the store [k][T_h][T_w] (`self._tile_store`)
        holds the merged tile logits and the blend runs on it as it does without views."""
        n, k, batch, views = int(n), int(k), int(batch), int(views)
        if plans.numel() < 16 * n or k < 1 or tiles.numel() < 16 * k:
            raise RuntimeError(f"predict_tiled_tta_u8: {n} images need {16 * n} plan bytes and k = {k} tile entries {16 * k} table bytes")
        self._check_logits_out("predict_tiled_tta_u8", logits_out, mask)
        h, w, ws, need, mean_c, std_c = self._eval_call_setup(
            "predict_tiled_tta_u8", (packed, in_descs, out_descs, mask, tiles, plans), n, batch, size,
            lambda h, w: L.lib().uwm_predict_tiled_tta_workspace_bytes(self._h, batch, k, h, w, views), mean, std)
        self._tile_store = ws[need - 4 * k * h * w: need].view(torch.float32).view(k, h, w)
        with L.on_device(packed):
            L.check(L.lib().uwm_predict_tiled_tta_u8(self._h, ptr(packed), packed.numel(), ptr(in_descs), n, ptr(tiles), k, ptr(plans), h, w,
                                                     int(overlap), mean_c, std_c, float(threshold), int(apply_sigmoid), ptr(out_descs), ptr(mask),
                                                     mask.numel(), ptr(logits_out), ptr(ws), need, batch, views,
                                                     C.c_void_p(L.stream_ptr(packed.device))), SegmentationModelError)
        return mask

    @torch.no_grad()
    def filter_images_u8(self, packed: torch.Tensor, in_descs: torch.Tensor, out_descs: torch.Tensor, counts: torch.Tensor, n: int,
                         size, mean, std, threshold: float = 0.5, post_process: bool = True, mask: Optional[torch.Tensor] = None,
                         return_logits: bool = False):
        """The reference's watermark_filter.py for a packed ragged batch of n uint8 images (as predict_images_u8 takes it), in ONE
        library call (uwm_filter_images_u8): resize to `size` + Normalize, eval forward (frozen or not), then per image at its own
        size sigmoid -> bilinear resize of the PROBABILITIES -> threshold -> [open, close with the 3 x 3 cross] -> the foreground
        count.  `counts`: an int64 (n, 2) device tensor that receives {foreground pixels, h_i * w_i}; `mask`: absent, no mask is
        written at all; else the flat uint8 buffer that receives every mask at out_descs' offsets.  Capturable like
        predict_images_u8.  Returns `counts` [, logits (n,classes,H,W)]."""
        n = int(n)
        self._require_gpu(counts)
        if counts.dtype != torch.int64 or counts.numel() < 2 * n or not counts.is_contiguous():
            raise RuntimeError(f"filter_images_u8: counts must be a contiguous int64 tensor of at least ({n}, 2)")
        h, w, ws, _, mean_c, std_c = self._eval_call_setup("filter_images_u8", (packed, in_descs, out_descs) + (() if mask is None else (mask,)), n, n,
                                                           size, self._predict_bytes(n, return_logits), mean, std)
        need = L.lib().uwm_filter_workspace_bytes(n)
        if need == 0:
            raise SegmentationModelError(L.lib().uwm_last_error().decode(errors="replace"))
        fws = getattr(self, "_filter_ws", None)
        if fws is None or fws.numel() < need or fws.device != packed.device:
            fws = self._filter_ws = torch.empty(need, dtype=torch.uint8, device=packed.device)      # (a captured graph's owner keeps its own reference)
        logits = torch.empty((n, h, w, self._cp), dtype=torch.float32, device=packed.device) if return_logits else None
        with L.on_device(packed):
            L.check(L.lib().uwm_filter_images_u8(self._h, ptr(packed), packed.numel(), ptr(in_descs), mean_c, std_c, float(threshold),
                                                 int(bool(post_process)), ptr(out_descs), ptr(mask), mask.numel() if mask is not None else 0,
                                                 ptr(counts), ptr(logits), ptr(ws), ws.numel(), ptr(fws), fws.numel(), n, h, w,
                                                 C.c_void_p(L.stream_ptr(packed.device))), SegmentationModelError)
        return (counts, self._logits_view(logits)) if return_logits else counts

    def _set_drop_connect(self, n: int, training: bool, device):
        """Draw this step's per-block, per-sample keep masks (efficientnet_pytorch utils.drop_connect: floor(keep_prob +
        U[0,1)) / keep_prob) on the device and hand them to the library; the tensor lives until the next forward."""
        if not (training and self.drop_connect):
            self._rowscale = None
            L.check(L.lib().uwm_set_drop_connect(self._h, None))
            return
        kp = getattr(self, "_keep_prob", None)
        if kp is None or kp.device != device:           # (cached: a host-to-device copy has no place in a captured step)
            kp = self._keep_prob = 1.0 - torch.tensor(self._mb_drop, dtype=torch.float32, device=device).view(-1, 1)
        keep_prob = kp
        if self._keep_override is not None:
            keep = self._keep_override.to(device=device, dtype=torch.float32).reshape(self._n_mb, n)
        else:
            keep = torch.floor(keep_prob + torch.rand((self._n_mb, n), dtype=torch.float32, device=device))
        self._rowscale = (keep / keep_prob).contiguous()
        L.check(L.lib().uwm_set_drop_connect(self._h, C.c_void_p(self._rowscale.data_ptr())))

    def _backward_raw(self, dlogits: torch.Tensor, stage_begin: int = 0, stage_end: Optional[int] = None):
        """dlogits [N,H,W,CP] (padding channels zero) -> gradient arena (overwritten)."""
        if stage_end is None:
            stage_end = len(self.stages)
        L.check(L.lib().uwm_backward(self._h, C.c_void_p(dlogits.data_ptr()), C.c_void_p(self._ws.data_ptr()),
                                     stage_begin, stage_end, C.c_void_p(L.stream_ptr(dlogits.device))))

    def debug_buffer(self, key: str) -> torch.Tensor:
        """Flat fp32 view of a planned workspace buffer (see uwm_debug_lookup) — for parity tests."""
        off, cnt = C.c_longlong(), C.c_longlong()
        L.check(L.lib().uwm_debug_lookup(self._h, key.encode(), C.byref(off), C.byref(cnt)))
        return self._ws.view(torch.float32)[off.value: off.value + cnt.value]

    def _logits_view(self, logits_nhwc: torch.Tensor) -> torch.Tensor:
        return logits_nhwc[..., : self.classes].permute(0, 3, 1, 2)

    def _as_padded_dlogits(self, g: torch.Tensor) -> torch.Tensor:
        n, c, h, w = g.shape
        cp = self._cp
        gp = g.permute(0, 2, 3, 1)
        if (getattr(g, "_uwm_padded", False) or g.data_ptr() in _PADDED_PTRS) and gp.stride()[:3] == (h * w * cp, w * cp, cp) \
                and (c == 1 or gp.stride(3) == 1):
            return gp
        dl = torch.zeros((n, h, w, cp), dtype=torch.float32, device=g.device)
        dl[..., :c] = gp
        return dl

    # ------------------------------------------------------------------ nn.Module protocol
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        needs_grad = torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self._plist)
        if needs_grad:
            return _UnetFunction.apply(self, x, *self._plist)
        return self._logits_view(self._forward_raw(x, training=self.training))

    @torch.no_grad()
    def predict(self, x):
        if self.training:
            self.eval()
        return self.forward(x)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                L.lib().uwm_destroy(self._h)
                self._h = None
        except Exception:
            pass


# data_ptrs of dlogits buffers whose padding channels are known to be zero (written by uwm_loss)
_PADDED_PTRS: set = set()


class UnetPlusPlus(Unet):
    """MI355X-native UNet++ (smp.UnetPlusPlus: ResNet-18/34 encoder, dense x_{depth}_{layer} decoder grid) — the
    reference's default architecture (MODEL.NAME, /root/reference/src/configs/config.py:15).  Same constructor
    surface, arenas, kernels and training path as `Unet`; state_dict keys `decoder.blocks.x_0_0.conv1.0.weight` ..."""
    _ARCH = "UnetPlusPlus"


# ---------------------------------------------------------------------------- factory (reference L3 glue)
SUPPORTED_MODELS = {"Unet": Unet, "UnetPlusPlus": UnetPlusPlus}


def create_model(model_name: str, encoder_name: str = "resnet34", encoder_weights: Optional[str] = None,
                 in_channels: int = 3, classes: int = 1, activation=None, **kwargs) -> nn.Module:
    """Counterpart of SMPModelFactory.create_model (/root/reference/src/models/unet_model.py:30-73)."""
    if model_name not in SUPPORTED_MODELS:
        raise ValueError(f"Unsupported model: {model_name}. Supported models: {list(SUPPORTED_MODELS.keys())}")
    return SUPPORTED_MODELS[model_name](encoder_name=encoder_name, encoder_weights=encoder_weights,
                                        in_channels=in_channels, classes=classes, activation=activation, **kwargs)


def create_model_from_config(cfg) -> nn.Module:
    """Counterpart of create_model_from_config (/root/reference/src/models/unet_model.py:93-120)."""
    m = cfg.MODEL
    params = dict(model_name=m.NAME, encoder_name=m.ENCODER_NAME, encoder_weights=m.ENCODER_WEIGHTS,
                  in_channels=m.IN_CHANNELS, classes=m.CLASSES, activation=m.ACTIVATION)
    if hasattr(m, "ENCODER_DEPTH"):
        params["encoder_depth"] = m.ENCODER_DEPTH
    if hasattr(m, "DECODER_CHANNELS"):
        params["decoder_channels"] = m.DECODER_CHANNELS
    return create_model(**params)
