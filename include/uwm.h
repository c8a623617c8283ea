/* libuwm — C ABI of the MI355X-native U-Net watermark-segmentation hot path.
 *
 * This is the drop-in boundary for ONE path of Dave-he/unet-watermark: the forward / backward of
 * smp.Unet | smp.UnetPlusPlus (encoders resnet18 | resnet34 | resnet50 | efficientnet-b0 .. b7; UnetPlusPlus is the
 * reference's default MODEL.NAME, src/configs/config.py:15) and its Dice + BCE loss, which the reference reaches through
 *   model = smp.Unet(**kwargs)                /root/reference/src/models/unet_model.py:17-27,64-71,93-120
 *   outputs = model(images)                    /root/reference/src/train.py:91,100,142 ; src/predict.py:339,611
 *   loss = criterion(outputs, masks)           /root/reference/src/train.py:94,103 ; src/utils/losses.py:11-52
 *   loss.backward(); optimizer.step()          /root/reference/src/train.py:96-98,104-105
 *   metrics(sigmoid(outputs), masks)           /root/reference/src/train.py:110-117 ; src/utils/metrics.py:11-37
 *   (mask > THRESHOLD) * 255                   /root/reference/src/predict.py:614-625
 * plus the data-parallel gradient exchange the reference lacks: uwm_allreduce_grads over RCCL.
 * The reference is pure Python and has no FFI of its own; INTEGRATION.md shows the ctypes stub a
 * maintainer adds (unet-watermark_amd/_lib.py is that stub).
 *
 * Conventions
 *   - plain pointers and sizes only; every device buffer is CALLER-OWNED (e.g. a torch tensor's
 *     data_ptr()); the library never allocates or frees device memory, never synchronises the
 *     host and enqueues all work on the caller's stream (a hipStream_t passed as void*).
 *   - every function returns 0 on success, non-zero on failure; uwm_last_error() then returns a
 *     thread-local message.  A handle is bound to one device — the device its arenas live on (uwm_bind reads it from
 *     the parameter pointer); uwm_forward / uwm_backward / uwm_allreduce_grads make that device current for the
 *     duration of the call, so the caller's current device need not match.  The free functions (uwm_loss, uwm_adam,
 *     uwm_stats ...) launch on the caller's stream and expect that stream's device to be current.  Not re-entrant.
 *   - activations are NHWC fp32 with channels padded to a multiple of 4; logits are returned as
 *     [N][H][W][CP], CP = uwm_logits_channels() (class k at channel k).
 *   - parameters live in ONE flat fp32 arena (caller-owned) whose layout the library defines:
 *     uwm_tensor_info_get() gives, per smp-compatible state_dict key, the arena offset plus logical
 *     OIHW shape and element strides (convolution weights are stored [O][kh][kw][I] with each
 *     output-channel row padded to a multiple of 32 floats).  Gradients use the same layout in a
 *     second arena; BatchNorm running statistics live in a third ("buffer") arena.
 */
#ifndef UWM_H
#define UWM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct uwm_model* uwm_handle;
typedef void* uwm_stream;              /* hipStream_t */

enum { UWM_ENC_RESNET18 = 18, UWM_ENC_RESNET34 = 34, UWM_ENC_RESNET50 = 50,     /* 50: Bottleneck blocks (unet_watermark_large.yaml) */
       /* MBConv blocks: efficientnet_pytorch's compound-scaled family; b4 = README.md:173-176 / BASELINE config 4, b3 = the
        * text-watermark config (unet_text_watermark.yaml) */
       UWM_ENC_EFFICIENTNET_B0 = 100, UWM_ENC_EFFICIENTNET_B1 = 101, UWM_ENC_EFFICIENTNET_B2 = 102,
       UWM_ENC_EFFICIENTNET_B3 = 103, UWM_ENC_EFFICIENTNET_B4 = 104, UWM_ENC_EFFICIENTNET_B5 = 105,
       UWM_ENC_EFFICIENTNET_B6 = 106, UWM_ENC_EFFICIENTNET_B7 = 107 };
enum { UWM_ARCH_UNET = 0, UWM_ARCH_UNETPLUSPLUS = 1 };   /* smp.Unet | smp.UnetPlusPlus (the reference's default MODEL.NAME, src/configs/config.py:15) */
enum { UWM_T_F32 = 0, UWM_T_I64 = 1, UWM_T_U8 = 2, UWM_T_I32 = 3 };          /* target dtypes */
enum { UWM_KIND_CONV_W = 0, UWM_KIND_BIAS = 1, UWM_KIND_BN_GAMMA = 2, UWM_KIND_BN_BETA = 3,
       UWM_KIND_BN_MEAN = 4, UWM_KIND_BN_VAR = 5 };
enum { UWM_ARENA_PARAM = 0, UWM_ARENA_BUFFER = 1 };
enum { UWM_PREC_F32 = 0, UWM_PREC_BF16X3 = 1, UWM_PREC_BF16X3_ALL = 2, UWM_PREC_F16X3 = 3, UWM_PREC_F16X3_ALL = 4,
       UWM_PREC_F16X1 = 5, UWM_PREC_F16X3_BWD2 = 6 };       /* uwm_set_precision */

/* mirrors smp.Unet(encoder_name, encoder_depth=5, decoder_channels, in_channels, classes) */
typedef struct {
  int encoder;                 /* UWM_ENC_* */
  int in_channels;             /* 1..4 */
  int classes;                 /* >= 1 */
  int decoder_channels[5];     /* e.g. 256,128,64,32,16 ; each a multiple of 4 */
  float bn_eps;                /* 1e-5 */
  float bn_momentum;           /* 0.1 */
  int arch;                    /* UWM_ARCH_* ; decoder of src/models/unet_model.py:19 (create_model_from_config) */
} uwm_unet_desc;

typedef struct {
  char name[96];               /* smp state_dict key, e.g. "encoder.layer1.0.conv1.weight" */
  int kind;                    /* UWM_KIND_* */
  int arena;                   /* UWM_ARENA_PARAM | UWM_ARENA_BUFFER */
  int ndim;                    /* 4 for conv weights, 1 otherwise */
  long long offset;            /* element offset into the arena */
  long long shape[4];          /* logical shape (OIHW for conv weights) */
  long long stride[4];         /* element strides of that logical view */
} uwm_tensor_info;

const char* uwm_last_error(void);
int uwm_version(void);

int  uwm_create(const uwm_unet_desc* desc, uwm_handle* out);
void uwm_destroy(uwm_handle h);

long long uwm_param_arena_floats(uwm_handle h);     /* incl. padding; padding must stay 0 */
long long uwm_buffer_arena_floats(uwm_handle h);
long long uwm_param_count(uwm_handle h);            /* logical number of trainable scalars */
int  uwm_num_tensors(uwm_handle h);
int  uwm_tensor_info_get(uwm_handle h, int index, uwm_tensor_info* out);
int  uwm_logits_channels(uwm_handle h);

/* number of backward stages (gradient buckets) and the arena range [begin,end) each one
 * completes; stage 0 = head+decoder, then the encoder from its deepest group to the stem (ResNet: layer4, layer3,
 * layer2, layer1+stem; EfficientNet-b4: blocks 22-31, 10-21, 6-9, 0-5+stem). */
int  uwm_num_stages(uwm_handle h);
int  uwm_stage_range(uwm_handle h, int stage, long long* begin, long long* end);

/* Bind caller-owned device arenas.  grads may be NULL for inference-only use. */
int  uwm_bind(uwm_handle h, float* params, float* grads, float* buffers);

size_t uwm_workspace_bytes(uwm_handle h, int N, int H, int W, int training);
/* algorithmic (direct-convolution) FLOPs per image at H x W: forward, and forward + backward (= 3x forward minus the
 * stem's dgrad) — SURVEY.md 8(d)'s roofline numerator (62.512 / 186.303 GFLOP for Unet-resnet34 at 512x512) */
int  uwm_conv_flops(uwm_handle h, int H, int W, double* fwd, double* fwd_bwd);

/* logits[N][H][W][CP] = Unet(x[N][Cin][H][W]).  training!=0: BatchNorm uses batch statistics,
 * updates running stats, and the workspace keeps what uwm_backward needs.  H, W % 32 == 0. */
int  uwm_forward(uwm_handle h, const float* x_nchw, float* logits, void* workspace, size_t workspace_bytes,
                 int N, int H, int W, int training, uwm_stream stream);

/* ---- Frozen-weight inference.  An eval forward derives three things from the parameters and buffers alone: the scale / shift of
 * every BatchNorm (from gamma, beta and the running statistics), the forward filter bank of every layer that has one (fp32
 * Winograd, bf16x3 Winograd or fp16x3, as the modes ask) and the stem's fp16x3 bank.  An unfrozen handle recomputes them in every
 * uwm_forward(training = 0).  A FROZEN handle computed them once, in uwm_freeze, into a caller-owned device arena; its eval
 * forwards read the arena and launch no weight-preparation kernel.  The results do not change: the same convolution kernels
 * run on banks with the same bits and on the same scale / shift values, so frozen logits equal unfrozen ones bit for bit.
 *
 * uwm_frozen_bytes: size of the arena = 2 floats per BatchNorm channel + one forward bank slot per layer that has one (stem
 * included); it follows from the model alone, not from a shape.  No dgrad banks, no repacks: the backward has no part in this.
 *
 * uwm_freeze fills `frozen` (16-byte aligned, >= uwm_frozen_bytes) from the bound arenas under the handle's CURRENT precision
 * mode, Winograd mode, fill threshold and routing batch, for the bank forms an eval forward of shape (N, H, W) selects.
 * Asynchronous on `stream`; forwards that use the arena must be ordered behind it.  The library writes the arena nowhere else:
 * it is immutable until uwm_unfreeze or the next uwm_freeze, so a hipGraph captured from a frozen forward stays valid while
 * eager forwards of other shapes run between its replays (the workspace's own copy of these items offers no such promise).
 *
 * uwm_forward(training = 0) and uwm_predict_u8 on a frozen handle: if every layer's bank form for the call's (N, H, W) under the
 * current modes equals the frozen one (uwm_frozen_serves tells in advance), scale / shift and banks come from the arena.
 * Otherwise the call takes the unfrozen path, in the workspace, and leaves the arena alone: same result, just not faster.
 * With the routing pinned (uwm_set_precision_fill(h, 1) or a routing batch) the forms no longer depend on N, and an arena
 * frozen at one batch serves every batch of that image size.
 *
 * What unfreezes: uwm_unfreeze; uwm_bind; uwm_forward(training = 1) (the running statistics move).  A caller that changes the
 * parameters or buffers in ANY other way (an optimizer step, a copy into the arenas, ...) must call uwm_unfreeze or uwm_freeze
 * again itself: the library cannot see such writes, and a frozen forward would go on using the old values.
 *
 * uwm_prep_launches: host-side counter (like the routing record: no device work, no effect on results) of the weight-preparation
 * launches this handle has enqueued since uwm_create: one per BatchNorm scale / shift launch (per layer in an unfrozen eval
 * forward, one bn_eval_multi launch per 128 BatchNorms in uwm_freeze), one per batch of forward bank builders, one per stem
 * bank builder; uwm_freeze's own launches count.  It stands still across forwards served from the arena. */
size_t uwm_frozen_bytes(uwm_handle h);
int  uwm_freeze(uwm_handle h, void* frozen, size_t bytes, int N, int H, int W, uwm_stream stream);
int  uwm_unfreeze(uwm_handle h);
int  uwm_is_frozen(uwm_handle h);
int  uwm_frozen_serves(uwm_handle h, int N, int H, int W);     /* 1: an eval forward of this shape would read the arena now */
long long uwm_prep_launches(uwm_handle h);

/* Image bytes to mask bytes in one call: images uint8 [N][H][W][C] (C = the model's in_channels, 4-byte aligned) are normalised
 * ((v / 255 - mean) / std, mean / std host pointers) straight into the forward's NHWC4 input buffer, the eval forward runs
 * (frozen or not), and the logit plane of class 0 is resized to out_h x out_w and thresholded as uwm_resize_threshold does:
 * mask uint8 [N][out_h][out_w] in {0, 255}.  logits (may be NULL): [N][H][W][CP] as uwm_forward writes them; with NULL they
 * live behind the plan in the workspace, which must then hold uwm_predict_workspace_bytes(h, N, H, W, 1) bytes (else
 * uwm_workspace_bytes(h, N, H, W, 0) = uwm_predict_workspace_bytes(.., 0)).  Masks and logits equal, bit for bit, the sequence
 * uwm_preprocess_u8(flags = NULL) -> uwm_forward(training = 0) -> uwm_resize_threshold.  Capturable in a hipGraph like uwm_forward. */
size_t uwm_predict_workspace_bytes(uwm_handle h, int N, int H, int W, int with_logits);
int  uwm_predict_u8(uwm_handle h, const uint8_t* images, const float* mean, const float* std, float threshold,
                    int apply_sigmoid, int out_h, int out_w, uint8_t* mask, float* logits, void* workspace,
                    size_t workspace_bytes, int N, int H, int W, uwm_stream stream);

/* Images of ANY size, device-resident from their bytes to masks at each image's own size: the reference's predict path
 * (A.Resize(IMG_SIZE, IMG_SIZE) = cv2.resize INTER_LINEAR on the uint8 image, src/utils/dataset.py:391-393; cv2.resize of the
 * prediction back to the original size + threshold, src/predict.py:327-335,620-625).
 *   A ragged batch is ONE buffer `src` of src_bytes bytes (4-byte aligned) plus one uwm_image_desc per image in DEVICE memory
 * (8-byte aligned): image i is h*w*C tightly packed interleaved bytes at src + offset (offset in bytes, 4-byte aligned).  Every
 * launch is sized from N, H, W or from a fixed block count per image, never from the descriptors, so ONE captured hipGraph serves
 * every batch of N images whatever their sizes: overwrite the bytes and the descriptors, replay.  No read leaves
 * [src, src + src_bytes) and no write leaves [mask, mask + mask_bytes): an image whose descriptor does not fit gives zeros / is skipped.
 *   The resize rule (exact integer work after the taps; a restatement of OpenCV 4.x's 8-bit HResizeLinear / VResizeLinear
 * fixed-point path with 11 coefficient bits, and of resizeNN — written from the source, NOT run against cv2).  One axis, dst
 * samples from src:
 *     scale = 1.0 / ((double)dst / (double)src)                                   doubles, in this order
 *     LINEAR   f = (float)((d + 0.5) * scale - 0.5); s = floor(f); f -= s; s < 0: f = 0, s = 0; s >= src - 1: f = 0, s = src - 1
 *              taps (s, min(s + 1, src - 1)), weights a0 = rint((1.f - f) * 2048), a1 = rint(f * 2048)      (round half to even)
 *     NEAREST  s = min((int)floor(d * scale), src - 1)
 *   and a pixel, per channel, with column taps (sx, sx1, a0, a1) and row taps (sy, sy1, b0, b1):
 *     S(row) = src[row][sx]*a0 + src[row][sx1]*a1;  dst = (((b0 * (S(sy) >> 4)) >> 16) + ((b1 * (S(sy1) >> 4)) >> 16) + 2) >> 2
 *   (within 0.78 grey levels of float bilinear with align_corners = false on the shapes of tests/test_resize.py; the identity at
 *   equal size.)
 * uwm_resize_u8: -> uint8 [N][H][W][C], C in 1..4.  uwm_op_resize_norm_u8_nhwc4: the LINEAR resize, then Normalize, as fp32
 * [N][H][W][4] (16-byte aligned, padding channels zero) = uwm_resize_u8 -> uwm_op_preprocess_u8_nhwc4 bit for bit.
 * uwm_resize_threshold_ragged: the logit plane [N][h][w] (element stride ld) of image i resized to out_descs[i]'s (h, w) and
 * thresholded into mask + out_descs[i].offset (any alignment) = uwm_resize_threshold on that image bit for bit.
 * uwm_predict_images_u8 = uwm_op_resize_norm_u8_nhwc4 into the forward's input -> eval forward (frozen or not) ->
 * uwm_resize_threshold_ragged; C = the model's in_channels; logits / workspace / N, H, W as uwm_predict_u8 (the same
 * uwm_predict_workspace_bytes).  Capturable, no host synchronisation.  Every argument is checked before any launch. */
typedef struct { long long offset; int h, w; } uwm_image_desc;
enum { UWM_INTER_NEAREST = 0, UWM_INTER_LINEAR = 1 };            /* cv2's values */
int  uwm_resize_u8(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int N, int C, int H, int W, int interp,
                   uint8_t* out, uwm_stream stream);
int  uwm_op_resize_norm_u8_nhwc4(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int N, int C, int H, int W,
                                 const float* mean, const float* std, float* out, uwm_stream stream);
int  uwm_resize_threshold_ragged(const float* logits, int ld, int N, int h, int w, const uwm_image_desc* out_descs, float threshold,
                                 int apply_sigmoid, uint8_t* mask, size_t mask_bytes, uwm_stream stream);
int  uwm_predict_images_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, const float* mean,
                           const float* std, float threshold, int apply_sigmoid, const uwm_image_desc* out_descs, uint8_t* mask,
                           size_t mask_bytes, float* logits, void* workspace, size_t workspace_bytes, int N, int H, int W,
                           uwm_stream stream);

/* Prediction at NATIVE resolution (no counterpart in the reference, which always resizes to IMG_SIZE): every image of a ragged batch
 * (as above) is cut into model-sized overlapping tiles on the device, the tiles go through the eval forward in batches of N, and the
 * tile logits are blended into one plane per image at the image's own size.  (the host side of the plan:
 * unet_watermark_amd/tiling.py.)
 *   The plan, per axis of length len with tile side T (<= 1024) and S = T - overlap, overlap an integer in [0, T / 2]:
 *     len <= T : one tile at origin 0;   len > T : n = ceil((len - T) / S) + 1 tiles at o_j = min(j * S, len - T)
 *   Tiles of an image are ordered row-major (jy outer, jx inner).  The tile table holds one uwm_tile_desc per tile, all images' plans
 *   back to back (`first`: the index of the image's first tile), padded to K entries with image = -1; one uwm_tile_image per image
 *   holds {first, ny, nx}.  Both live in DEVICE memory (4-byte aligned) and are checked there.
 * uwm_op_tile_norm_u8_nhwc4 (the gather): out[k][y][x][c] = Normalize(image[R(y0 + y, h)][R(x0 + x, w)][c]) as fp32 [K][T_h][T_w][4]
 *   (16-byte aligned, padding channels zero), the arithmetic of uwm_op_preprocess_u8_nhwc4; R = BORDER_REFLECT_101
 *   (cv2.borderInterpolate: period 2 (len - 1), len 1 gives 0), which only moves a coordinate where the tile leaves the image.  A tile
 *   is written as zeros when image = -1 or out of range, when its origin is negative or beyond the image, or when the image's
 *   descriptor does not fit [0, src_bytes).  The grid is sized from K and T_h; no read leaves [src, src + src_bytes).
 * uwm_tile_blend_threshold_ragged (the blend): tile_logits is the store [K][T_h][T_w].  Output pixel (y, x) of image i collects the
 *   tiles that cover it in ascending (jy, jx) order; the covering range of an axis follows from (n, S, T, len) by arithmetic.  With
 *   w1(t) = min(t + 1, T - t), t the coordinate inside the tile, and the integer weight w = w1(ty) * w1(tx):
 *     one covering tile:  v = its logit, unchanged
 *     otherwise:          acc = w_0 * l_0;  acc += w_k * l_k in order;  v = acc / sum(w)      every operation rounded to fp32 on its own
 *   mask[out_descs[i].offset + y * w + x] = (apply_sigmoid ? 1.f / (1.f + expf(-v)) : v) > threshold ? 255 : 0, and, where logits_out
 *   is not NULL, logits_out[out_descs[i].offset + y * w + x] = v (a buffer of mask_bytes floats).  One thread per pixel gathers: no
 *   atomics, the result does not depend on the schedule.  An image whose mask region does not fit [0, mask_bytes) is skipped; one
 *   whose plan entry disagrees with the formula or does not fit K, or whose in_descs entry (in_descs may be NULL: not checked) has
 *   another size or does not fit [0, src_bytes) at C bytes per pixel, gets zeros.  No write leaves the outputs.
 * uwm_predict_tiled_u8: for each of the K / N chunks of the tile table (K a multiple of N) the gather into the forward's input, the
 *   eval forward of (N, T_h, T_w) (frozen or not), and a copy of the N logit planes into the store; then one blend.  The workspace
 *   (16-byte aligned, uwm_predict_tiled_workspace_bytes) holds the forward's and, as its last K * T_h * T_w floats, the store.
 *   Capturable: no host synchronisation, allocation or copy; the launch count depends on K / N alone.  Every argument is checked
 *   before any launch. */
typedef struct { int image, y0, x0, first; } uwm_tile_desc;
typedef struct { int first, ny, nx, reserved; } uwm_tile_image;
int    uwm_op_tile_norm_u8_nhwc4(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int num_images,
                                 const uwm_tile_desc* tiles, int K, int C, int T_h, int T_w, const float* mean, const float* std,
                                 float* out, uwm_stream stream);
int    uwm_tile_blend_threshold_ragged(const float* tile_logits, int K, const uwm_tile_image* plans, int num_images, int T_h, int T_w,
                                       int overlap, const uwm_image_desc* in_descs /* may be NULL */, size_t src_bytes, int C,
                                       const uwm_image_desc* out_descs, float threshold, int apply_sigmoid, uint8_t* mask,
                                       size_t mask_bytes, float* logits_out /* may be NULL */, uwm_stream stream);
size_t uwm_predict_tiled_workspace_bytes(uwm_handle h, int N, int K, int T_h, int T_w);
int    uwm_predict_tiled_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, int num_images,
                            const uwm_tile_desc* tiles, int K, const uwm_tile_image* plans, int T_h, int T_w, int overlap,
                            const float* mean, const float* std, float threshold, int apply_sigmoid, const uwm_image_desc* out_descs,
                            uint8_t* mask, size_t mask_bytes, float* logits_out, void* workspace, size_t workspace_bytes, int N,
                            uwm_stream stream);

/* Prediction with TEST-TIME AUGMENTATION (no counterpart in the reference): the network sees every image (or tile) under the views of
 * a set, every logit plane is mapped back, and the planes are averaged before the threshold.  (the host side:
 * unet_watermark_amd/tta.py.)
 *   Views.  A view of an H x W plane is a code c = r + 4 f, r in 0..3, f in 0..1:  view_c(x) = rot90^r(hflip^f(x)) — the horizontal
 *     flip first, then r counter-clockwise quarter turns as torch.rot90(x, r, (H, W)) makes them; one turn of a square of side S:
 *     out[i][j] = in[j][S - 1 - i].  Code 0 is the identity, 4 the horizontal flip, 2 the half turn, 6 the vertical flip.  Codes 1, 3,
 *     5 and 7 need H == W and are refused otherwise.
 *   View sets.  A bitmask `views` in 1..255, bit c = view c, k = popcount(views).  hflip = 0x11, flips = 0x55, d4 = 0xFF, none = 0x01.
 *   Slots.  The network inputs of B items (images, or tiles of a tile table) are slots: slot s = i * k + j is the j-th view of the set,
 *     in ascending code order, of item i.  The forward runs them N at a time; the slot count is padded up to a multiple of N with
 *     all-zero inputs whose logits are ignored.
 *   Merge, at the network's resolution (before the resize back / the tile blend), per pixel:
 *     acc = l'_{c0};  acc += l'_{cj} in ascending code order;  v = acc / (float)k        every operation rounded to fp32 on its own
 *     with l'_c the logit plane of view c mapped back by view_c^-1.  k = 1 with code 0: v is that logit bit for bit (k = 1 does not
 *     divide).  The order is fixed by the slot order, not by the chunking: a view set that straddles two forward chunks gives the same
 *     bits as one that does not (the partial sum waits in the store).  No float atomics.  The sigmoid, where asked for, is applied
 *     to v: this is the mean of the LOGITS, not of the probabilities.
 * A slot range is [slot0, slot0 + num_slots).  The two input calls first write the base planes of the items the range touches into
 *   `stage` (16-byte aligned, uwm_view_stage_bytes(views, num_slots, H, W): at most min(num_slots, (num_slots + k - 2) / k + 1) planes
 *   of [H][W][4] floats — never k copies of a batch) with the existing kernel, then one launch writes every slot's view into out.
 * uwm_op_resize_norm_view_u8_nhwc4: out[s - slot0] = view_c(uwm_op_resize_norm_u8_nhwc4's plane of image s / k), fp32 [num_slots][H][W][4]
 *   (16-byte aligned, padding channel zero); a slot whose image is >= num_images is zeros.
 * uwm_op_tile_norm_view_u8_nhwc4: the same over the K entries of a tile table, on uwm_op_tile_norm_u8_nhwc4's planes.
 * uwm_op_view_merge: logits = the planes [num_slots][H][W] (element stride ld) of the range; store = one plane [H][W] per item,
 *   [num_items] of them.  One thread owns a pixel of an item and walks the views of that item present in the range in slot order: the
 *   first view of an item writes, later views add (to the store where the range starts inside the item), the last divides.  Slots of
 *   items >= num_items are ignored.  A sequence of calls over consecutive ranges gives the same bits as one call over their union.
 * uwm_predict_images_tta_u8: uwm_predict_images_u8 with num_images apart from the forward batch N: per chunk of N slots the viewed
 *   resize + Normalize into the forward's input, the eval forward of (N, H, W) (frozen or not), the merge into the store
 *   [num_images][H][W]; then uwm_resize_threshold_ragged of the store (ld = 1).  merged (may be NULL, 4-byte aligned): the store is
 *   written there instead of the workspace's tail.  views = 0x01 gives uwm_predict_images_u8's masks.
 * uwm_predict_tiled_tta_u8: uwm_predict_tiled_u8 with `views`: the store [K][T_h][T_w] (the workspace's tail) holds MERGED tile logits
 *   and the existing blend runs on it unchanged.  K need not be a multiple of N: the slots K * k are padded instead.
 * All: capturable — no host synchronisation, allocation or copy; ceil(items * k / N) chunks of {base planes, views, forward, merge}
 *   launches and one closing launch, whatever the image sizes.  Every argument is checked before any launch.  An image whose
 *   descriptor does not fit goes in as zeros / has its mask skipped, as in the calls without views, and costs only itself. */
size_t uwm_view_stage_bytes(int views, int num_slots, int H, int W);
int    uwm_op_resize_norm_view_u8_nhwc4(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int num_images, int C, int H,
                                        int W, const float* mean, const float* std, int views, int slot0, int num_slots, float* stage,
                                        size_t stage_bytes, float* out, uwm_stream stream);
int    uwm_op_tile_norm_view_u8_nhwc4(const uint8_t* src, size_t src_bytes, const uwm_image_desc* descs, int num_images,
                                      const uwm_tile_desc* tiles, int K, int C, int T_h, int T_w, const float* mean, const float* std,
                                      int views, int slot0, int num_slots, float* stage, size_t stage_bytes, float* out,
                                      uwm_stream stream);
int    uwm_op_view_merge(const float* logits, int ld, int H, int W, int views, int slot0, int num_slots, int num_items, float* store,
                         uwm_stream stream);
size_t uwm_predict_images_tta_workspace_bytes(uwm_handle h, int N, int H, int W, int num_images, int views);
int    uwm_predict_images_tta_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, int num_images,
                                 int views, const float* mean, const float* std, float threshold, int apply_sigmoid,
                                 const uwm_image_desc* out_descs, uint8_t* mask, size_t mask_bytes, float* merged /* may be NULL */,
                                 void* workspace, size_t workspace_bytes, int N, int H, int W, uwm_stream stream);
size_t uwm_predict_tiled_tta_workspace_bytes(uwm_handle h, int N, int K, int T_h, int T_w, int views);
int    uwm_predict_tiled_tta_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, int num_images,
                                const uwm_tile_desc* tiles, int K, const uwm_tile_image* plans, int T_h, int T_w, int overlap,
                                const float* mean, const float* std, float threshold, int apply_sigmoid, const uwm_image_desc* out_descs,
                                uint8_t* mask, size_t mask_bytes, float* logits_out, void* workspace, size_t workspace_bytes, int N,
                                int views, uwm_stream stream);

/* Masks from watermarked / clean pairs: the reference's WatermarkDataset._generate_mask with use_blurred_mask = False
 * (src/utils/dataset.py:197-211,277-278), which serves every image that has a clean counterpart and no mask file.  wm, clean and mask
 * are ragged batches as above (uint8 RGB interleaved, C = 3; masks one byte per pixel at any alignment); image i, at its OWN size:
 *     d = |wm - clean| per channel                                                 cv2.absdiff
 *     g = (d.R*9798 + d.G*19235 + d.B*3735 + 16384) >> 15                          cvtColor RGB2GRAY, OpenCV 4.x's 8-bit rule (15 bits;
 *                                                                                  3.x used 14: 4899, 9617, 1868) — restated, NOT run
 *     m = g > threshold ? 255 : 0                                                  cv2.threshold THRESH_BINARY
 *     m = open(m, ELLIPSE(3,3) = the cross, 1 iteration)                           the morphology of uwm_optimize_mask below: the erosion
 *                                                                                  ignores pixels outside the image, the dilation reads
 *                                                                                  the eroded plane as 0 there
 *   and the reference's closing GaussianBlur((3,3), 0.5) + threshold 127 is the identity on {0,255} images (see uwm_optimize_mask).
 * A clean image of another size is first brought to the watermarked size by uwm_resize_u8(UWM_INTER_LINEAR): the caller's step.
 * image i: mask_i = open3(gray(|wm_i - clean_i|) > threshold) at the image's own size, into mask + mask_descs[i].offset.
 * clean_descs[i].h == 0: image skipped, its mask bytes untouched (a mask read from a file stays).  Any other misfit
 * (sizes differ, a descriptor leaves its buffer, a side above 2^30): the mask region, if it fits, is zeroed.  open != 0: with the
 * opening; 0: without it.  One launch of N * 64 workgroups on the caller's stream, no workspace, no host synchronisation: capturable,
 * and one captured launch serves every batch of N pairs.  Every argument is checked before any launch (C must be 3, threshold 0..255,
 * wm / clean 4-byte and descriptors 8-byte aligned).  No read leaves [wm, wm+wm_bytes) or [clean, clean+clean_bytes), no write leaves
 * [mask, mask+mask_bytes). */
int  uwm_pair_mask_u8(const uint8_t* wm, size_t wm_bytes, const uwm_image_desc* wm_descs,
                      const uint8_t* clean, size_t clean_bytes, const uwm_image_desc* clean_descs,
                      int N, int C /* 3 */, int threshold /* 0..255 */, int open,
                      uint8_t* mask, size_t mask_bytes, const uwm_image_desc* mask_descs, uwm_stream stream);

/* Logo-watermarked training samples: the LOGO branch of the reference's src/scripts/gen_data.py (apply_watermark_effects,
 * resize_watermark, generate_multiple_watermarks_image / generate_watermarked_image, calculate_overlap_area, and main()'s
 * single/multi and transparent/normal choices).  Text and mixed watermarks are uwm_synth_text_u8's, below; the JPEG quality=95 save
 * is uwm_jpeg_ragged_u8's; a device-resident logo bank is NOT served.  A JOB is one logo on one image.  The HOST draws every random number, computes every size and does the placement
 * loop (data.sample_synth_jobs); the device only executes descriptors, so a batch is a pure function of its inputs.  Stages, in
 * order, on an RGBA patch (uint8, R G B A interleaved); MULDIV255(x, y) = (t = x*y + 128, ((t >> 8) + t) >> 8):
 *   1 RESIZE to (w1, h1) = Image.resize(LANCZOS) on RGBA.  Equal size: a copy.  Else premultiply c = MULDIV255(c, a); the horizontal
 *     pass, then the vertical pass, each to uint8 and each skipped when its side does not change; unpremultiply: a == 0 or 255
 *     copies, else min(255, (255*c) / a) (integer division).  Coefficients per axis (in -> out), all float64, Pillow's
 *     precompute_coeffs: scale = in/out; fs = max(scale, 1.0); support = 3.0*fs; ksize = (int)ceil(support)*2 + 1; ss = 1.0/fs;
 *     for output xx: center = (xx + 0.5)*scale; xmin = max((int)(center - support + 0.5), 0);
 *     xmax = min((int)(center + support + 0.5), in) - xmin; w[x] = lanczos((x + xmin - center + 0.5)*ss);
 *     lanczos(x) = sinc(x)*sinc(x/3) on -3 <= x < 3, else 0; sinc(0) = 1, sinc(x) = sin(pi*x)/(pi*x); ww = the sequential sum of w;
 *     w /= ww when ww != 0; k = (int)(w*2^22 + 0.5), or - 0.5 for w < 0.  Pixel: clip8(((1 << 21) + sum k*p) >> 22).
 *   2 ROTATE (rotate != 0) = Image.rotate(angle, expand=True), NEAREST, fill 0.  Host, as Image.rotate: a = -radians(angle % 360);
 *     rot = [round(cos a, 15), round(sin a, 15), 0, round(-sin a, 15), round(cos a, 15), 0] about the centre (w/2, h/2); (w2, h2) from
 *     ceil(max) - floor(min) of the four transformed corners; the final translation.  angle % 360 == 0 is the identity (rotate = 0).
 *     Device, Pillow's affine_fixed, FIX(v) = floor(v*65536 + 0.5): a2 = FIX(m2 + m0/2 + m1/2), a5 = FIX(m5 + m3/2 + m4/2),
 *     xin = (a2 + a1*y + a0*x) >> 16, yin = (a5 + a4*y + a3*x) >> 16; outside the source gives 0.
 *   3 STRETCH (stretch != 0): stage 1 again, to (w3, h3).  Then, shear != 0: cv2.warpAffine(M = [[1, sx, 0], [sy, 1, 0]] as float32,
 *     (w, h), INTER_LINEAR, BORDER_CONSTANT 0) on the four channels — restated from knowledge and NOT run against cv2: shear_minv =
 *     OpenCV's float64 inverse (D = 1/(M0*M4 - M1*M3); A11 = M4*D, A22 = M0*D; M1 *= -D, M3 *= -D; b1 = -A11*M2 - M1*M5,
 *     b2 = -M3*M2 - A22*M5) = [A11, M1, b1, M3, A22, b2]; X = (rint((m1*y + m2)*1024) + 16 + rint(m0*x*1024)) >> 5, Y likewise with
 *     m4, m5, m3 (round half to even; 10 coordinate bits, 5 interpolation bits); taps (X >> 5, Y >> 5) and + 1 with weights from
 *     X & 31, Y & 31, out = (acc + 512) >> 10; a tap outside the patch reads 0.
 *   4 BLUR (blur != 0) = ImageFilter.GaussianBlur on all four channels, not premultiplied: three horizontal box passes, then three
 *     vertical, out = (ww*sum_{i=-R..R} p[clamp(x + i)] + fw*(p[clamp(x - R - 1)] + p[clamp(x + R + 1)]) + 2^23) >> 24, edges
 *     replicated.  Host, as Pillow's C (float32 unless said): sigma2 = r*r/3; L = (float)sqrt(12.0*sigma2 + 1.0) (the square root in
 *     double); l = floor((L - 1)/2); a = (2l + 1)*(l*(l + 1) - 3*sigma2) / (6*(sigma2 - (l + 1)^2)); fr = l + a; blur_r = R = (int)fr;
 *     blur_ww = (uint32)(2^24/(2*fr + 1)); blur_fw = (2^24 - (2R + 1)*ww)/2.  R is at most 32.
 *   5 DEFECTS: ndefects (0..3) rectangles {x, y, w, h} get alpha 0.
 *   6 ENHANCE (enhance != 0) = ImageEnhance.Brightness, Contrast, Color: each Image.blend(degenerate, image, f) over RGB, alpha
 *     untouched; in float32 t = d + f*(p - d); 0 <= f <= 1: (uint8)t truncated; else 0 for t <= 0, 255 for t >= 255, else truncated.
 *     Degenerates: Brightness 0; Contrast the constant (int)(mean(L) + 0.5) (float64) over ALL pixels of the patch, transparent ones
 *     included; Color the pixel's own L; L = (19595*R + 38470*G + 7471*B + 0x8000) >> 16.
 *   7 OPACITY: a = opacity[a], the host's table of (uint8)(a*alpha) in float64.
 *   8 PASTE = watermarked.paste(patch, (x, y), patch) and combined_mask.paste(alpha, (x, y), alpha), clipped to the image:
 *     c = MULDIV255-blend: t = src*a + dst*(255 - a) + 128, ((t >> 8) + t) >> 8; the mask likewise with src = a, from 0.  The jobs of
 *     one image are applied in slot order.
 * A PLAIN job (the reference's fallback resize_watermark for an oversized patch) is stage 1 with every other stage off and the
 * identity opacity table.  Stages 1, 2, 4, 6, 7 and 8 are held to Pillow bit for bit by tests/test_synth.py; stage 3's shear is not
 * run against cv2.
 * images: a ragged batch as above (uint8 RGB interleaved), worked on IN PLACE; masks (may be NULL): one byte per pixel, every pixel
 * of a mask whose descriptor equals its image's is written (0 where no logo landed).  logos: a ragged batch of RGBA images, each
 * offset a multiple of 4.  jobs: [N][K] in device memory, K <= 8 slots per image.  The workspace holds, per job, two patch buffers
 * of max_patch_pixels pixels, four coefficient tables of max_taps int32 (a table in -> out takes out*(ksize + 2)) and the partial
 * sums of the Contrast mean.  A job with enabled == 0, or one that does not fit (a logo index or descriptor outside its buffer, a
 * side outside 1..32767, an intermediate or final patch above max_patch_pixels, a table above max_taps, non-finite matrix
 * entries, blur_r above 32, a defect outside 0..32767) is skipped by every stage and costs only itself.  16 launches of
 * N * K * 32 workgroups on the caller's stream, sized from N and K alone, no host synchronisation: capturable, and one captured call
 * serves every batch.  Integer sums have one result whatever their order and every float operation is spelt out, so runs are
 * bit-identical.  The LANCZOS tables are built on the device in float64 (one thread per output index);
 * uwm_op_lanczos_table exposes that builder: int32 [out][2 + ksize] = {xmin, xmax, coefficients}.  uwm_op_synth_patches runs stages
 * 1-7 on J jobs and stores job j's finished patch at out + j*max_patch_pixels*4 (stage-level tests).  Every argument is checked
 * before any launch.  No read leaves the inputs; no write leaves [images, +image_bytes), [masks, +mask_bytes) or the workspace. */
typedef struct uwm_synth_job {
  int enabled;                 /* 0: an empty slot */
  int logo;                    /* index into logo_descs */
  int w1, h1;                  /* stage 1 */
  int rotate, w2, h2;          /* stage 2 and its expanded size */
  int stretch, w3, h3, shear;  /* stage 3 */
  int blur, blur_r;            /* stage 4 */
  unsigned blur_ww, blur_fw;
  int ndefects, defects[3][4]; /* stage 5: {x, y, w, h} */
  int enhance;                 /* stage 6 */
  float brightness, contrast, color;
  int x, y;                    /* stage 8 */
  double rot[6], shear_minv[6];
  uint8_t opacity[256];        /* stage 7 */
} uwm_synth_job;
size_t uwm_synth_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps);
int  uwm_synth_u8(uint8_t* images, size_t image_bytes, const uwm_image_desc* image_descs,
                  uint8_t* masks /* may be NULL */, size_t mask_bytes, const uwm_image_desc* mask_descs,
                  const uint8_t* logos, size_t logo_bytes, const uwm_image_desc* logo_descs, int num_logos,
                  const uwm_synth_job* jobs, int N, int K, long long max_patch_pixels, long long max_taps,
                  void* workspace, size_t workspace_bytes, uwm_stream stream);
int  uwm_op_synth_patches(const uint8_t* logos, size_t logo_bytes, const uwm_image_desc* logo_descs, int num_logos,
                          const uwm_synth_job* jobs, int J, long long max_patch_pixels, long long max_taps,
                          void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_bytes, uwm_stream stream);
int  uwm_lanczos_table_ints(int in, int out);         /* out*(ksize + 2); 0 for a side outside 1..32767 */
int  uwm_op_lanczos_table(int in, int out, int* table /* device */, size_t table_ints, uwm_stream stream);

/* Text-watermarked training samples: the TEXT branch of the reference's src/scripts/gen_data.py (apply_text_effects,
 * generate_text_watermark) and the mask rule of generate_mixed_watermark.  A JOB is one text on one image.  The HOST chooses the text
 * and the font, rasterises the text to a COVERAGE PLANE (one byte per pixel: font.getmask2(text, "L") placed on the canvas of the
 * text's bounding box plus a margin of 20; data.render_text_plane), draws every random number and computes every size
 * (data.sample_text_job); the device only executes descriptors.  Stages, in order, on an RGBA patch; "stage n" is uwm_synth_u8's:
 *   A COLOUR   what ImageDraw.text(fill = ink) leaves on a transparent canvas: coverage c != 0 gives (ink[0], ink[1], ink[2], c),
 *              c == 0 gives (0, 0, 0, 0).
 *   B ROTATE   (rotate != 0) stage 2 to (w2, h2) with rot: Image.rotate(angle, expand=True, fillcolor=(0, 0, 0, 0)).
 *   C SCALE    (scale != 0) stage 1 to (w3, h3): Image.resize(LANCZOS) on RGBA, premultiplied; an equal size is a copy.
 *   D BLUR     (blur != 0) stage 4 with blur_r, blur_ww, blur_fw (the script draws radii 0.5..1.5).
 *   E ENHANCE  Brightness (brighten != 0), then Contrast (recontrast != 0), by stage 6's rule; the Contrast mean is taken over the
 *              brightened patch.  There is no Color step.  A step that is off is that step at factor 1, which is Image.blend's copy.
 *   F OPACITY  stage 7: a = opacity[a].
 *   G FIT      nfit (0..3) further LANCZOS resizes, in order, to fit[f] = {w, h}: the script's "wider than 0.8 W", "taller than
 *              0.8 H" and "still does not fit" rescales, with the sizes the host derived.  An equal size is a copy.
 *   H PASTE    stage 8 into the image at (x, y), clipped; the jobs of one image are applied in slot order.  The mask plane follows
 *              mask_mode.  0: mask.paste(alpha, (x, y), alpha) over what the plane holds (text alone: the caller zeroes the plane).
 *              1: the mixed rule: every byte m of the plane becomes max(m >> 1, t), t the alpha planes pasted from 0 — m >> 1 is
 *              Image.blend(0, m, 0.5) followed by convert("L"); each byte is halved once whatever K is.
 * An image none of whose K jobs runs is left as it is, mask plane included (in mode 1 too: no text, no mixed rule), so one call
 * serves a batch in which only some images carry text.
 * images: a ragged batch (uint8 RGB interleaved), worked on IN PLACE; masks (may be NULL): one byte per pixel, used where a mask's
 * descriptor equals its image's.  planes: a ragged batch of one-channel uint8 images, each offset a multiple of 4.  jobs: [N][K] in
 * device memory, K <= 8.  The workspace holds, per job, two patch buffers of max_patch_pixels pixels, eight coefficient tables of
 * max_taps int32 and the partial sums of the Contrast mean.  A job with enabled == 0, or one that does not fit (a plane index or
 * descriptor outside its buffer, an ink outside 0..255, a side outside 1..32767, the plane or an intermediate or final patch above
 * max_patch_pixels, a table above max_taps, non-finite matrix entries, blur_r above 32, nfit outside 0..3) is skipped by every
 * stage and costs only itself.  20 launches of N * K * 32 workgroups on the caller's stream, sized from N and K alone, no host
 * synchronisation: capturable, and one captured call serves every batch of equal capacities.  Integer sums and spelt-out float
 * operations only: runs are bit-identical.  uwm_op_text_patches runs stages A-G on J jobs and stores job j's finished patch at
 * out + j*max_patch_pixels*4 (stage-level tests).  Every argument is checked before any launch.  No read leaves the inputs; no write
 * leaves [images, +image_bytes), [masks, +mask_bytes) or the workspace.  Held to Pillow through tests/textsynth_ref.py. */
typedef struct uwm_text_job {
  int enabled;                 /* 0: an empty slot */
  int glyph;                   /* index into plane_descs */
  int ink[3];                  /* A */
  int rotate, w2, h2;          /* B and its expanded size */
  int scale, w3, h3;           /* C */
  int blur, blur_r;            /* D */
  unsigned blur_ww, blur_fw;
  int brighten, recontrast;    /* E */
  float brightness, contrast;
  int nfit, fit[3][2];         /* G: {w, h} */
  int x, y;                    /* H */
  double rot[6];
  uint8_t opacity[256];        /* F */
} uwm_text_job;
size_t uwm_synth_text_workspace_bytes(int N, int K, long long max_patch_pixels, long long max_taps);
int  uwm_synth_text_u8(uint8_t* images, size_t image_bytes, const uwm_image_desc* image_descs,
                       uint8_t* masks /* may be NULL */, size_t mask_bytes, const uwm_image_desc* mask_descs, int mask_mode,
                       const uint8_t* planes, size_t plane_bytes, const uwm_image_desc* plane_descs, int num_planes,
                       const uwm_text_job* jobs, int N, int K, long long max_patch_pixels, long long max_taps,
                       void* workspace, size_t workspace_bytes, uwm_stream stream);
int  uwm_op_text_patches(const uint8_t* planes, size_t plane_bytes, const uwm_image_desc* plane_descs, int num_planes,
                         const uwm_text_job* jobs, int J, long long max_patch_pixels, long long max_taps,
                         void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_bytes, uwm_stream stream);

/* The dataset filter: the reference's src/scripts/watermark_filter.py (predict_mask, _post_process_mask, has_watermark), which sorts a
 * folder by the share of each image that the model calls watermark.  Only one integer per image is wanted, so the mask need not leave
 * the kernel.  Image i of a ragged batch, at its OWN size (h_i, w_i) = out_descs[i], from the logit plane [N][h][w] (element stride ld):
 *     p = 1.f / (1.f + expf(-logit))                       at each of the four taps: sigmoid FIRST          (watermark_filter.py:136)
 *     v = bilinear(p)                                      uwm_resize_threshold's interpolation, unchanged: same coordinates, clamps
 *                                                          and order of operations, horizontal inside vertical   (:147, cv2.resize)
 *     m = v > threshold ? 255 : 0                                                                                (:150)
 *     post_process != 0:  m = close(open(m, E), E), E = ELLIPSE(3,3) = the cross, one iteration each            (:164-171)
 *                         with the morphology of uwm_op_morph: an erosion ignores pixels outside the image, a dilation reads its
 *                         input plane as 0 there
 *     counts[i] = {number of pixels with m != 0, h_i * w_i};  mask != NULL: m is also stored at mask + out_descs[i].offset
 *   This is NOT uwm_resize_threshold(apply_sigmoid = 1), which interpolates the logits and applies the sigmoid afterwards; the two
 *   agree without a resize only.  Logits -1 and +5 with weight 0.25 on the second: sigmoid(0.5) = 0.62 > 0.5 logit first,
 *   0.75 * 0.269 + 0.25 * 0.993 = 0.45 < 0.5 probability first.  uwm_resize_threshold* keep their order.
 * A misfit image (a side outside 1 .. 2^30 or, with a mask, a region that leaves [0, mask_bytes)) gets counts[i] = {0, 0} and costs
 * that image only; its mask region is zeroed if that region fits.  mask == NULL: mask_bytes and the offsets are not read.
 * uwm_filter_workspace_bytes(N): the bytes of per-workgroup partial counts (N * 64 * 8; 0 and a message for N < 1 or too large); the
 * counts are integer sums in a fixed order, the same on every run.  uwm_prob_mask_count_ragged: two launches (N * 64 workgroups, then
 * the sum) on the caller's stream, no host synchronisation: capturable, and one captured call serves every batch of N images.
 * uwm_filter_images_u8 = uwm_op_resize_norm_u8_nhwc4 into the forward's input -> eval forward (frozen or not) ->
 * uwm_prob_mask_count_ragged; logits / workspace / N, H, W as uwm_predict_images_u8 (the same uwm_predict_workspace_bytes).
 * Both check every argument before any launch: nulls, N >= 1, ld >= 1, a finite threshold, logits 4-byte, descriptors / counts /
 * filter workspace 8-byte aligned, the workspace sizes.  No read leaves the inputs, no write leaves [mask, mask + mask_bytes),
 * counts[0 .. 2N) or the workspaces. */
size_t uwm_filter_workspace_bytes(int N);
int  uwm_prob_mask_count_ragged(const float* logits, int ld, int N, int h, int w, const uwm_image_desc* out_descs, float threshold,
                                int post_process, uint8_t* mask /* may be NULL */, size_t mask_bytes,
                                long long* counts /* device, [N][2] = {foreground pixels, h_i*w_i} */,
                                void* workspace, size_t workspace_bytes, uwm_stream stream);
int  uwm_filter_images_u8(uwm_handle h, const uint8_t* src, size_t src_bytes, const uwm_image_desc* in_descs, const float* mean,
                          const float* std, float threshold, int post_process, const uwm_image_desc* out_descs,
                          uint8_t* mask /* may be NULL */, size_t mask_bytes, long long* counts, float* logits, void* workspace,
                          size_t workspace_bytes, void* filter_workspace, size_t filter_workspace_bytes, int N, int H, int W,
                          uwm_stream stream);

/* Backward of the last training forward held in `workspace`; writes (overwrites) the gradient arena
 * ranges of stages [stage_begin, stage_end).  Call with (0, uwm_num_stages) for everything, or stage
 * by stage to overlap gradient all-reduce with the rest of the backward. */
int  uwm_backward(uwm_handle h, const float* dlogits, void* workspace, int stage_begin, int stage_end,
                  uwm_stream stream);

/* loss = w_dice*Dice(logits,target) + w_bce*BCEWithLogits(logits,target) over class channel 0.
 * logits [npix][ld]; target [npix] of dtype target_dtype; scratch: >= 64 bytes device memory;
 * loss_out: 3 device floats {total, dice, bce}; dlogits [npix][ldd] (may be NULL) = grad_scale*dL/dlogits. */
int  uwm_loss(const float* logits, int ld, const void* target, int target_dtype, long long npix,
              float w_dice, float w_bce, float smooth, float eps, void* scratch, float* loss_out,
              float* dlogits, int ldd, float grad_scale, uwm_stream stream);

/* The two halves of uwm_loss, for the data-parallel "global Dice" of SURVEY.md 8(e) (Dice is a ratio of batch sums, so the
 * mean of per-rank Dice losses is NOT the Dice of the global batch): uwm_loss_sums leaves the local sums
 * {sum p*t, sum p, sum t, sum bce} as four doubles in scratch[0..3]; the host all-reduces (SUM) those 32 bytes over the ranks
 * (ncclAllReduce / torch.distributed on the same stream); uwm_loss_apply then evaluates loss_out and dlogits of the GLOBAL
 * batch, npix_total = pixels over all ranks.  The parameter gradients of the ranks must then be SUMMED, not averaged: pass
 * grad_scale = world_size here when the exchange averages.  npix_total == npix reproduces uwm_loss. */
int  uwm_loss_sums(const float* logits, int ld, const void* target, int target_dtype, long long npix, void* scratch,
                   uwm_stream stream);
int  uwm_loss_apply(const float* logits, int ld, const void* target, int target_dtype, long long npix, long long npix_total,
                    float w_dice, float w_bce, float smooth, float eps, const void* scratch, float* loss_out,
                    float* dlogits, int ldd, float grad_scale, uwm_stream stream);

/* The rest of the reference's loss menu (LOSS.NAME JaccardLoss | TverskyLoss | FocalLoss, and any weighted mix with Dice and BCE)
 * on one fused pass.  The terms are smp's JaccardLoss / TverskyLoss / FocalLoss in mode='binary', from_logits=True (log_loss,
 * normalized, reduced_threshold, ignore_index: not served), with I = sum p*t, P = sum p, T = sum t over the batch:
 *   jaccard = 1 - (I + smooth) / max(P + T - I + smooth, eps)
 *   tversky = (1 - (I + smooth) / max(I + alpha (P - I) + beta (T - I) + smooth, eps)) ^ gamma
 *   focal   = mean_i a_i (1 - pt_i)^gamma bce_i,  pt_i = exp(-bce_i),  a_i = alpha t_i + (1 - alpha)(1 - t_i), or 1 without alpha
 * Dice and BCE as in uwm_loss; the three region losses are 0 for a batch without foreground (T == 0).  smp's defaults: smooth 0,
 * eps 1e-7, tversky alpha = beta 0.5, gamma 1, focal alpha none, gamma 2. */
typedef struct uwm_loss_spec {
  float w_dice, w_bce, w_jaccard, w_tversky, w_focal;
  float dice_smooth, dice_eps, jaccard_smooth, jaccard_eps, tversky_smooth, tversky_eps;
  float tversky_alpha, tversky_beta, tversky_gamma;   /* gamma > 0 */
  float focal_alpha;                                  /* < 0: none; otherwise <= 1 */
  float focal_gamma;                                  /* >= 0 */
} uwm_loss_spec;
/* loss = sum of the five weighted terms.  Arguments as uwm_loss, except: loss_out: 8 device floats {total, dice, bce, jaccard,
 * tversky, focal, 0, 0} — every term is reported whatever its weight, but focal only when w_focal != 0 (its arithmetic is compiled
 * out of both passes otherwise, and it reads 0); dlogits' padding channels 1..ldd-1 are written as zeros (one 16-byte store per
 * pixel when ldd == 4 and dlogits is 16-byte aligned).  Nothing synchronises with the host.  uwm_loss_ext_sums leaves FIVE doubles
 * {sum p*t, sum p, sum t, sum bce, sum focal} in scratch[0..4] (40 bytes to all-reduce); uwm_loss_ext_apply is the counterpart of
 * uwm_loss_apply, with the same grad_scale = world_size rule.  Both halves must see the same spec. */
int  uwm_loss_ext(const float* logits, int ld, const void* target, int target_dtype, long long npix, const uwm_loss_spec* spec,
                  void* scratch /* >= 64 B */, float* loss_out /* 8 */, float* dlogits /* may be NULL */, int ldd, float grad_scale,
                  uwm_stream stream);
int  uwm_loss_ext_sums(const float* logits, int ld, const void* target, int target_dtype, long long npix, const uwm_loss_spec* spec,
                       void* scratch, uwm_stream stream);
int  uwm_loss_ext_apply(const float* logits, int ld, const void* target, int target_dtype, long long npix, long long npix_total,
                        const uwm_loss_spec* spec, const void* scratch, float* loss_out, float* dlogits, int ldd, float grad_scale,
                        uwm_stream stream);

/* out[N][4] int64 = tp, fp, fn, tn of (v >= threshold), v = sigmoid(logit) if apply_sigmoid else logit */
int  uwm_stats(const float* logits, int ld, const void* target, int target_dtype, int N, long long hw,
               float threshold, int apply_sigmoid, long long* out, uwm_stream stream);
/* mask[npix] uint8 = (v > threshold) ? 255 : 0 */
int  uwm_threshold(const float* logits, int ld, long long npix, float threshold, int apply_sigmoid,
                   uint8_t* mask, uwm_stream stream);

/* torch.optim.Adam (coupled weight decay) over a flat range; step = 1-based step count */
int  uwm_adam(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
              float eps, float weight_decay, long long step, float grad_scale, uwm_stream stream);
/* same, preceded by global-norm gradient clipping (torch.nn.utils.clip_grad_norm_(params, max_norm)): the norm of
 * grad_scale*g over the whole range is reduced on the device (scratch: >= 8 bytes) and folded into the update */
int  uwm_adam_clip(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, long long step, float grad_scale, float max_norm, void* scratch,
                   uwm_stream stream);
/* The same update with every hyper-parameter in DEVICE memory, for a hipGraph-captured train step (one captured launch must
 * serve every step): hyper = 10 floats {lr, beta1, beta2, eps, weight_decay, grad_scale, max_norm, step, -, -}; the call
 * advances hyper[7] (the step count of the update it performs: write step - 1 there before the first call / after a restore)
 * and fills the two bias-correction slots itself.  clip_scratch != NULL (>= 8 bytes): global-norm clipping to hyper[6]. */
int  uwm_adam_graph(float* p, const float* g, float* m, float* v, long long n, float* hyper, void* clip_scratch,
                    uwm_stream stream);
/* torch.optim.AdamW (decoupled weight decay): the same arguments and hyper layout as uwm_adam / uwm_adam_clip /
 * uwm_adam_graph; p *= 1 - lr*weight_decay, then the Adam moments of the (scaled, clipped) gradient without an L2 term */
int  uwm_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
               float eps, float weight_decay, long long step, float grad_scale, uwm_stream stream);
int  uwm_adamw_clip(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, long long step, float grad_scale, float max_norm, void* scratch,
                    uwm_stream stream);
int  uwm_adamw_graph(float* p, const float* g, float* m, float* v, long long n, float* hyper, void* clip_scratch,
                     uwm_stream stream);
/* torch.optim.SGD(lr, momentum, weight_decay) (coupled L2, dampening 0; the reference's OPTIMIZER.NAME == "SGD" branch,
 * /root/reference/src/train.py:272-278) over a flat range: buf = step == 1 ? g' : momentum*buf + g', p -= lr*buf with
 * g' = grad_scale*g + weight_decay*p; max_norm > 0 adds global-norm clipping as uwm_adam_clip (scratch >= 8 bytes). */
int  uwm_sgd(float* p, const float* g, float* buf, long long n, float lr, float momentum, float weight_decay,
             long long step, float grad_scale, float max_norm, void* scratch, uwm_stream stream);
int  uwm_scale(float* p, long long n, float s, uwm_stream stream);
/* Staged backward under data parallelism: uwm_backward runs its weight-gradient kernels on an internal side stream and,
 * by default, makes the caller's stream wait for them before it returns.  With a join stream set (the stream the
 * gradient all-reduces are issued on), the stages before the last make THAT stream wait instead, so the caller's
 * stream continues into the next stage while the side stream drains; the last stage joins both.  NULL restores the
 * default. */
int  uwm_set_join_stream(uwm_handle h, uwm_stream stream);
/* The data-parallel exchange itself (nothing comparable exists in the reference, which has no DDP):
 * SUM all-reduce, in place, of the gradient-arena ranges of backward stages [stage_begin, stage_end) over the RCCL
 * communicator `nccl_comm` (an ncclComm_t), one ncclAllReduce per stage, enqueued on `stream` (the communication
 * stream — order it behind uwm_backward of those stages with an event, or hand it to uwm_set_join_stream).  Averaging
 * is the optimizer's grad_scale = 1/world.  RCCL is not linked: ncclAllReduce is looked up in the host process (the
 * library that created the communicator), else librccl.so.1 is opened. */
int  uwm_allreduce_grads(uwm_handle h, void* nccl_comm, int stage_begin, int stage_end, uwm_stream stream);
float* uwm_grad_arena(uwm_handle h);     /* the bound gradient arena (NULL before uwm_bind) */
/* Input pipeline on the device (src/utils/dataset.py:298-395 get_*_transform tails): uint8 HWC images [N][H][W][C] ->
 * Normalize(mean, std) of x/255 as NCHW fp32 (what uwm_forward takes); uint8 masks [N][H][W] -> (m > threshold) as
 * uint8 {0,1} (what uwm_loss takes).  flags (device int[N] or NULL): bit0 HorizontalFlip, bit1 VerticalFlip, bits 2-3
 * k of RandomRotate90 (counter-clockwise, needs H == W), applied flips first, then the rotation — the same flags on
 * image and mask keep them aligned.  mean/std are host pointers (C values). */
int  uwm_preprocess_u8(const uint8_t* images, int N, int H, int W, int C, const float* mean, const float* std,
                       const int* flags, float* out_nchw, uwm_stream stream);
int  uwm_preprocess_mask_u8(const uint8_t* masks, int N, int H, int W, int threshold, const int* flags, uint8_t* out,
                            uwm_stream stream);
/* Train-time augmentation on the device: the reference's basic recipe (get_train_transform, src/utils/dataset.py:375-387) behind
 * the resize, in one launch for the images and one for the masks, on the caller's stream, without host synchronisation;
 * capturable like uwm_preprocess_u8.  images uint8 [N][H][W][C], C in 1..4; masks uint8 [N][H][W] (NULL together with out_masks:
 * no masks); descs: one uwm_aug_desc per image in DEVICE memory (8-byte aligned).  out_nchw: fp32 [N][C][H][W] normalised;
 * out_masks: uint8 {0,1}; out_u8 (may be NULL): the augmented uint8 image [N][H][W][C] before Normalize, for tests and for
 * looking at what the augmenter makes.  mean / std are host pointers (C values).
 *   Stage order per output pixel: flips -> rot90 -> affine warp -> table -> HSV -> Normalize.  The warp is an inverse-map gather,
 * so output (x, y) goes to fixed-point coordinates in the flipped and rotated image, four taps are taken there, each
 * border-reflected, and each goes through the flags' index map of uwm_preprocess_u8 into the input.
 *   The rule, in integers so that it can be checked bit for bit (a restatement of OpenCV 4.x's 8-bit warpAffine with
 * WARP_INVERSE_MAP semantics, AB_BITS = 10, INTER_BITS = 5, BORDER_REFLECT_101 — written from knowledge of the source, NOT run
 * against cv2).  rne = round half to even to int; float64 arithmetic with every product and sum rounded on its own (no fused
 * multiply-add):
 *     adelta[x] = rne(minv0*x*1024)               bdelta[x] = rne(minv3*x*1024)
 *     X0[y] = rne((minv1*y + minv2)*1024) + r      Y0[y] = rne((minv4*y + minv5)*1024) + r
 *   image (linear), r = 16:  X = (X0[y] + adelta[x]) >> 5, Y likewise; sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
 *     out = ((32-fx)(32-fy)*p00 + fx(32-fy)*p01 + (32-fx)fy*p10 + fx*fy*p11 + 512) >> 10    p_ij = tap (sy + i, sx + j)
 *   mask (nearest), r = 512: sx = (X0[y] + adelta[x]) >> 10, sy likewise; then (m > mask_threshold) -> {0,1}.
 *   border: reflect-101 of ANY coordinate (period 2(n-1), as many reflections as it takes; n = 1 -> 0).
 *   table: v = lut[v] on every channel (brightness / contrast; computed by the host, so no device float rule is involved).
 *   HSV, only when C == 3 and some shift != 0.  Forward = OpenCV's 8-bit RGB -> HSV with H in 0..179:
 *     v = max, d = max - min, s = (d*sdiv[v] + 2048) >> 12, h0 = (v == r) ? g-b : (v == g) ? b-r+2d : r-g+4d,
 *     h = (h0*hdiv[d] + 2048) >> 12 (+180 if negative); sdiv[i] = rne((255<<12)/i), hdiv[i] = rne((180<<12)/(6i)), both 0 at i = 0
 *     shifts: h = (h + hue) mod 180 (non-negative), s = clip(s + sat, 0, 255), v = clip(v + val, 0, 255)
 *   The way back is THIS PROJECT'S OWN integer rule (OpenCV's goes through float32 and is not bit-stable across its own builds):
 *     sec = h/30, f = h%30, p = (v(255-s) + 127)/255, q = (v(7650 - s*f) + 3825)/7650, t = (v(7650 - s(30-f)) + 3825)/7650,
 *     (r,g,b) = (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q) for sec = 0..5
 *   Normalize: the expression of uwm_preprocess_u8, so out_nchw = uwm_preprocess_u8(out_u8, flags = NULL) bit for bit.
 *   The kernels only clamp: coordinates are clamped to +-(2^30 - 2048) fixed-point units, rot90 flags are ignored where H != W and
 *   HSV shifts where C != 3.  A host wrapper should refuse such descriptors, and matrices with non-finite entries, before the call. */
typedef struct {
  int flags;              /* as uwm_preprocess_u8: bit0 hflip, bit1 vflip, bits 2-3 rot90 k (needs H == W) */
  int hue, sat, val;      /* HueSaturationValue shifts; all three 0 = stage skipped */
  double minv[6];         /* INVERSE affine map, dst (x,y) -> src: sx = minv0*x + minv1*y + minv2, sy = minv3*x + minv4*y + minv5 */
  unsigned char lut[256]; /* per-value table applied to every channel after the warp */
} uwm_aug_desc;           /* 320 bytes */
int  uwm_augment_u8(const uint8_t* images, const uint8_t* masks, const uwm_aug_desc* descs, int N, int H, int W, int C,
                    const float* mean, const float* std, int mask_threshold, float* out_nchw, uint8_t* out_masks, uint8_t* out_u8,
                    uwm_stream stream);
/* The stages that the reference's enhanced recipe (get_enhanced_train_transform, src/utils/dataset.py:336-373) adds behind the basic
 * ones: per image, on the uint8 image that uwm_augment_u8 forms (flips -> rot90 -> warp -> table -> HSV),
 *     tone -> noise -> blur -> Normalize
 * from a SECOND descriptor array, one uwm_aug_ext_desc per image in DEVICE memory (8-byte aligned).  ext == NULL is uwm_augment_u8
 * bit for bit (workspace is then not used).  The mask does not see these stages: out_masks is uwm_augment_u8's.  Arguments and
 * checks as uwm_augment_u8, plus workspace: device memory, 16-byte aligned, at least uwm_augment_ext_workspace_bytes(N, H, W, C)
 * bytes (a uint8 stage image [N][H][W][C] and the CLAHE tile tables [N][64][256]).  No host synchronisation and every launch is
 * sized from N, H, W alone, so a captured graph serves every batch of a shape — except that the FIRST call on a device copies the
 * library's tables there synchronously and is refused inside a stream capture: call once before capturing.
 *   After the host's parameter and table setup everything is integer work, or float32 with every product, sum and difference rounded
 * on its own (no fused multiply-add), so the result can be checked bit for bit (tests/augment_ext_ref.py is the numpy form).
 * rne = round half to even; reflect-101 as above.
 *   tone = 2 (RandomGamma): v = lut2[v] on every channel; the host builds the table, trunc(((i/255.0)**gamma)*255).
 *   tone = 1 (CLAHE, 8 x 8 tiles; OpenCV 4.x's algorithm, written from knowledge of the source, NOT run against cv2).  C = 1: on the
 * plane; C = 3: on the lightness plane L8 below; skipped where C is 2 or 4 or H < 8 or W < 8.  The plane is extended at the bottom
 * and the right by reflect-101 to multiples of 8; tileH = Hp/8, tileW = Wp/8, area = tileH*tileW.  Per tile: 256-bin histogram over
 * the padded tile; with clip = max(clahe_clip, 1): excess = sum max(h - clip, 0), h = min(h, clip) + excess/256, and the residual
 * excess%256 goes one to a bin at bins 0, step, 2 step, ... (step = max(256/residual, 1)) until spent;
 * lut[i] = saturate(rne(float(cumsum[i]) * (255.0f/area))).  Per pixel: tyf = float(y) * (1.0f/tileH) - 0.5f, ty1 = floor(tyf),
 * ya = tyf - ty1, ty1 and ty1 + 1 clamped to 0..7, x likewise;
 * res = (lut11[v]*(1-xa) + lut12[v]*xa)*(1-ya) + (lut21[v]*(1-xa) + lut22[v]*xa)*ya, then saturate(rne(res)).  The host passes
 * clahe_clip = max(1, int(clipLimit * area / 256)) (data.clahe_clip_limit).
 *   Lightness (C = 3) is THIS PROJECT'S OWN integer rule (OpenCV's 8-bit Lab code is not restated).  With the tables of
 * uwm_aug_lab_tables — LIN[256] = rne(16384 * srgb_to_linear(v/255)); F[i] = rne(32768 * f(i/16384)), f(t) = cbrt(t) above
 * 0.008856, else 7.787 t + 16/116; FINV[j] = rne(16384 * f^-1(j/8192)) (f^3 above 0.206893, else (f - 16/116)/7.787, not below 0);
 * GAM[i] = rne(255 * linear_to_srgb(i/16384)) — and OpenCV's D65 matrix over the white point in 12 fraction bits:
 *     X = (1777 r + 1541 g + 778 b + 2048) >> 12, Y = (871 r + 2929 g + 296 b + 2048) >> 12, Z = (73 r + 448 g + 3575 b + 2048) >> 12
 *     (r, g, b = LIN of the bytes; every row sums to 4096, so a grey has X = Y = Z), fx = F[X], fy = F[Y], fz = F[Z],
 *     L8 = clip((2 * (116 fy - 524288) * 255 + 3276800) / 6553600)                          = round(L * 255 / 100)
 *   back, with the new L8: fy' = (65536 * (100 L8 + 4080) + 29580) / 59160, fx' = fy' + (fx - fy), fz' = fy' - (fy - fz),
 *     t = FINV[(clip(f', 0, 65535) + 2) >> 2], linear = clip((row . t + 2048) >> 12, 0, 16384) with the rows
 *     (12615, -6296, -2223), (-3773, 7684, 185), (217, -836, 4715), byte = GAM[linear].
 *   noise (GaussNoise; numpy's generator is not reproduced, only the distribution): noise_sigma = sigma * 256 (0 = off, clamped to
 * 16383), per byte counter = (y*W + x)*4 + c, z = seed + (counter + 1) * 0x9E3779B97F4A7C15, then splitmix64's finaliser
 * (z ^= z >> 30, *= 0xBF58476D1CE4E5B9, z ^= z >> 27, *= 0x94D049BB133111EB, z ^= z >> 31); r = z >> 40, k = r >> 14, fr = r & 16383,
 * normal = (QN[k] * (16384 - fr) + QN[k+1] * fr) >> 12 with QN[i] = rne(4096 * Phi^-1(i/1024)) and the two ends at
 * Phi^-1(1/4096) = -+3.4871, where the tails stop (the table's distribution has variance 0.99908);
 * out = clip(v + ((normal * noise_sigma) >> 22), 0, 255) = clip(floor(v + g)).
 *   blur, 3 x 3 correlation over the pre-blur values (tone and noise of the neighbours, reflect-101): blur = 2 (Gaussian, sigma 0):
 * weights [1 2 1] x [1 2 1], out = (sum + 8) >> 4; blur = 1 (motion): weights blur_w[3*i + j] != 0 for the tap (y + i - 1, x + j - 1),
 * out = sum / count rounded half to even; no tap set = no blur.  The host rasterises a line between two distinct points of the 3 x 3
 * grid: both end points and, between end points two apart, the middle, a half rounded up (the project's rasterisation).
 *   The kernels only clamp: unknown tone / blur values are "none", clahe_clip < 1 is 1, noise_sigma is clamped. */
typedef struct {
  int tone;                  /* 0 none, 1 CLAHE, 2 table lut2 */
  int clahe_clip;            /* CLAHE's integer clip limit per bin, >= 1 */
  int noise_sigma;           /* GaussNoise sigma * 256; 0 = off */
  int blur;                  /* 0 none, 1 motion (blur_w), 2 Gaussian */
  unsigned char blur_w[9];   /* the motion kernel's 0/1 taps, row by row */
  unsigned long long seed;   /* of the noise (offset 32) */
  unsigned char lut2[256];   /* tone = 2: per-value table (offset 40) */
} uwm_aug_ext_desc;          /* 296 bytes */
size_t uwm_augment_ext_workspace_bytes(int N, int H, int W, int C);      /* 0 (and an error message) for a bad shape */
int  uwm_augment_ext_u8(const uint8_t* images, const uint8_t* masks, const uwm_aug_desc* descs, const uwm_aug_ext_desc* ext, int N,
                        int H, int W, int C, const float* mean, const float* std, int mask_threshold, void* workspace,
                        size_t workspace_bytes, float* out_nchw, uint8_t* out_masks, uint8_t* out_u8, uwm_stream stream);
/* The host's tables of the rule above, built at first use: which = 0 LIN (int), 1 F (unsigned short), 2 FINV (int), 3 GAM
 * (unsigned char), 4 QN (int). */
int  uwm_aug_lab_tables(int which, const void** data, int* count, int* elem_bytes);
/* A.ImageCompression of the reference's transparent_watermark recipe (get_transparent_watermark_transform, src/utils/dataset.py:298-334)
 * in front of Normalize: what a baseline JPEG encode + decode at quality q does to the pixels.  Huffman coding is lossless, so this is
 * libjpeg's default path without it (what cv2.imencode / imdecode and Pillow run, through libjpeg-turbo): 4:2:0 sampling, the "islow"
 * integer DCT, "fancy" up-sampling.  images uint8 [N][H][W][3] RGB, H % 16 == 0 and W % 16 == 0; quality: DEVICE int[N] (4-byte aligned),
 * 0 = the image passes through unchanged (and is still normalised), else 1..100 (the kernels clamp to 0..100; a host wrapper should
 * refuse other values).  out_nchw (fp32 [N][3][H][W], 16-byte aligned) and out_u8 ([N][H][W][3], 4-byte aligned like images): either
 * may be NULL, not both;
 * out_nchw = uwm_preprocess_u8(out_u8, flags = NULL) bit for bit.  workspace: device memory, 16-byte aligned, at least
 * uwm_jpeg_workspace_bytes(N, H, W) bytes (the reconstructed Y plane [N][H][W] and Cb, Cr planes [N][H/2][W/2]).  mean / std are host
 * pointers (3 values).  Two launches on the caller's stream, sized from N, H, W alone, no host synchronisation: capturable.
 *   The rule (tests/jpeg_ref.py is the numpy form, held to Pillow bit for bit).  All arithmetic is signed 32-bit integer, >> is an
 * arithmetic shift, D(x, n) = (x + (1 << (n-1))) >> n.
 *   tables: T = Annex K luminance (for Y) and chrominance (for Cb, Cr), natural order; s = 5000 / q for q < 50, else 200 - 2q;
 *     Q[i] = clamp((T[i]*s + 50) / 100, 1, 255).
 *   RGB -> YCbCr: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128<<16) + 32767) >> 16,
 *     Cr = (32768 R - 27439 G - 5329 B + (128<<16) + 32767) >> 16.
 *   chroma down-sampling 2 x 2: (sum of the four + bias) >> 2, bias 1 in even output columns and 2 in odd ones.
 *   forward DCT of every 8 x 8 block of (sample - 128), libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2), rows first, then columns.
 *     1-D pass on d0..d7: t0 = d0+d7, t7 = d0-d7, t1 = d1+d6, t6 = d1-d6, t2 = d2+d5, t5 = d2-d5, t3 = d3+d4, t4 = d3-d4;
 *     t10 = t0+t3, t13 = t0-t3, t11 = t1+t2, t12 = t1-t2; rows: out0, out4 = (t10 +- t11) << 2; columns: D(t10 +- t11, 2);
 *     z1 = (t12+t13)*4433, out2 = D(z1 + t13*6270, n), out6 = D(z1 - t12*15137, n)          n = 11 for rows, 15 for columns
 *     z1 = t4+t7, z2 = t5+t6, z3 = t4+t6, z4 = t5+t7, z5 = (z3+z4)*9633; t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
 *     z1 *= -7373, z2 *= -20995, z3 = z3*-16069 + z5, z4 = z4*-3196 + z5;
 *     out7 = D(t4+z1+z3, n), out5 = D(t5+z2+z4, n), out3 = D(t6+z2+z3, n), out1 = D(t7+z1+z4, n).       (8 times the DCT)
 *   quantise: qv = Q[i] << 3, a = (|c| + (qv >> 1)) / qv, coefficient = a with the sign of c; dequantised value = coefficient * Q[i].
 *   inverse DCT, libjpeg's jidctint, columns first with n = 11, then rows with n = 18.  1-D pass: z1 = (d2+d6)*4433,
 *     t2 = z1 - d6*15137, t3 = z1 + d2*6270, t0 = (d0+d4) << 13, t1 = (d0-d4) << 13, t10 = t0+t3, t13 = t0-t3, t11 = t1+t2, t12 = t1-t2;
 *     (t0, t1, t2, t3) = (d7, d5, d3, d1); z1 = t0+t3, z2 = t1+t2, z3 = t0+t2, z4 = t1+t3, z5 = (z3+z4)*9633; t0 *= 2446, t1 *= 16819,
 *     t2 *= 25172, t3 *= 12299; z1 *= -7373, z2 *= -20995, z3 = z3*-16069 + z5, z4 = z4*-3196 + z5; t0 += z1+z3, t1 += z2+z4,
 *     t2 += z2+z3, t3 += z1+z4; out0, out7 = D(t10 +- t3, n), out1, out6 = D(t11 +- t2, n), out2, out5 = D(t12 +- t1, n),
 *     out3, out4 = D(t13 +- t0, n).  Then + 128 and clamp to 0..255.
 *   chroma up-sampling, h2v2 "fancy": for output row 2r + v, s[x] = 3*c[r][x] + c[r'][x], r' = r-1 (v = 0) or r+1 (v = 1);
 *     out[2x] = (3 s[x] + s[x-1] + 8) >> 4, out[2x+1] = (3 s[x] + s[x+1] + 7) >> 4; r', x-1 and x+1 clamped to the plane.
 *   YCbCr -> RGB with cb, cr minus 128: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 *     G = Y + ((-22554 cb - 46802 cr + 32768) >> 16); clamp to 0..255. */
size_t uwm_jpeg_workspace_bytes(int N, int H, int W);      /* 0 (and an error message) for a bad shape */
int  uwm_jpeg_u8(const uint8_t* images, const int* quality, int N, int H, int W, const float* mean, const float* std, void* workspace,
                 size_t workspace_bytes, float* out_nchw, uint8_t* out_u8, uwm_stream stream);
/* The JPEG save of the reference's gen_data.py (quality 95: the final save, gen_data.py:908, and the temporary file between the logos
 * and the text of a mixed sample, gen_data.py:402-410): uwm_jpeg_u8's round trip for a RAGGED batch, every image at its own size, any
 * h and w >= 1.  in / out: packed uint8 RGB images of `bytes` bytes (4-byte aligned) with one uwm_image_desc each (DEVICE memory,
 * 8-byte aligned); out may be in itself, and must not overlap it otherwise.  quality: DEVICE int[N] (4-byte aligned), 0 = the image is
 * left as it is, else 1..100 (the kernels clamp to 0..100; a host wrapper should refuse other values).  C must be 3.  max_pixels: an
 * upper bound of h*w over the batch, below 2^31 - 1; it sizes the launches.  workspace: device memory, 8-byte aligned, at least
 * uwm_jpeg_ragged_workspace_bytes(N, bytes) = bytes bytes, apart from in and out: image i's reconstructed planes (Y [h][w], Cb and Cr
 * [hc][wc], hc = ceil(h/2), wc = ceil(w/2)) lie back to back at the image's own offset, h*w + 2*hc*wc <= 3*h*w.  Two launches of
 * N * K workgroups on the caller's stream, K from max_pixels alone, geometry read on the device, no host synchronisation: one captured
 * graph serves every batch of N images with these `bytes` and `max_pixels`.  An image whose descriptor does not fit (a side < 1, more than
 * max_pixels pixels, not inside `bytes`) is skipped: nothing of it is read or written.  No read leaves [in, in+bytes), no write
 * [out, out+bytes) or the workspace.
 *   The rule is uwm_jpeg_u8's (tables, colour conversion, DCTs, quantisation) with libjpeg's edges (tests/jpeg_any_ref.py is the numpy
 * form, held to Pillow bit for bit); c8(x) = x rounded up to a multiple of 8:
 *   Y: the last column and the last row are replicated out to c8(h) x c8(w); its 8 x 8 blocks go through the luminance table; crop.
 *   Cb, Cr: COLUMNS are replicated at full resolution, in front of the down-sampling, and so is an odd last row; ROWS are replicated
 *     behind it.  Down-sampled sample (r, c) of the c8(hc) x c8(wc) plane is the 2 x 2 mean (bias 1 in even c, 2 in odd c) of image
 *     rows 2r' and min(2r'+1, h-1), r' = min(r, hc-1), and columns min(2c, w-1) and min(2c+1, w-1).  Its blocks go through the
 *     chrominance table; crop to hc x wc.
 *   up-sampling: wc > 2: the "fancy" filter above on the cropped hc x wc plane, neighbours clamped to it, cropped to h x w;
 *     wc <= 2: libjpeg falls back to replication, every chroma sample fills its 2 x 2 pixels. */
size_t uwm_jpeg_ragged_workspace_bytes(int N, size_t bytes);      /* 0 (and an error message) for arguments out of range */
int  uwm_jpeg_ragged_u8(const uint8_t* in, uint8_t* out /* may be in */, size_t bytes, const uwm_image_desc* descs /* device */,
                        const int* quality /* device int[N] */, int N, int C /* 3 */, long long max_pixels, void* workspace,
                        size_t workspace_bytes, uwm_stream stream);
/* 3x3/stride-1 convolutions (forward, dgrad and weight gradient) run as Winograd F(2x2,3x3) on the fp32 MFMA path by
 * default (2.25x fewer multiplies, results within a few fp32 ulps of the direct form); mode 0 selects the direct
 * kernels everywhere; 2 (tests) prefers the 512-thread Winograd variant wherever its shape rules allow, whatever the
 * launch size.  uwm_set_winograd_mode is PER HANDLE.  uwm_set_winograd sets the process default, which the
 * single-operator entry points (uwm_op_*) use and which a handle takes at uwm_create (also UWM_WINOGRAD=0 in the
 * environment); it does not change existing handles. */
int  uwm_set_winograd(int on);
int  uwm_set_winograd_mode(uwm_handle h, int mode);
int  uwm_get_winograd_mode(uwm_handle h);
/* Precision mode, per handle.  UWM_PREC_F32 (default): every product on the exact-fp32 matrix instruction.
 * "bf16x3" arithmetic takes a product as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi over bf16 halves (hi = bf16(x), lo = bf16(x - hi))
 * of the fp32 operands with fp32 accumulation: ~17 mantissa bits per operand on 3 bf16 matrix instructions at 16x the fp32
 * rate (conv_wino_x3.hip).  Parameters, activations, accumulators, BatchNorm, loss, weight gradients and optimizer state
 * stay fp32 in every mode.
 *   UWM_PREC_BF16X3      the BACKWARD data-gradient (dgrad) products of the 3x3 stride-1 layers with whole 16-channel
 *                        chunks.  The forward is untouched, so logits are the fp32 mode's bit for bit and the 1e-3 bar
 *                        against the fp32 CPU reference holds at every depth; gradients meet the fp32 mode's bars.
 *   UWM_PREC_BF16X3_ALL  forward products of those layers as well.  Measured logit error vs the fp32 CPU reference:
 *                        < 1e-3 on resnet18 / efficientnet-b4, 1.6e-3 on resnet34 (2x256x192) — outside BASELINE's bar on
 *                        the deeper encoders, offered for what the reference itself does on a GPU: reduced-precision
 *                        training (fp16 autocast + GradScaler, /root/reference/src/train.py:75,89-98).
 * "fp16x3" arithmetic (conv_f16x3.hip) is the same three-term product over FP16 halves (hi = fp16(x), lo = fp16(x - hi): 22
 * mantissa bits per operand, relative error 2^-22 per product against 2^-24 for fp32) on gfx950's
 * v_mfma_f32_16x16x32_f16, direct-form convolution, fp32 accumulation; fp16's exponent range is covered by exact
 * power-of-two scaling of every filter row (and of a dgrad's dY).  fp32-class accuracy: it meets the fp32 mode's bars.
 *   UWM_PREC_F16X3       the FORWARD products of the 3x3 stride-1 layers with channels % 32 == 0
 *   UWM_PREC_F16X3_ALL   their data-gradient and weight-gradient products as well
 * Two REDUCED-precision modes on the same kernels (never the default, never bench.py's headline; reported under alt_modes):
 *   UWM_PREC_F16X1       one product per tile, hi * hi' — plain fp16 products with fp32 accumulation, fp32 storage, BatchNorm and
 *                        optimizer: the arithmetic of the reference's own GPU path (torch.autocast fp16 + GradScaler,
 *                        /root/reference/src/train.py:75,89-98) with the exact power-of-two range scaling in place of a loss
 *                        scaler.  Forward, dgrad and wgrad.  Logits differ from the fp32 CPU reference by 2e-2 (resnet18) to
 *                        7e-2 (resnet34; tests/test_model_gpu.py, bench.py alt_modes): OUTSIDE BASELINE's 1e-3 bar.
 *   UWM_PREC_F16X3_BWD2  forward as UWM_PREC_F16X3_ALL (logits identical, inside the bar); in the backward the gradient operand dY
 *                        enters as ONE fp16 (two products per tile: dy_hi * w_hi + dy_hi * w_lo), i.e. gradients carry 11-bit dY
 *                        against 22-bit weights / activations — still above the reference's GPU arithmetic. */
int  uwm_set_precision(uwm_handle h, int mode);
int  uwm_get_precision(uwm_handle h);
/* The fp16x3 forward / dgrad kernels work in 16x16-pixel x 64-channel workgroups and are taken for launches of at least
 * `min_workgroups` of them (0 = the default: one per two compute units — measured: layer4 at batch 16, 128 workgroups on 256 CUs,
 * is still 2 % of the step faster there than on the fp32 Winograd kernels; smaller launches stay on those, which tile finer).  1 = wherever the shape allows (tests). */
int  uwm_set_precision_fill(uwm_handle h, int min_workgroups);
/* Routing batch: with batch > 0 every size-dependent kernel choice (fp16x3 fill rule, 4- / 8-wave and tile-width variants, tile
 * configurations of the implicit GEMM) is made as if the batch were `batch` images, whatever N uwm_forward gets; grids and split
 * counts follow the real N.  A 2-image parity sample then runs on exactly the kernels the 16-image step takes (bench.py, tests).
 * 0 (default) = the real batch. */
int  uwm_set_routing_batch(uwm_handle h, int batch);
/* Routing record: while enabled, every convolution-class launch of uwm_forward / uwm_backward appends one line
 * "<fwd|dgrad|wgrad> <layer name> <kernel>" (launch order) to a per-handle text.  uwm_routing_dump copies it (NUL-terminated, at
 * most cap bytes) and returns the size the whole text needs including the NUL; clear != 0 empties it afterwards.  Host-side
 * bookkeeping only: no device work, no effect on results. */
int  uwm_routing_enable(uwm_handle h, int on);
long long uwm_routing_dump(uwm_handle h, char* buf, long long cap, int clear);
/* EfficientNet encoders only: stochastic depth ("drop connect") of the MBConv blocks in training mode.  `rowscale` is a
 * device array [uwm_num_mbconv_blocks][N] holding, per block and sample, keep/(1 - p_block) with keep in {0,1}; the host
 * draws it each step (uwm_mbconv_drop_rate gives p_block; blocks without identity skip ignore their row).  NULL (the
 * default) disables it.  The pointer is read by the next uwm_forward(training=1) and its uwm_backward. */
int  uwm_set_drop_connect(uwm_handle h, const float* rowscale);
/* Single-operator entry point of the depthwise k x k convolution (k 3|5, stride 1|2; tests and kernel timing).  NHWC
 * activations, weights tap-major [k*k][C]; pad_begin = zero pad at the top/left (efficientnet_pytorch's static "same"
 * padding: the bottom/right pad follows from Ho, Wo).  mode 0: out[N][Ho][Wo][C] = conv(a = x[N][H][W][C], b = w);
 * mode 1: out[N][H][W][C] = dgrad(a = dy[N][Ho][Wo][C], b = w) (+ addend); mode 2: out[k*k][C] += wgrad(a = x, b = dy),
 * scratch = uwm_op_depthwise_scratch_floats(...) floats. */
int  uwm_op_depthwise(int mode, const float* a, const float* b, int k, int stride, int pad_begin, int N, int H, int W, int C,
                      int Ho, int Wo, const float* addend, float* out, float* scratch, uwm_stream stream);
long long uwm_op_depthwise_scratch_floats(int k, int N, int C, int Ho, int Wo);
/* Single-operator entry points of the rest of the MBConv block (tests and kernel timing).  Activations are NHWC
 * [N][hw][C] floats with C a multiple of 4 (>= 4), per-channel vectors [C], per-sample vectors [N][C]; N, hw, npix >= 1.
 * Every entry returns non-zero without launching on a NULL required pointer or a size outside these limits.
 * out[npix][C] = swish(y*scale + shift),  swish(z) = z * sigmoid(z) */
int  uwm_op_swish(const float* y, const float* scale, const float* shift, long long npix, int C, float* out, uwm_stream stream);
/* act_out = swish(y*scale + shift) and pool[N][C] = mean over hw of act_out, one pass; part: uwm_op_se_scratch_floats(N, C)
 * floats.  A sample's pool row does not depend on N, bit for bit. */
int  uwm_op_swish_pool(const float* y, const float* scale, const float* shift, int N, long long hw, int C, float* act_out,
                       float* pool, float* part, uwm_stream stream);
/* out[N][C] = mult * sum over hw of a (b == NULL) or of a*b; part as above; deterministic and independent of N */
int  uwm_op_se_reduce(const float* a, const float* b, int N, long long hw, int C, float mult, float* out, float* part,
                      uwm_stream stream);
long long uwm_op_se_scratch_floats(int N, int C);
/* Squeeze-and-excitation FC pair: hpre[N][nsq] = W1 pool + b1, hid = swish(hpre), s[N][C] = sigmoid(W2 hid + b2).
 * w1 [nsq][K1pad] (K1pad >= C), w2 [C][K2pad] (K2pad >= nsq rounded up to 4, a multiple of 4, w2 16-byte aligned): the
 * parameter arena's layout of the two 1x1 layers; pad columns are never read for their value. */
int  uwm_op_se_fc(const float* pool, const float* w1, const float* b1, int K1pad, const float* w2, const float* b2, int K2pad,
                  int N, int C, int nsq, float* hpre, float* hid, float* s, uwm_stream stream);
/* Backward of the pair: gs[N][C] (gradient wrt s) is overwritten with the gradient wrt W2 hid + b2; gpool[N][C], gw1
 * [nsq][K1pad], gb1 [nsq], gw2 [C][K2pad], gb2 [C] are plain stores that leave the pad columns alone; acc1: scratch
 * [N][nsq], zeroed here. */
int  uwm_op_se_fc_backward(float* gs, const float* s, const float* hpre, const float* pool, const float* w1, int K1pad,
                           const float* w2, int K2pad, int N, int C, int nsq, float* gpool, float* acc1, float* gw1, float* gb1,
                           float* gw2, float* gb2, uwm_stream stream);
/* out[n][hw][c] = a[n][hw][c] * s[n][c] */
int  uwm_op_se_scale(const float* a, const float* s, int N, long long hw, int C, float* out, uwm_stream stream);
/* block output: out = (y*scale + shift) * rowscale[n] + id; rowscale [N] (drop connect) and id may each be NULL */
int  uwm_op_mb_out(const float* y, const float* scale, const float* shift, const float* rowscale, const float* id, int N,
                   long long hw, int C, float* out, uwm_stream stream);
/* out[n][hw][c] = g[n][hw][c] * rowscale[n] */
int  uwm_op_rowscale(const float* g, const float* rowscale, int N, long long hw, int C, float* out, uwm_stream stream);
/* Training-mode BatchNorm statistics of y[npix][C] as a depthwise layer takes them: per-channel sum and sum of squares
 * into sums2c (2*C doubles, zeroed here), then mean, rstd = 1/sqrt(var + eps) (biased variance), scale = gamma*rstd,
 * shift = beta - mean*scale; with update_running != 0 also run = (1 - momentum)*run + momentum*{mean, unbiased variance}
 * (run_mean / run_var may be NULL otherwise and are left untouched). */
int  uwm_op_bn_stats(const float* y, long long npix, int C, const float* gamma, const float* beta, float eps, float momentum,
                     int update_running, float* run_mean, float* run_var, double* sums2c, float* mean, float* rstd,
                     float* scale, float* shift, uwm_stream stream);
int  uwm_num_mbconv_blocks(uwm_handle h);
float uwm_mbconv_drop_rate(uwm_handle h, int block);
/* predict.py:620-625 on the device: bilinear resize (cv2.INTER_LINEAR convention) of each image's logit plane
 * [N][h][w] (element stride ld) to [N][H][W], then (v > threshold) ? 255 : 0.  mask and/or resized may be NULL. */
int  uwm_resize_threshold(const float* logits, int ld, int N, int h, int w, int H, int W, float threshold,
                          int apply_sigmoid, uint8_t* mask, float* resized, uwm_stream stream);

/* Mask post-processing on the device: the reference's WatermarkPredictor._optimize_mask (src/predict.py:161-301), which every
 * mask passes before it is returned or written.  Masks are uint8 [N][H][W], any H, W >= 1 with H*W < 2^31 - 1, N <= 65535;
 * foreground = value > 127, results in {0, 255}.  Integer work only: results are exact and the same on every run.
 *   elements    cv2.getStructuringElement: RECT all ones; ELLIPSE (w,h) with r = h/2, c = w/2: row i (dy = i - r) has ones in
 *               columns [max(c - dx, 0), min(c + dx + 1, w)), dx = round_half_even(c * sqrt((r*r - dy*dy) / (r*r)))
 *   morphology  anchor (w/2, h/2), no reflection: dilate dst(y,x) = OR over element(i,j) != 0 of src(y+i-ay, x+j-ax), erode the
 *               same with AND; pixels outside the image are ignored (0 for dilate, 1 for erode); open(k,n) = erode n times then
 *               dilate n times, close(k,n) the other way round
 *   components  8-connected; a component's id is the linear index y*W + x of its first pixel in raster order; "largest" =
 *               greatest area, ties to the smallest id
 *   pipelines   WATERMARK: open E(3,3)x1, close E(7,7)x3, close E(11,11)x2, dilate E(9,9)x2; keep the largest component, or, when
 *               its area is below 500, every component with area > 200.  TEXT: open E(2,2)x1, close E(3,3)x2, close R(5,1)x1 OR
 *               close R(1,5)x1 (same input), dilate E(4,4)x1; keep area > 50.  MIXED: open E(2,2)x1, close E(5,5)x2, dilate
 *               E(6,6)x1; keep area > 100.  (The reference's trailing 3x3 blur + threshold is the identity on {0,255} images.)
 * Caller-owned buffers, work enqueued on the caller's stream, no host synchronisation: capturable behind uwm_predict_u8.  Every
 * argument is checked before any launch.  workspace: uwm_mask_workspace_bytes(N, H, W) bytes (0 on a bad shape), 16-byte aligned. */
enum { UWM_MASK_WATERMARK = 0, UWM_MASK_TEXT = 1, UWM_MASK_MIXED = 2 };
enum { UWM_MORPH_RECT = 0, UWM_MORPH_ELLIPSE = 2 };              /* cv2's values */
/* host only, no device: the element as kh*kw bytes of 0/1 (1 <= kw, kh <= 15) */
int    uwm_mask_element(int shape, int kw, int kh, uint8_t* out);
size_t uwm_mask_workspace_bytes(int N, int H, int W);
/* the whole pipeline; out may alias in.  summary (device, may be NULL): long long [N][4] =
 * {components found, area of the largest (0 if none), foreground pixels of the output, id of the largest or -1} */
int    uwm_optimize_mask(const uint8_t* in, uint8_t* out, int N, int H, int W, int mask_type, long long* summary,
                         void* workspace, size_t workspace_bytes, uwm_stream stream);
/* The same on a ragged batch in ONE call, whatever the sizes: image i is descs[i].h x descs[i].w, one byte per pixel, at
 * in + descs[i].offset (any alignment: the layout uwm_resize_threshold_ragged writes); its result goes to out + descs[i].offset and
 * equals uwm_optimize_mask on that image alone bit for bit (ids are image-local, y * w_i + x).  out may be in.  UWM_MASK_NONE (this
 * call only): binarise (> 127), no morphology, keep every component.  stats (device, may be NULL): long long [N][8] =
 *   0 components found, 1 largest area, 2 foreground pixels of the output, 3 id of the largest or -1   (the summary above)
 *   4 components kept, 5 largest kept area       (the output is a union of whole components, so these ARE its components: what
 *                                                 cv2.connectedComponentsWithStats on the output counts; NONE: = entries 0, 1)
 *   6 h_i * w_i, 7 status: 0 done, 1 misfit
 * The descriptors are read on the device; the host arguments are capacities, so one captured call serves every batch of N images
 * that fits them: max_pixels (1 .. 2^31 - 2) bounds h_i * w_i and sizes the grids, rows bounds the sum of h_i and, with mask_bytes,
 * sizes the bit planes (image i takes h_i * ceil(w_i / 64) words; a plane holds mask_bytes / 64 + rows).  The launch count does
 * not depend on N (N <= 65535).  Misfit: a side outside 1 .. 2^30, h_i * w_i > max_pixels, a region that leaves [0, mask_bytes),
 * or, counting the images before it that pass those three tests, a sum of rows above `rows` or of plane words above the plane.  A
 * misfit gets status 1 and entries 0..6 zero, its bytes are not written and it costs the others nothing.  Whatever the
 * descriptors hold, no read leaves in / descs and no write leaves out + [0, mask_bytes), stats or the workspace; overlapping regions
 * are the caller's error.  workspace: uwm_mask_ragged_workspace_bytes(N, mask_bytes, rows) bytes (0 and a message on a bad
 * argument), descs / stats / workspace 8-byte aligned.  Every argument is checked before any launch; no host synchronisation,
 * allocation or copy. */
enum { UWM_MASK_NONE = 3 };
size_t uwm_mask_ragged_workspace_bytes(int N, size_t mask_bytes, long long rows);
int    uwm_optimize_masks_ragged(const uint8_t* in, uint8_t* out /* may alias in */, size_t mask_bytes,
                                 const uwm_image_desc* descs /* device */, int N, int mask_type, long long max_pixels,
                                 long long rows, long long* stats /* device [N][8], may be NULL */, void* workspace,
                                 size_t workspace_bytes, uwm_stream stream);
/* Scoring predicted masks against ground truth (mask_score.hip): a ragged batch of mask PAIRS in ONE call.  pred and
 * truth are two buffers of mask_bytes bytes under the same descriptors: image i is descs[i].h x descs[i].w, one byte per pixel, at
 * + descs[i].offset in both (any alignment: the layout uwm_resize_threshold_ragged writes).  Both are binarised as > 127, so raw
 * grey truth bytes go in as they are; pred may be truth.  With P, G the two binary masks of image i and d = radius[i]:
 *   E_d(M)[y][x] = 1 iff the whole (2d+1) x (2d+1) window centred on (y, x) lies inside the image and is set (the 3 x 3 square
 *                  erosion iterated d times, everything outside the image unset: Boundary IoU's mask_to_boundary)
 *   B_d(M)       = M & ~E_d(M)
 *   counts[i]    = long long [8]: 0 tp |P & G|, 1 fp |P & ~G|, 2 fn |~P & G|, 3 tn |~P & ~G|, 4 |B_d(P) & B_d(G)|, 5 |B_d(P)|,
 *                  6 |B_d(G)|, 7 status: 0 done, 1 misfit
 * d = 0 skips the boundary part (entries 4..6 are 0); 2d + 1 above a side makes E_d empty, so B_d(M) = M.  The cost does not depend
 * on d beyond the log2(2d + 1) doubling steps of the row erosion.  Counts are integers summed with integer atomics: the same on
 * every run.  The descriptors and radii are read on the device; the host arguments are capacities, so one captured call serves every
 * batch of N pairs that fits them: max_pixels (1 .. 2^31 - 2) bounds h_i * w_i and sizes the grids, rows bounds the sum of h_i and,
 * with mask_bytes, sizes the bit planes (image i takes h_i * ceil(w_i / 64) words; a plane holds mask_bytes / 64 + rows).  Five
 * launches whatever N (N <= 65535) and the radii are.  Misfit: a side outside 1 .. 2^30, h_i * w_i > max_pixels, a region that
 * leaves [0, mask_bytes), d outside 0 .. 32767, or, counting the images before it that pass those four tests, a sum of rows above
 * `rows` or of plane words above the plane.  A misfit gets status 1 and entries 0..6 zero, and it costs the others nothing.
 * Whatever the descriptors and radii hold, no read leaves pred / truth / descs / radius and no write leaves counts or the
 * workspace.  workspace: uwm_score_masks_workspace_bytes(N, mask_bytes, rows) bytes (0 and a message on a bad argument); descs /
 * counts / workspace 8-byte aligned, radius 4-byte aligned.  Every argument is checked before any launch; no host
 * synchronisation, allocation or copy. */
size_t uwm_score_masks_workspace_bytes(int N, size_t mask_bytes, long long rows);
int    uwm_score_masks_ragged(const uint8_t* pred, const uint8_t* truth, size_t mask_bytes,
                              const uwm_image_desc* descs /* device */, const int* radius /* device [N] */, int N,
                              long long max_pixels, long long rows, long long* counts /* device [N][8] */,
                              void* workspace, size_t workspace_bytes, uwm_stream stream);
/* Exact Euclidean distance transforms and surface distances (mask_dist.hip).  Masks are one byte per pixel, binarised
 * as > 127, under the descriptors of uwm_score_masks_ragged: image i is descs[i].h x descs[i].w at + descs[i].offset (any alignment).
 * Everything outside an image is unset.
 *   D2(M)[y][x]  = the minimum of (y - y')^2 + (x - x')^2 over the set pixels (y', x') of M: int32, 0 on set pixels, UWM_EDT_NONE
 *                  everywhere when M has no set pixel.  Sides are 1 .. 32768, so every real value is below UWM_EDT_NONE.
 *   dM           = M & ~erode(M), erode over the 4-neighbour cross: a set pixel with an unset 4-neighbour or on the image edge
 *                  (scipy's binary_erosion(M, generate_binary_structure(2, 1), border_value=0): MedPy's hd, hd95, assd).
 * uwm_edt_ragged writes D2 of image i's pixel k to d2[descs[i].offset + k]; d2 holds mask_bytes int32.  A misfit's entries are not
 * written.  Three launches.
 * uwm_surface_distances_ragged, with P = pred and G = truth of pair i (pred may alias truth):
 *   a = D2(dG) read at the pixels of dP, b = D2(dP) read at the pixels of dG, v = a and b together, sorted, n = |v|
 *   (lo, rem) = divmod(95 * (n - 1), 100), hi = lo + (rem > 0)
 *   records[i] = long long [10]: 0 border_pred |dP|, 1 border_truth |dG|, 2 hd_d2_pred max a, 3 hd_d2_truth max b, 4 p95_d2_lo v[lo],
 *                5 p95_d2_hi v[hi], 6 p95_rem rem, 7 cover_d2, 8 defined, 9 status: 0 done, 1 misfit
 *   cover_d2   = the maximum over the set pixels of G of D2(P): the squared radius of the smallest Euclidean disc dilation of P that
 *                covers G; 0 when G is empty, -1 when P is empty and G is not
 *   sums[i]    = double [2]: the sum of sqrt(a), the sum of sqrt(b), added in a fixed order without float atomics: the same bits on
 *                every run with the same capacities
 *   defined    both masks empty: defined = 1 and every other entry 0.  Exactly one empty: defined = 0, entries 2..5 are -1, entry 6
 *              and the sums are 0 (entries 0, 1 and 7 as above).  Otherwise defined = 1.
 * From these on the host: hd = sqrt(max(record[2], record[3])); hd95 = sqrt(v[lo]) + (sqrt(v[hi]) - sqrt(v[lo])) * rem / 100 (numpy's
 * linear percentile of sqrt(v)); assd = (sums[0] / |dP| + sums[1] / |dG|) / 2; cover_radius = ceil(sqrt(cover_d2)).
 * Misfit: the rule of uwm_score_masks_ragged with sides limited to 32768 and no radius: a side outside 1 .. 32768, h_i * w_i >
 * max_pixels, a region that leaves [0, mask_bytes), or, counting the images before it that pass those tests, a sum of rows above
 * `rows` or of h_i * ceil(w_i / 64) above mask_bytes / 64 + rows.  A misfit's record is status 1 and zeros, its sums are 0 and it
 * costs the others nothing.  Thirteen launches whatever N (N <= 65535) and the masks hold; max_pixels (1 .. 2^31 - 2) sizes the grids.
 * Every per-pixel array of the workspace is indexed like the masks, so it grows with mask_bytes: 8 bytes per mask byte for the
 * transform, 36 for the surface call.  Whatever the descriptors hold, no read leaves the masks / descs and no write leaves d2 +
 * [0, mask_bytes), records, sums or the workspace; overlapping regions are the caller's error.  descs / records / sums / workspace
 * 8-byte aligned, d2 4-byte.  Every argument is checked before any launch; no host synchronisation, allocation or copy. */
#define UWM_EDT_NONE 2147483647
size_t uwm_edt_workspace_bytes(int N, size_t mask_bytes, long long rows);
int    uwm_edt_ragged(const uint8_t* masks, size_t mask_bytes, const uwm_image_desc* descs /* device */, int N, long long max_pixels,
                      long long rows, int* d2 /* device [mask_bytes] */, void* workspace, size_t workspace_bytes, uwm_stream stream);
size_t uwm_surface_distances_workspace_bytes(int N, size_t mask_bytes, long long rows);
int    uwm_surface_distances_ragged(const uint8_t* pred, const uint8_t* truth, size_t mask_bytes,
                                    const uwm_image_desc* descs /* device */, int N, long long max_pixels, long long rows,
                                    long long* records /* device [N][10] */, double* sums /* device [N][2] */, void* workspace,
                                    size_t workspace_bytes, uwm_stream stream);
/* Mask enhancement on the device: the reference's enhance_mask (src/scripts/enhance_masks.py:16-67), which turns a tight
 * segmentation mask into the rounded, enlarged one people train on.  A ragged batch in ONE call, as above: image i is descs[i].h x
 * descs[i].w 8-bit grey pixels at in + descs[i].offset (any alignment), its result, in {0, 255}, goes to out + descs[i].offset; out
 * may be in.  With e = expand_pixels, k = blur_kernel (an even k is raised by one, 0 = no blur), s = smooth_iterations:
 *   1 m = grey close E(7,7) (dilate = max, then erode = min)     2 m = grey dilate E(2e+1, 2e+1)
 *   3 f = float32(m), blurred by the k x k Gaussian when k > 0     4 s times: f = open E(5,5), then close E(5,5), on floats
 *   5 u = f > 127 ? 255 : 0                                        6 u = bilateralFilter(u, 9, 75, 75), then u > 127 ? 255 : 0
 * computed as the chain 1, 2, 3, 5, then s times a BINARY open and close E(5,5): thresholding commutes with min and max, and step
 * 6 is the identity on a {0, 255} image (tests/test_enhance.py holds both against the literal chain).
 *   elements    the ELLIPSE rule above at odd sides 1..63: row i of E(2r+1, 2r+1) spans columns [r - dx, r + dx + 1),
 *               dx = round_half_even(r * sqrt((r*r - dy*dy) / (r*r))), dy = i - r; 1 x 1 is the identity; anchor at the centre;
 *               pixels outside the image are ignored, by max and by min
 *   taps        cv2.getGaussianKernel(k, 0, CV_32F): k = 1, 3, 5, 7 the fixed tables {1}, {.25, .5, .25}, {.0625, .25, .375, .25,
 *               .0625}, {.03125, .109375, .21875, .28125, .21875, .109375, .03125}; k >= 9 in double, sigma = ((k-1)*0.5 - 1)*0.3
 *               + 0.8, t_i = exp(-0.5 * x*x / sigma^2), x = i - (k-1)/2, divided by their double sum, rounded to float32
 *   blur        this library's own arithmetic (OpenCV's float filter differs by build): row pass (result stored as float32),
 *               then column pass, each acc = t[c]*x[0], then for i = 1 .. r in order acc += t[c+i] * (x[-i] + x[+i]), every
 *               operation rounded to float32, no fused multiply-add; border BORDER_REFLECT_101 by borderInterpolate's loop
 *               (length 1: index 0; else p = -p below 0 and p = 2*(len-1) - p from len on, repeated until inside)
 * OpenCV is not available to this project: every OpenCV rule here is restated, not run against cv2; equality with cv2 is claimed
 * only away from blurred values within a few ulp of 127.  Results are exact and the same on every run.
 * stats (device, may be NULL): long long [N][4] = {foreground (> 127) pixels of the input, of the output, h_i * w_i, status: 0
 * done, 1 misfit}.  The descriptors are read on the device; the host arguments are capacities, so one captured call serves every
 * batch of N images that fits them: max_pixels (1 .. 2^31 - 2) bounds h_i * w_i and sizes the grids.  The launch count does not
 * depend on N (N <= 65535).  Misfit: a side outside 1 .. 2^30, h_i * w_i > max_pixels, or a region that leaves [0, mask_bytes).  A
 * misfit gets status 1 and entries 0..2 zero, its bytes are not written and it costs the others nothing.  Whatever the descriptors
 * hold, no read leaves in / descs and no write leaves out + [0, mask_bytes), stats or the workspace; overlapping regions are the
 * caller's error.  Ranges: expand_pixels 0..31, blur_kernel 0..63, smooth_iterations 0..8.  workspace:
 * uwm_enhance_masks_workspace_bytes(N, mask_bytes) bytes (0 and a message on a bad argument), descs / stats / workspace 8-byte
 * aligned.  Every argument is checked before any launch; no host synchronisation, allocation or copy. */
size_t uwm_enhance_masks_workspace_bytes(int N, size_t mask_bytes);
int    uwm_enhance_masks_ragged(const uint8_t* in, uint8_t* out /* may alias in */, size_t mask_bytes,
                                const uwm_image_desc* descs /* device */, int N, int expand_pixels, int blur_kernel,
                                int smooth_iterations, long long max_pixels, long long* stats /* device [N][4], may be NULL */,
                                void* workspace, size_t workspace_bytes, uwm_stream stream);
/* host only, no device: the taps the blur uses for blur_kernel 0..63 (0 and 1: the one tap {1}) -> out[0 .. k), returns the
 * effective k (even + 1), or 0 and a message on a bad argument; out holds up to 63 floats */
int    uwm_enhance_gauss_taps(int blur_kernel, float* out);
/* Text-feature enhancement on the device: the reference's WatermarkPredictor._enhance_text_features (src/predict.py:370-404), the
 * OpenCV chain it runs on an image before the network sees it when the mask type is text or mixed.  A ragged batch in ONE call:
 * image i is descs[i].h x descs[i].w x 3 interleaved RGB bytes at in + descs[i].offset (any alignment), its result goes to out +
 * descs[i].offset; out must not overlap in (the last stage reads neighbours).  Six stages, each image at its own size:
 *   1 grey     g = (R*9798 + G*19235 + B*3735 + 16384) >> 15                                       cvtColor(RGB2GRAY), 8 bit
 *   2 CLAHE    createCLAHE(2.0, (8, 8)).apply(g): when h % 8 or w % 8 is non-zero the plane is extended at the bottom by 8 - h % 8
 *              rows AND at the right by 8 - w % 8 columns (a side that divides grows by a full 8), BORDER_REFLECT_101; tile th x tw
 *              = the (extended) size / 8; per tile the 256-bin histogram, clipped at max(int(2.0 * th*tw / 256), 1), the excess
 *              handed out (excess / 256 to every bin, the rest one each to bins 0, s, 2s, ... with s = max(256 / rest, 1)), table[v] =
 *              rint(float32(cumulative sum) * (255.0f / float32(th*tw))); per pixel f = y * (1.0f / th) - 0.5f, tiles floor(f) and
 *              floor(f) + 1 clamped to 0..7, weight a = f - floor(f), likewise in x; c = rint((t11*(1-xa) + t12*xa)*(1-ya) +
 *              (t21*(1-xa) + t22*xa)*ya), every float32 operation rounded on its own
 *   3 Canny    Canny(c, 50, 150), aperture 3, L2gradient = false: dx, dy = the 3 x 3 Sobel derivatives, BORDER_REPLICATE; m = |dx| +
 *              |dy|, 0 outside the image.  A pixel is a candidate when m > 50 and, with x = |dx|, y = |dy| << 15, t = x * 13573:
 *              y < t: m > m(left) and m >= m(right); else y > t + (x << 16): m > m(above) and m >= m(below); else, s = -1 when
 *              (dx ^ dy) < 0, otherwise 1: m > m(y-1, x-s) and m > m(y+1, x+s).  The edge image is 255 on the candidates that are
 *              8-connected, through candidates, to a candidate with m > 150, else 0
 *   4 dilate   with getStructuringElement(MORPH_ELLIPSE, (2, 2)) = [[0,1],[1,1]], anchor (1, 1): d(y, x) = max(e(y-1, x), e(y, x-1),
 *              e(y, x)); pixels outside the image are ignored
 *   5 boost    where d != 0 every channel value v becomes trunc(min(float32(v) * 1.2f, 255))
 *   6 sharpen  filter2D with [[-1,-1,-1],[-1,9,-1],[-1,-1,-1]] per channel of the boosted image, BORDER_REFLECT_101, saturated
 * Every OpenCV rule here is restated, NOT run against cv2 (DESIGN.md 8n lists them); tests/textenh_ref.py is the literal form the
 * kernels are held to byte for byte.  edges (may be NULL; then edges_bytes and edge_descs are ignored): receives d, one byte per pixel
 * in {0, 255}, at edges + edge_descs[i].offset; edge_descs[i] must carry image i's h and w.  The descriptors are read on the device;
 * the host arguments are capacities, so one captured call serves every batch of N images that fits them: max_pixels (1 .. 2^30) bounds
 * h_i * w_i and sizes the grids, total_pixels (1 .. 2^40) bounds the sum of h_i * w_i over the enhanced images and sizes the workspace.
 * The launch count (11) does not depend on N (N <= 65535) or on what the images hold.  Per-image status: the first N ints of the
 * workspace after the call = 0 enhanced | 1 misfit, nothing written (a side outside 1 .. 2^30, h*w > max_pixels, a region that leaves
 * [0, bytes) or [0, edges_bytes), an edge descriptor of another size, or a sum of h*w over the enhanced images up to this one above
 * total_pixels) | 2 a side below 16: the image is copied through unchanged and its edge plane is 0.  A misfit costs the others
 * nothing.  Whatever the descriptors hold, no read leaves in / the descriptors and no write leaves out + [0, bytes), edges + [0,
 * edges_bytes) or the workspace; overlapping regions are the caller's error.  workspace:
 * uwm_text_enhance_workspace_bytes(total_pixels, N) bytes (0 and a message on a bad argument); descriptors and workspace 8-byte
 * aligned.  Every argument is checked before any launch; no host synchronisation, allocation or copy.  Integer atomics only: runs
 * are bit-identical. */
enum { UWM_TEXT_ENHANCE_DONE = 0, UWM_TEXT_ENHANCE_MISFIT = 1, UWM_TEXT_ENHANCE_COPIED = 2, UWM_TEXT_ENHANCE_MIN_SIDE = 16 };
size_t uwm_text_enhance_workspace_bytes(long long total_pixels, int N);
int    uwm_text_enhance_ragged(const uint8_t* in, uint8_t* out, size_t bytes, const uwm_image_desc* descs /* device */, int N,
                               int C /* 3 */, long long max_pixels, long long total_pixels,
                               uint8_t* edges /* may be NULL */, size_t edges_bytes, const uwm_image_desc* edge_descs /* device */,
                               void* workspace, size_t workspace_bytes, uwm_stream stream);
/* Membrane (harmonic) fill on the device: what `repair` puts in the place of the predicted watermark.  A ragged batch in ONE call:
 * image i is img_descs[i].h x img_descs[i].w x C interleaved bytes at images + img_descs[i].offset (any alignment), its mask is one
 * byte per pixel at masks + mask_descs[i].offset (a byte != 0 is a hole pixel) and must have the image's size; the result goes to
 * out + img_descs[i].offset; out may BE images (no other overlap).  Per image and channel, in float32, every operation rounded on
 * its own and every division IEEE (tests/inpaint_ref.py is the numpy form the bytes are held to):
 *   levels    level 0 is the image, level l + 1 has ((h_l + 1) >> 1) x ((w_l + 1) >> 1) cells, L = ceil(log2(max(h, w)));
 *             children of (Y, X) in this order: (2Y, 2X), (2Y, 2X+1), (2Y+1, 2X), (2Y+1, 2X+1); neighbours of (y, x) in this order:
 *             up, left, right, down; in both cases those inside the level only.  S(p) = the neighbours' sum in that order, cnt
 *             their number.  up(c)(y, x) = ((9 c[py][px] + 3 c[py][qx]) + (3 c[qy][px] + c[qy][qx])) * 0.0625f, py = y >> 1,
 *             qy = clamp(py + (y & 1 ? 1 : -1), 0, rows of c - 1), likewise in x
 *   sweep     at level l with right-hand side b: the unknown cells with y + x even, then those with y + x odd, each u = (b + S) / cnt
 *   1 pull    v_0 = the byte at known pixels (valid); a coarse cell with n > 0 valid children: v = their sum in children order / n
 *   2 push    g_L = v_L; for l = L-1 .. 0: g_l = v_l where valid, else up(g_{l+1}), then one sweep with b = 0 over the non-valid
 *             cells; u = g_0
 *   3 cycles  `cycles` times V(0) on cnt * u - S = 0 over the hole pixels H_0.  H_{l+1} = the cells all of whose children are in
 *             H_l; on levels >= 1 the values outside H_l are zero.  V(l): two sweeps; r = b - (cnt * u - S) on H_l; if l < L:
 *             b_{l+1}(P) = the children's r in children order on H_{l+1}, e_{l+1} = 0, V(l+1), u += up(e_{l+1}) on H_l; two sweeps
 *   4 store   hole pixels rint(min(max(u, 0), 255)), half to even; known pixels byte for byte
 * stats (device, may be NULL): long long [N][4] = {hole pixels, status, levels that held unknowns, 0}; status 0 filled | 1 no hole
 * pixel | 2 no known pixel (both: the output is the input, entry 2 is 0) | 3 misfit, nothing written, entries 0 and 2 zero.  The
 * descriptors are read on the device; the host arguments are capacities, so one captured call serves every batch of N images that
 * fits them: max_pixels (1 .. 2^30) bounds h_i * w_i, max_side (1 .. 32768) bounds every side and sets the number of levels, rows
 * (1 .. 2^40) bounds the sum of h_i; grids are sized from N, max_pixels and max_side.  Misfit: a side outside 1 .. max_side, h_i * w_i
 * > max_pixels, a region that leaves [0, image_bytes) or [0, mask_bytes), a mask of another size, or, counting the images before it
 * that pass those tests, a sum of rows above `rows` or of cells above the workspace's planes (sized from image_bytes / C pixels).  A
 * misfit costs the others nothing.  The launch count, uwm_inpaint_launch_count(cycles, max_side) = 5 + L + lc + cycles * (2 lc + 1)
 * with L = ceil(log2(max_side)) and lc the first level whose sides fit 64 (from there on the levels run in LDS), depends on nothing
 * else.  Work after the pull is done only in 32 x 32 tiles that hold a hole pixel (per level: an unknown).  Whatever the descriptors
 * hold, no read leaves images / masks / the descriptors and no write leaves out + [0, image_bytes), stats or the workspace;
 * overlapping regions are the caller's error.  workspace: uwm_inpaint_workspace_bytes(N, image_bytes, C, max_side) bytes (0 and a
 * message on a bad argument): two float planes per channel at level 0 and three above (8 C + 4 C + 0.4 bytes per pixel of
 * image_bytes / C, plus about 24 C max_side bytes per image).  Descriptors, stats and workspace 8-byte aligned.  Every argument is checked
 * before any launch; no host synchronisation, allocation or copy.  Integer atomics only: runs are bit-identical. */
enum { UWM_INPAINT_FILLED = 0, UWM_INPAINT_NO_HOLE = 1, UWM_INPAINT_NO_KNOWN = 2, UWM_INPAINT_MISFIT = 3 };
size_t uwm_inpaint_workspace_bytes(int N, size_t image_bytes, int C, int max_side);
int    uwm_inpaint_launch_count(int cycles /* 0..32 */, int max_side);        /* host only; 0 and a message on a bad argument */
int    uwm_inpaint_ragged(const uint8_t* images, uint8_t* out /* may alias images */, size_t image_bytes,
                          const uwm_image_desc* img_descs /* device */, const uint8_t* masks, size_t mask_bytes,
                          const uwm_image_desc* mask_descs /* device */, int N, int C /* 1..4 */, int cycles /* 0..32 */,
                          long long max_pixels, long long rows, int max_side, long long* stats /* device [N][4], may be NULL */,
                          void* workspace, size_t workspace_bytes, uwm_stream stream);
/* Watermark cut-outs from watermarked / clean pairs on the device: the reference's extract_watermarks.py (extract_watermark_from_pair,
 * _extract_single_watermark / _extract_combined_watermark, _create_transparent_watermark), whose transparent RGBA cut-outs are the logos
 * gen_data.py pastes.  Two calls with a small host plan between them (extract.plan_cutouts: centres, clustering, margins).
 * STAGE 1, uwm_extract_regions_ragged.  wm, clean: ragged batches as above (uint8 RGB interleaved, C = 3); pair i at its OWN size:
 *     g = gray(|wm - clean|), the rule of uwm_pair_mask_u8; m = g > threshold                     absdiff, cvtColor, threshold
 *     m = open(close(m, RECT(3,3)), RECT(3,3)), one iteration each, the morphology of               morphologyEx(np.ones((3,3)))
 *         uwm_optimize_mask: pixels outside the image are ignored
 *     F = m plus every background pixel that is not 4-connected through background to the           findContours(RETR_EXTERNAL) +
 *         outside of the image: holes are filled, islands in holes join the enclosing region       fillPoly of each outer contour
 *     regions = the 8-connected components of F; id = y*w + x of the raster-first pixel
 *     per region, over every 2 x 2 window of neighbouring pixels (top-left corner (x, y)):          contourArea / moments of the outer
 *         4 corners in F: a00 += 2, a10 += 6x + 3, a01 += 6y + 3                                   contour = the polygon through the
 *         3 corners in F: a00 += 1, a10 += the three corners' x, a01 += the three corners' y       pixel centres: area = a00/2,
 *         fewer: nothing                                                                           m10 = a10/6, m01 = a01/6
 *     kept = the regions with a00 > 2*min_area                                                     contourArea(c) > min_area
 *   -> stats[i][4] = {regions found, regions kept, status, h_i*w_i}; table[i][254][9], one row per kept region in ascending id order =
 *   {id, a00, a10, a01, x0, y0, x1, y1 (bounding box, inclusive), pixels of F}, the other rows zero; plane + plane_descs[i].offset <-
 *   one byte per pixel: the row index of the kept region at that pixel, 255 for none.  status: 0 done; 1 misfit (a side outside
 *   3 .. 2^30, sizes of wm / clean / plane that differ, h*w > max_pixels, a region that leaves its buffer, or a sum of h*w, over the
 *   pairs up to this one that pass those tests, above total_pixels): found = kept = h*w = 0, its plane bytes are not written; 2 more than 254
 *   kept regions: found and kept are reported, the table is empty and the plane all 255.  Every OpenCV rule here is restated, NOT
 *   run against cv2; tests/test_extract.py holds the window sums and the fill to a literal border follower with the shoelace
 *   formulas and to scipy's binary_fill_holes.  A pair whose two files differ in size is first brought to (min w, min h) by
 *   uwm_resize_u8(UWM_INTER_LINEAR): the caller's step.
 * STAGE 2, uwm_extract_cutouts_ragged.  Job j: the crop (x, y, w, h) of image `image`, written as w*h RGBA pixels at out + out_offset:
 *   RGB from wm, A = 255 where member[plane byte] != 0 (the byte 255 is never a member), else 0; then, over RGB with alpha carried:
 *     ImageEnhance.Contrast(1.3)     blend(d, p, 1.3f), d = (int)(sum of L over ALL crop pixels / (w*h) + 0.5) in float64,
 *                                    L = (19595*R + 38470*G + 7471*B + 0x8000) >> 16
 *     ImageEnhance.Sharpness(1.4)    blend(d, p, 1.4f), d = ImageFilter.SMOOTH of the contrast stage: k1 = 1.f/13.f, k5 = 5.f/13.f,
 *                                    ss = 0.5f; for the rows y+1, y, y-1: ss += (l*k1 + c*kc) + r*k1 (kc = k5 on row y, else k1), every
 *                                    operation rounded to float32, no fused multiply-add; d = 0 for ss <= 0, 255 for ss >= 255, else
 *                                    (int)ss; the one-pixel frame of the crop is not filtered (d = p)
 *     ImageEnhance.Brightness(1.1)   blend(0, p, 1.1f)
 *     blend(d, p, f) in float32: t = d + f*(p - d); 0 for t <= 0, 255 for t >= 255, else (int)t      (Image.blend, as in uwm_synth_u8)
 *   held to Pillow bit for bit by tests/test_extract.py.  status[j]: 0 done; 1 misfit, nothing written (an image index outside 0..N-1, an
 *   image or plane descriptor that fails stage 1's tests, a crop side below 3 or a crop outside the image, w*h > max_crop_pixels,
 *   out_offset negative, not a multiple of 4, or a region that leaves [0, out_bytes)).
 * Both calls: descriptors and jobs are read on the device, the host arguments are capacities (max_pixels 1 .. 2^30 bounds h_i*w_i,
 * total_pixels their sum, max_crop_pixels a crop; all size the grids and the workspace), so one captured call serves every batch that
 * fits them; the launch count (18 and 3) does not depend on N or J (both <= 65535).  A misfit costs the others nothing.  Whatever the
 * descriptors hold, no read leaves the inputs and no write leaves plane + [0, plane_bytes), out + [0, out_bytes), stats, table, status or
 * the workspace; overlapping output regions are the caller's error.  workspace: uwm_extract_workspace_bytes(N, total_pixels, J) bytes
 * serves both calls (N = 0 or J = 0: the other call alone; 0 and a message on a bad argument).  wm / clean / out 4-byte, descriptors /
 * jobs / stats / table / workspace 8-byte aligned.  Every argument is checked before any launch; no host synchronisation, allocation
 * or copy.  Integer sums and extrema have one result whatever their order, so runs are bit-identical. */
enum { UWM_EXTRACT_MAX_REGIONS = 254, UWM_EXTRACT_ROW_INTS = 9 };
typedef struct uwm_extract_job {
  int image;                   /* index into the descriptors */
  int x, y, w, h;              /* the crop, inside the image, sides >= 3 */
  int reserved;
  long long out_offset;        /* bytes, a multiple of 4 */
  uint8_t member[256];         /* member[k] != 0: kept region k of the image belongs to this cut-out */
} uwm_extract_job;
size_t uwm_extract_workspace_bytes(int N, long long total_pixels, int J);
int    uwm_extract_regions_ragged(const uint8_t* wm, size_t wm_bytes, const uwm_image_desc* wm_descs,
                                  const uint8_t* clean, size_t clean_bytes, const uwm_image_desc* clean_descs,
                                  int N, int C /* 3 */, int threshold /* 0..255 */, int min_area, long long max_pixels,
                                  long long total_pixels, uint8_t* plane, size_t plane_bytes, const uwm_image_desc* plane_descs,
                                  long long* stats /* device [N][4] */, long long* table /* device [N][254][9] */,
                                  void* workspace, size_t workspace_bytes, uwm_stream stream);
int    uwm_extract_cutouts_ragged(const uint8_t* wm, size_t wm_bytes, const uwm_image_desc* wm_descs,
                                  const uint8_t* plane, size_t plane_bytes, const uwm_image_desc* plane_descs, int N,
                                  const uwm_extract_job* jobs /* device [J] */, int J, long long max_crop_pixels,
                                  uint8_t* out, size_t out_bytes, int* status /* device [J] */,
                                  void* workspace, size_t workspace_bytes, uwm_stream stream);
/* building blocks, for tests and other callers; out may alias in */
int    uwm_op_morph(const uint8_t* in, uint8_t* out, int N, int H, int W, int dilate, int shape, int kw, int kh,
                    int iterations, void* workspace, size_t workspace_bytes, uwm_stream stream);
int    uwm_op_components(const uint8_t* in, int32_t* labels /* [N][H][W]: id+1, 0 = background */,
                         int32_t* areas /* [N][H][W]: area at the id pixel, 0 elsewhere */, int N, int H, int W,
                         void* workspace, size_t workspace_bytes, uwm_stream stream);

/* Weight-gradient kernels run on an internal side stream (forked from / joined to the caller's stream with events,
 * per backward stage) so they overlap the dgrad chain; this switches that off/on at run time (default on). */
int  uwm_set_side_stream(uwm_handle h, int on);

/* Optional HIP-event profiler: while enabled every conv / wgrad launch carries a hipEvent pair attached to the kernel
 * dispatch itself (hipExtLaunchKernelGGL: the dispatch's own begin / end timestamps, the clock rocprofv3's kernel trace
 * reads).  uwm_prof_collect waits for the events and returns, per kernel class, {launches, total ms, total algorithmic
 * FLOPs, total algorithmic HBM bytes} in out[class*4 + 0..3] (out: >= 4*max_classes doubles); returns the number of
 * classes. */
int  uwm_prof_enable(int on);
int  uwm_prof_collect(double* out, int max_classes);
const char* uwm_prof_class_name(int cls);

/* Workspace introspection for parity tests: element offset (in floats from the workspace base) and
 * element count of a planned intermediate.  Keys: "y:<conv>", "g:<conv>" (raw conv output / its
 * gradient; <conv> = state_dict prefix such as "encoder.layer1.0.conv1"), "xn:<i>", "gx:<i>"
 * (encoder block i output / masked gradient), "pool", "g_pool", "x4", "dcat:<i>", "gskip:<i>".
 * The fixed (shape-independent) region needs no plan: "fixed" (all of it, offset 0), "bnf:<bn>" (a BatchNorm's {scale[C],
 * shift[C]}; <bn> = state_dict prefix such as "encoder.bn1"), "wu:<conv>" / "wud:<conv>" / "wd:<conv>" (a conv's forward bank
 * slot / dgrad bank slot / dgrad repack; count 0 where the layer has none). */
int  uwm_debug_lookup(uwm_handle h, const char* key, long long* offset, long long* count);

/* ---- single-operator entry points (used by the parity tests) ---- */
typedef struct {
  const float* ptr; const float* scale; const float* shift;   /* NHWC fp32, optional lazy affine */
  int C, H, W, up, relu;
} uwm_src;
/* y[N][Ho][Wo][Cout] = conv(cat(s0,s1), w) ; w [Cout][Kpad] packed (k = tap*Ctot + c).
 * stats (2*Cout doubles: sum, sumsq; pre-zeroed) may be NULL.
 * cfg (tests / timing; every code the library accepts, anything else is an error):
 *    -1         the library's routing
 *    0..5       flattened implicit GEMM, tile configuration {BM, BN}: 0 {128,128} 1 {128,64} 2 {128,32} 3 {128,16} 4 {64,64} 5 {64,128}
 *    100+BN     direct patch kernel, BN = 16 | 32 | 64 | 128 output channels per workgroup (conv_patch.hip)
 *    200        16-channel patch kernel (conv_patch16.hip)
 *    300, 300+BN  Winograd F(2x2,3x3): 300 auto tile, BN = 16 | 32 | 64; 308 = the 8-wave variant (conv_wino8.hip)
 *    400        Winograd in bf16x3 arithmetic (conv_wino_x3.hip)
 *    500        segmentation-head streaming kernel (conv_head.hip)
 *    600..603   fp16x3 direct form: 600 = the kernel the model would take (conv_f16x3.hip or conv_f16x3v2.hip by shape); conv_f16x3.hip's
 *               601 four-wave kernel | 602 eight-wave kernel | 603 four-wave kernel, 32-channel tiles
 *    607, 605   conv_f16x3v2.hip (whole 8 x 32-pixel tiles, Cout % 32 == 0, 32-channel tiles): 607 = its kernel (8 waves), 605 = the 4-wave
 *               kernel no routing takes.  604 and 606 named removed forms: rejected
 *    1600..1603, 1605, 1607  = 6xx without re-packing the filter bank (kernel-only timing: the previous call must have been the same layer and code)
 *    610        the 7x7 / stride-2 ResNet stem in fp16x3 arithmetic (conv_stem_f16x3.hip; 4 stored input channels, 64 outputs)
 *    700        sub-pixel kernel for a 3x3 over a nearest-x2 upsampled 32-channel source with 16 outputs (conv_up2.hip; with
 *               uwm_op_set_igemm_f16x3(1): conv_up2_f16.hip)
 *    710, 711   3x3 16 -> 16 / 32 -> 32 at full resolution in fp16x3 arithmetic (conv_c16_f16.hip)
 *    800, 864, 928  persistent LDS-DMA GEMM for 1x1 / stride-1 layers with Cin % 32 == 0 (conv_gemm.hip): auto | 64 | 128 channel tile
 * Two test hooks go with the 600..607 codes:
 *    uwm_op_set_f16x3_products(n)   split products per tile (ConvArgs::nprod) of every later uwm_op_conv cfg 600..607 and
 *               uwm_op_dgrad_f16x3 launch: 3 = hi*hi' + hi*lo' + lo*hi' (the default), 2 = without the pixel operand's low half,
 *               1 = hi*hi' only; anything else is an error.  The model takes its count from the precision mode, never from here.
 *               The same count goes to uwm_op_wgrad force_igemm 6 / 7 (WgradArgs::nprod), where wgrad_f16x3.hip reads it:
 *               3 = dy_hi*x_hi + dy_hi*x_lo + dy_lo*x_hi, 2 = without dy_lo*x_hi, 1 = dy_hi*x_hi only.
 *    uwm_op_dgrad_f16x3(...)        the DGRAD role of the same kernels, as the model's backward launches it: see its declaration.
 * A 600..607 call whose coded kernel does not take the shape returns an error before anything is launched. */
/* preprocess_u8_nhwc4 alone (uwm_predict_u8's input kernel): uint8 [npix][C] (4-byte aligned, C 1..4) -> Normalize as fp32 [npix][4]
 * (16-byte aligned), padding channels zero; any pixel count */
int  uwm_op_preprocess_u8_nhwc4(const uint8_t* images, long long npix, int C, const float* mean, const float* std, float* out,
                                uwm_stream stream);
/* on = 1: ... with the weight operand pre-split into a bank by one job of the fp16x3 bank launch, built on the fly (the model builds
 * its banks once per step); on = 2: the same arithmetic with the weights split while staging (bit-identical products; the form
 * behind UWM_DEBUG=1 UWM_NO_IG_BANK=1 in the model); 0: exact fp32 */
int  uwm_op_set_igemm_f16x3(int on);   /* tests / kernel timing: uwm_op_conv / uwm_op_dgrad launches that end on the implicit GEMM (stride 2, 1x1) use its fp16x3 split-product form (what the model does for the stride-2 layers in the fp16x3 precision modes) */
int  uwm_op_conv(const uwm_src* s0, const uwm_src* s1, const float* w, int wrows, int Kpad, int kh, int kw, int stride,
                 int pad, int N, int Cout, const float* bias, float* y, double* stats, int cfg, uwm_stream stream);
/* dx[N][H][W][Cin] = conv_transpose(dy[N][Ho][Wo][Cout], wd) (+addend, *relu-mask) ; wd [Cin][KpadD] */
int  uwm_op_dgrad(const float* dy, int N, int Ho, int Wo, int Cout, const float* wd, int Cin, int KpadD, int kh, int kw,
                  int stride, int pad, int H, int W, const float* addend, const float* mask, const float* mscale,
                  const float* mshift, float* dx, uwm_stream stream);
int  uwm_op_set_f16x3_products(int n);   /* tests: n = 1 | 2 | 3 split products in the op-level fp16x3 direct launches (see cfg above) and in uwm_op_wgrad force_igemm 6 on wgrad_f16x3.hip; default 3 */
/* dx[N][H][W][Cin] = the 3x3 / stride-1 / pad-1 input gradient on an fp16x3 direct kernel (cfg = 600 | 601 | 602 | 603 | 605 | 607, as
 * uwm_op_conv's; 600 = conv_f16x3v2.hip where the model would take it for this layer, else conv_f16x3.hip), launched as the model's
 * backward launches it.  dy [N][H][W][CoutP] (CoutP % 32 == 0, channels >= Cout zero); w = the FORWARD weights [Cout][Kpad],
 * k = tap * Cin + c, from which the tap-mirrored filter bank is packed; dY is staged times the power of two that puts max|dY|
 * (a one-off reduction) into [2^13, 2^14).  Epilogue: dx = (conv + addend) where (mask * mscale + mshift) > 0, else 0 (each optional;
 * mscale / mshift [Cin] come together).  bnb_mean / bnb_rstd [Cin] (optional): the fused BatchNorm-backward sums — sums[c] += dx,
 * sums[Cin + c] += dx * (y - mean) * rstd with y = bnb_y if given, else the mask tensor — workgroup b adding into replica
 * b & (nrep - 1) at sums + replica * sums_stride doubles (nrep a power of two; the caller zeroes every replica).  sums without
 * bnb_mean: (sum, sum of squares) of dx.  A shape the coded kernel does not take is an error and nothing is launched. */
int  uwm_op_dgrad_f16x3(const float* dy, int N, int H, int W, int Cout, int CoutP, const float* w, int Kpad, int Cin,
                        const float* addend, const float* mask, const float* mscale, const float* mshift, const float* bnb_mean,
                        const float* bnb_rstd, const float* bnb_y, double* sums, int nrep, long long sums_stride, float* dx, int cfg,
                        uwm_stream stream);
/* force_igemm (tests / timing), low byte: 0 = the library's routing (Winograd-domain / sub-pixel / 16-channel / stem / 1x1-GEMM /
 * fp16x3 kernels where they apply); 1 = flattened implicit GEMM only; 2 = none of the dedicated kernels but wgrad_patch.hip; 4 =
 * wgrad_gemm.hip (an error where it does not apply); 6 = the dedicated fp16x3 kernels (wgrad_f16x3.hip: 3x3 stride 1, channels % 32 == 0,
 * Wo % 32 == 0, Ho % 4 == 0; the sub-pixel, stem and 16-channel kernels in their fp16x3 forms; an error elsewhere); 7 = the flattened
 * implicit GEMM in its fp16x3 form.  6 and 7 take max|dy| through a one-off reduction, and the split products per tile from
 * uwm_op_set_f16x3_products (default 3; wgrad_f16x3.hip alone has the 1- and 2-product forms, the other kernels ignore the count). */
int  uwm_op_wgrad(const uwm_src* s0, const uwm_src* s1, const float* dy, int N, int Ho, int Wo, int Cout, int wrows,
                  int Kpad, int kh, int kw, int stride, int pad, float* dw, int force_igemm, uwm_stream stream);
int  uwm_op_pack_dgrad(const float* w, int Cout, int Kpad, int ntaps, int Cin, float* wd, int KpadD, int CoutP,
                       uwm_stream stream);
int  uwm_op_maxpool(const uwm_src* in, int N, float* out, uint8_t* idx, uwm_stream stream);
/* gin[N][H][W][C] = (maxpool3x3s2_backward(gout, idx) + addend) * [relu(in) > 0] */
int  uwm_op_maxpool_backward(const float* gout, const uint8_t* idx, const float* addend, const uwm_src* in, int N,
                             float* gin, uwm_stream stream);
/* BatchNorm backward (batch statistics): g = grad wrt the BN output, y = BN input; scratch2c: 2*C doubles.
 * dy = gamma*rstd*(g - mean(g) - yhat*mean(g*yhat)), dgamma = sum g*yhat, dbeta = sum g */
int  uwm_op_bn_backward(const float* g, const float* y, const float* mean, const float* rstd, const float* gamma,
                        double* scratch2c, float* dy, float* dgamma, float* dbeta, long long npix, int C, uwm_stream stream);
/* BatchNorm backward behind swish [and the squeeze-and-excitation product] (EfficientNet MBConv): y = BN input [N][hw][C],
 * scale / shift = gamma*rstd / beta - mean*gamma*rstd (the forward's swish(y*scale + shift)); g = grad wrt the swish output or,
 * with se_s / gpool ([N][C] each, both or neither), wrt swish(.) * se_s, the pooled branch contributing gpool / hw.
 * Writes dy = grad wrt y, dgamma, dbeta; scratch2c: 2*C doubles; xmax (optional, 32 floats): max over its slots = max|dy|, the
 * value the fp16x3 dgrad / wgrad that reads dy scales by */
int  uwm_op_bn_backward_act(const float* g, const float* y, const float* mean, const float* rstd, const float* gamma,
                            const float* scale, const float* shift, const float* se_s, const float* gpool, int N, long long hw,
                            int C, double* scratch2c, float* dy, float* dgamma, float* dbeta, float* xmax, uwm_stream stream);
/* gradient of cat(nearest_x2(prev), skip): gprev[N][H/2][W/2][C0] = mask(sum 2x2 dcat[..., :C0]), gskip = dcat[..., C0:] */
/* decoder block conv1 dgrad with the concat split fused (Winograd epilogue): gprev [N][H/2][W/2][C0] = ReLU-masked
 * 2x2 sums of the first C0 gradient channels, gskip [N][H][W][C1] the rest; wd = uwm_op_pack_dgrad output */
int  uwm_op_dgrad_upsplit(const float* dy, int N, int H, int W, int Cout, const float* wd, int C0, int C1, int KpadD,
                          float* gprev, const float* pmask, const float* pscale, const float* pshift, float* gskip,
                          uwm_stream stream);
int  uwm_op_upsplit(const float* dcat, int N, int H, int W, int C0, int C1, float* gprev, const float* pmask,
                    const float* pscale, const float* pshift, float* gskip, uwm_stream stream);
/* out = relu(y*s2+b2 + (sd ? id*sd+bd : id)) */
int  uwm_op_residual(const float* y, const float* s2, const float* b2, const float* id, const float* sd, const float* bd,
                     float* out, long long npix, int C, uwm_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* UWM_H */
