/* vit_unet_amd.h - C ABI of libvitunet_amd.so, the MI355X (gfx950) ViT-UNet forward/backward path.
 *
 * This is the drop-in boundary for the hot path of benayas1/vit-unet.  The
 * reference has no native code: every entry point below replaces a run of PyTorch ATen calls
 * made by /root/reference/vit_unet/torch/model.py (cited per function as model.py:LINES).  The
 * Python package vit-unet_amd/vit_unet binds these symbols with ctypes (INTEGRATION.md shows the
 * stub) and mirrors the reference's nn.Module surface on top of them.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory unless stated otherwise;
 *  - all work is enqueued on the caller's `stream` (a hipStream_t passed as void*); no hidden
 *    synchronisation, no allocation; state between calls: the thread-local last-error text, the
 *    opt-in launch profiler below (process-global, one instrumented stream at a time), and two
 *    opt-in experiment switches that keep per-thread streams / events (VU_FLASH_FORK=1,
 *    VU_SIDE_LANE=1: off by default).  Environment switches (VU_ATTN_FLASH, VU_TSGEMM, ...) are
 *    A/B measurement aids read at call time;
 *  - return 0 (VU_OK) on success, negative VU_E* otherwise; vu_last_error() gives the text;
 *  - `dtype` selects the STORAGE type of activations / GEMM weights: 0 = fp32, 1 = bf16.
 *    Arithmetic is always fp32 (fp32 MFMA accumulators).  Parameters that are not GEMM operands
 *    (conv taps, head-mix matrix, BatchNorm / LayerNorm affine, biases, positional embedding)
 *    are always read from the fp32 master arena.
 */
#ifndef VIT_UNET_AMD_H
#define VIT_UNET_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VU_OK 0
#define VU_EINVAL (-1)
#define VU_EUNSUPPORTED (-2)
#define VU_EWORKSPACE (-3)
#define VU_ELAUNCH (-4)

int vu_version(void);      /* 200 = this header; bumped whenever a struct or a signature changes */
int vu_config_size(void);  /* sizeof(vu_config) as the library was built: a binding compares it with its own struct before any call */
const char* vu_last_error(void);

/* HViT_UNet constructor arguments (model.py:264-299). */
typedef struct vu_config {
  int depth, depth_te, size_bottleneck;
  int im_size, patch_size, num_channels, hidden_dim, num_heads;
  float attn_drop, proj_drop, linear_drop;
  int out_conv; /* preprocessing == 'conv' (model.py:369-370, 427-428) */
  int dtype;    /* 0 fp32, 1 bf16 */
  int attn_operands; /* 0: q, k, v enter the attention products as stored; 1: rounded to OCP e4m3 first
                      * (BASELINE config 5, "fp8 attention operands"; see vu_round_e4m3) */
} vu_config;

/* One parameter of the flat arena, in the reference's registration order (model.py:309-370);
 * `name` is the reference state_dict key.  Offsets are in elements and 8-element aligned. */
typedef struct vu_param_entry {
  char name[96];
  long long offset;
  int ndim;
  int shape[4];
  int bn_index; /* >= 0 for var_norm.weight: index of this module's running stats */
} vu_param_entry;

int vu_model_validate(const vu_config* cfg);                    /* asserts of model.py:281-283 */
long long vu_model_param_elems(const vu_config* cfg);           /* arena length (padded)       */
int vu_model_num_params(const vu_config* cfg);
int vu_model_param_table(const vu_config* cfg, vu_param_entry* out, int capacity);
int vu_model_num_attn(const vu_config* cfg);                    /* BatchNorm modules           */
size_t vu_model_workspace_bytes(const vu_config* cfg, int B);   /* = vu_model_workspace_bytes_ex(cfg, B, 1): fits either mode */
/* The workspace of an eval-mode forward (training = 0; model.py:372-435 under model.eval(), functions.py:7-19) leaves out what only a
 * training step uses: the probability caches of the recompute attention (vu_set_flash_pcache).  vu_model_forward / _backward carve by
 * their own `training` argument, so a workspace sized for training serves both and one sized for eval is refused by a training call
 * (VU_EWORKSPACE).  vu_model_pcache_bytes: the part of the training workspace that is probability cache (after the budget below). */
size_t vu_model_workspace_bytes_ex(const vu_config* cfg, int B, int training);
size_t vu_model_pcache_bytes(const vu_config* cfg, int B);
/* Diagnostic (no reference counterpart): the carve of that workspace as text, one "name offset bytes" line per buffer, the
 * forward's buffers in execution order.  Returns the length of the full text (snprintf convention), < 0 on a bad config. */
int vu_model_workspace_describe(const vu_config* cfg, int B, char* out, int cap);
/* 1 when a training step of this configuration at B images per GPU is faster launched eagerly than replayed from a captured
 * graph: the recompute attention's backward then runs its dv sweep on a low-priority stream in the tails of the dq / dk
 * sweeps (more workgroups than the chip holds at once), and a captured kernel node carries no stream priority.  Needs a
 * current device.  (No reference counterpart: launch policy of this library.) */
int vu_model_prefers_eager(const vu_config* cfg, int B);

/* HViT_UNet.forward (model.py:372-435).
 *  params      fp32 master arena            shadow   bf16 copy of the arena (dtype 1) or NULL
 *  bn_state    fp32 [num_attn][2][heads] running_mean / running_var (updated when training)
 *  x, y        fp32 (B, C, im, im)          ws       workspace of vu_model_workspace_bytes()
 *  training    1: BatchNorm batch statistics + dropout (seed); 0: running statistics
 *  rng_salt    optional device uint32 mixed into the dropout keys (hipGraph replay), or NULL */
int vu_model_forward(const vu_config* cfg, const float* params, const void* shadow, float* bn_state,
                     const float* x, float* y, void* ws, size_t ws_bytes, int B, int training,
                     uint64_t seed, const uint32_t* rng_salt, void* stream);
/* Backward of the forward that last filled `ws`.  Parameter gradients are ACCUMULATED into the
 * fp32 arena `grads`; dx (fp32 (B,C,im,im)) may be NULL.  stage: 0 = all, 1 = output conv +
 * decoders + skips, 2 = bottleneck, 3 = encoders + positional embedding (for bucketed
 * all-reduce overlap; stages must be run in order 1,2,3). */
int vu_model_backward(const vu_config* cfg, const float* params, const void* shadow,
                      const float* bn_state, float* grads, const float* dy, float* dx, void* ws,
                      size_t ws_bytes, int B, int training, uint64_t seed, const uint32_t* rng_salt,
                      int stage, void* stream);

/* The same backward cut into UNITS in reverse execution order (unit 0 = output conv; then per decoder block, last
 * first, preceded by the SkipConnection that follows it in the forward; bottleneck blocks; encoder blocks; last unit =
 * positional embedding + dx), so that a data-parallel caller can start the all-reduce of a gradient bucket as soon
 * as the units producing it are enqueued.  vu_model_backward_unit_ranges fills lo_hi[2u], lo_hi[2u+1] with
 * the arena range [lo, hi) of unit u's parameter gradients.  Units must be run in order, each exactly once per step;
 * any split of [0, n) into calls is equivalent to vu_model_backward(stage = 0). */
int vu_model_num_backward_units(const vu_config* cfg);
int vu_model_backward_unit_ranges(const vu_config* cfg, long long* lo_hi, int capacity);
int vu_model_backward_units(const vu_config* cfg, const float* params, const void* shadow,
                            const float* bn_state, float* grads, const float* dy, float* dx, void* ws,
                            size_t ws_bytes, int B, int training, uint64_t seed, const uint32_t* rng_salt,
                            int first_unit, int last_unit, void* stream);

/* ---- per-op entry points (used by the parity tests and by the stand-alone sub-modules) ---- */

/* patch / unpatch / downsampling / upsampling (model.py:8-53): one latent image re-tiled from
 * patch size s_in to s_out (the (B,C,im,im) image is the s = im case).  pos (fp32, output
 * layout, one sample) is added when non-NULL (PatchEncoder, model.py:84-91). */
int vu_retile(int dtype, int in_f32, int out_f32, const void* in, void* out, const float* pos,
              int B, int C, int im, int s_in, int s_out, void* stream);
/* out = retile(in) + add: the backward of a level change where a second gradient arrives in the output tiling - the gradient of
 * downsampling (model.py:40-53 run backwards) meets the one that comes through the skip connection (model.py:407-410, 420-423).  All
 * three tensors in the storage type, `add` and `out` in the s_out tiling, three distinct buffers; the sum is formed in fp32 and
 * rounded once, as a separate add would leave it. */
int vu_retile_add(int dtype, const void* in, const void* add, void* out, int B, int C, int im, int s_in, int s_out, void* stream);

/* Conv2d(C,C,3,padding='same') applied per patch (model.py:137-139,152-154) or on the whole
 * image (model.py:370,428: npatch = B, s = im). */
int vu_conv3x3_fwd(int dtype, int out_f32, const void* in, const float* w, const float* bias,
                   void* out, long long npatch, int C, int s, void* stream);
int vu_conv3x3_bwd(int dtype, int dout_f32, const void* dout, const void* in, const float* w,
                   const void* add, void* din, float* dw, float* dbias, long long npatch, int C,
                   int s, void* stream);

/* The three convolutions of a ReAttention / SkipConnection at once (model.py:137-139 qconv2d / kconv2d / vconv2d applied at
 * :152-154; SkipConnection :246-248 takes q from one tensor and k, v from another: xq != xkv): one read of the input(s),
 * no bias; and the sum of their data gradients: dxq = convT(dq) [+ convT(dk) + convT(dv) when dxkv is NULL] + add_q,
 * dxkv = convT(dk) + convT(dv) + add_kv (add_* may be NULL).  Stencil kernels (csrc/vu_conv.hip); a matrix-core form exists
 * behind VU_CONV_MM=1 (csrc/vu_conv_mm.hip: measured, not faster). */
int vu_conv3x3_qkv_fwd(int dtype, const void* xq, const void* xkv, const float* wq, const float* wk, const float* wv,
                       void* q, void* k, void* v, long long npatch, int C, int s, void* stream);
int vu_conv3x3_qkv_dgrad(int dtype, const void* dq, const void* dk, const void* dv, const float* wq, const float* wk,
                         const float* wv, const void* add_q, const void* add_kv, void* dxq, void* dxkv,
                         long long npatch, int C, int s, void* stream);
/* ... and their weight gradients (autograd of model.py:152-154): dwq += d(q)/d(wq) etc., fp32 (C, C, 3, 3).  `scratch` (optional, at
 * least 1 MiB, device memory): with it the per-workgroup partial sums are added in a fixed order (bit-reproducible; the model executor
 * always lends one), without it the sums end in float atomics. */
int vu_conv3x3_qkv_wgrad(int dtype, const void* dq, const void* dk, const void* dv, const void* xq, const void* xkv, float* dwq,
                         float* dwk, float* dwv, void* scratch, size_t scratch_bytes, long long npatch, int C, int s, void* stream);

/* ReAttention.forward / SkipConnection.forward (model.py:150-164, 244-259) on token maps
 * xq, xkv (B,N,D); prm = pointers into the arenas.  ws from vu_attn_workspace_bytes. */
typedef struct vu_attn_params {
  const float* mix_w; const float* mix_b; const float* bn_w; const float* bn_b;
  const float* wq; const float* wk; const float* wv;
  const void* proj_w;  /* storage dtype */
  const float* proj_b;
  float* run_mean; float* run_var;
  int operands;  /* 0 storage dtype, 1 OCP e4m3 (as vu_config.attn_operands) */
} vu_attn_params;
typedef struct vu_attn_grads {
  float* mix_w; float* mix_b; float* bn_w; float* bn_b; float* wq; float* wk; float* wv;
  float* proj_w; float* proj_b;
} vu_attn_grads;
size_t vu_attn_workspace_bytes(int dtype, int B, int N, int D, int H);
int vu_attn_forward(int dtype, const vu_attn_params* prm, const void* xq, const void* xkv, void* y,
                    void* map_out, void* ws, size_t ws_bytes, int B, int N, int D, int H, int C,
                    float attn_drop, float proj_drop, int training, uint64_t seed, uint64_t stream_id,
                    void* stream);
int vu_attn_backward(int dtype, const vu_attn_params* prm, const vu_attn_grads* grd, const void* xq,
                     const void* xkv, const void* dy, void* dxq, void* dxkv, void* ws, size_t ws_bytes,
                     int B, int N, int D, int H, int C, float attn_drop, float proj_drop, int training,
                     uint64_t seed, uint64_t stream_id, void* stream);

/* residual add + LayerNorm((N,D)) (model.py:193-196, 203-206); x may be NULL. */
size_t vu_layernorm_workspace_floats(int B, long long P);
int vu_add_layernorm_fwd(int dtype, const void* a, const void* x, void* z, const float* w,
                         const float* b, void* y, float* ws, float* stats, int B, long long P,
                         void* stream);
int vu_layernorm_bwd(int dtype, const void* dy, const void* z, const float* w, const float* stats,
                     float* dw, float* db, float* ws, void* dz, int B, long long P, void* stream);

/* FeedForward.forward (model.py:95-110): y = Dropout(Linear(Dropout(GELU(Linear(x))))) on (rows, D) tokens; w1 (hid,D),
 * w2 (D,hid) in the storage dtype, biases fp32.  hpre / hact (rows,hid) keep the GELU pre-activation and the (dropped)
 * activation for the backward.  vu_ff_backward accumulates dw1 (hid,D), db1, dw2 (D,hid), db2 (fp32) and writes dx;
 * scratch >= vu_ff_scratch_bytes.  Dropout sites replay from (seed, stream_id) as in vu_attn_forward. */
size_t vu_ff_scratch_bytes(int dtype, long long rows, int D, int hid);
int vu_ff_forward(int dtype, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                  void* hpre, void* hact, void* y, long long rows, int D, int hid, float linear_drop,
                  int training, uint64_t seed, uint64_t stream_id, void* stream);
int vu_ff_backward(int dtype, const void* x, const void* w1, const void* w2, const void* hpre, const void* hact,
                   const void* dy, void* dx, float* dw1, float* db1, float* dw2, float* db2, void* scratch,
                   long long rows, int D, int hid, float linear_drop, int training, uint64_t seed,
                   uint64_t stream_id, void* stream);

/* strided batched GEMM C = alpha * A * B (+bias) used for every contraction on the path;
 * strides in elements; exactly one of (sAm,sAk) and one of (sBk,sBn) must be 1. */
int vu_gemm(int dtype, int c_float, const void* A, const void* Bm, void* C, int M, int N, int K,
            long long sAm, long long sAk, long long sBk, long long sBn, long long ldc, int Z1, int Z2,
            long long sA1, long long sA2, long long sB1, long long sB2, long long sC1, long long sC2,
            float alpha, const float* bias, int accumulate, void* stream);

/* MSELoss + its gradient (run_denoising.py:80); partials: >= 1024 floats. */
int vu_mse_loss(const float* out, const float* target, float* dout, float* loss, float* partials,
                long long n, float grad_scale, void* stream);
/* AdamW over the flat arena (run_denoising.py:81); hyper = {lr,beta1,beta2,eps,weight_decay}
 * and the int step counter live in device memory. */
int vu_adamw(float* params, const float* grads, float* m, float* v, void* shadow_bf16, long long n,
             const float* hyper, int* step, float grad_scale, void* stream);
int vu_cast_bf16(const float* in, void* out, long long n, void* stream);
/* out[n] += sum over rows of in[row * ld + n], n < ncols (bias / embedding gradients: the sum over the batch). */
int vu_colsum(int dtype, const void* in, float* out, long long rows, int ncols, long long ld, void* stream);
/* In place: every element of x (dtype 0 fp32 / 1 bf16, n % 4 == 0) becomes the nearest OCP e4m3fn value (round to
 * nearest even, 3 mantissa bits, subnormal step 2^-9, saturating at +-448; NaN stays NaN) held in the same container.
 * An e4m3 value is exactly a bf16 value, so the bf16 MFMA on rounded operands forms the same products an fp8 MFMA
 * does; at this model's head dims (d <= 96) the non-scaled fp8 MFMA has the bf16 rate, so nothing is lost.
 * The conversion itself is the hardware's (v_cvt_pk_fp8_f32 / v_cvt_f32_fp8). */
int vu_round_e4m3(int dtype, void* x, long long n, void* stream);

/* Dice loss with its gradient (README.md:91-101: smooth = 1, flattened,
 * 1 - (2 sum(p t) + 1) / (sum p + sum t + 1)).  apply_sigmoid != 0: p = sigmoid(logits) (the
 * segmentation head of BASELINE config 5 - the reference has none) and dlogits is the
 * gradient w.r.t. the logits; dlogits may be NULL (loss only).  partials: >=
 * vu_dice_partials_floats() floats.  Operands 16-byte aligned. */
size_t vu_dice_partials_floats(void);
int vu_dice_loss(const float* logits, const float* target, float* dlogits, float* loss,
                 float* partials, long long n, int apply_sigmoid, float grad_scale, void* stream);
/* Per-image PSNR = 10 log10(R^2 / mean((target-out)^2)) over P elements per image
 * (vit_unet/torch/functions.py:7-19, skimage.metrics.peak_signal_noise_ratio per image);
 * psnr: B floats; partials: >= vu_psnr_partials_floats(B) floats. */
size_t vu_psnr_partials_floats(int B);
int vu_psnr(const float* target, const float* out, float* psnr, float* partials, int B, long long P,
            float data_range, void* stream);
/* Per-image mean SSIM of (B,C,H,W) float images, averaged over channels (README.md:85-89;
 * scikit-image structural_similarity defaults: uniform win x win window (7), K1 = 0.01,
 * K2 = 0.03, sample covariance, (win-1)/2 border cropped).  ssim: B floats; partials: >=
 * vu_ssim_partials_floats(...) floats. */
size_t vu_ssim_partials_floats(int B, int C, int H, int W, int win);
int vu_ssim(const float* target, const float* out, float* ssim, float* partials, int B, int C, int H,
            int W, int win, float data_range, void* stream);

/* Device-side input pipeline of the denoising runs: DenoisingDataset.__getitem__
 * (vit_unet/torch/dataset.py:52-71) + the albumentations transforms of run_denoising.py:52-59 for
 * a whole batch.  noisy / clean: (B,Hs,Ws,channels) uint8 HWC as decoded; x / y: (B,channels,im,im)
 * float32.  Steps: cv2.resize to im x im (skipped when Hs == Ws == im) -> warpAffine with the
 * per-image INVERSE 2x3 matrices inv_affine (B x 6 doubles, device memory; NULL = validation
 * transform, no warp; bilinear for noisy, nearest for clean, constant border 0) -> Normalize
 * ((v - 255 mean) / (255 std)) on noisy only -> /255 on both -> CHW.  A pair may be omitted
 * (noisy == x == NULL or clean == y == NULL).  scratch: >= vu_denoise_prepare_scratch_bytes. */
size_t vu_denoise_prepare_scratch_bytes(int B, int im, int channels);
int vu_denoise_prepare(const uint8_t* noisy, const uint8_t* clean, float* x, float* y,
                       uint8_t* scratch, size_t scratch_bytes, const double* inv_affine, int B,
                       int Hs, int Ws, int channels, int im, float mean, float std, void* stream);

/* Device-side input pipeline for SegmentationDataset items (vit_unet/torch/dataset.py:18-38): the
 * reference reads a DICOM slice (pixel_array, 16-bit) and one NIfTI mask plane on the host and
 * leaves scaling/augmentation to the caller's `augments`.  Here, for a whole batch: image
 * (B,Hs,Ws) int16 and mask (B,Hs,Ws) uint8 labels -> cv2.resize to oh x ow (bilinear, float
 * coefficients, for the slice; nearest for the mask; skipped when sizes match) -> optional
 * warpAffine with per-image INVERSE 2x3 matrices (B x 6 doubles, device; NULL = no warp;
 * bilinear / nearest, border 0) -> x = clip((v - lo) / (hi - lo), 0, 1), y = label * (1 - ls) +
 * ls / 2 (the dataset's `ls` argument); x / y: (B,1,oh,ow) float32.  Either pair may be omitted
 * (is_test).  scratch: >= vu_seg_prepare_scratch_bytes, 2-byte aligned. */
size_t vu_seg_prepare_scratch_bytes(int B, int oh, int ow);
int vu_seg_prepare(const int16_t* image, const uint8_t* mask, float* x, float* y, uint8_t* scratch,
                   size_t scratch_bytes, const double* inv_affine, int B, int Hs, int Ws, int oh,
                   int ow, float lo, float hi, float ls, void* stream);

/* Whole-image restoration (csrc/vu_tile.hip; no reference counterpart: the reference only ever resizes to im_size): sliding-window
 * inference.  An H x W image is covered by T x T windows (T = im_size) overlapping by `overlap` pixels, 0 <= overlap <= T / 2, stride
 * S = T - overlap.  Per axis of length L: L <= T gives one window at 0 whose T - L missing rows / columns are reflected without
 * repeating the edge (m = 2 (L - 1), k = i mod m, source k if k < L else m - k; L == 1 replicates) and of whose output only the first
 * L rows / columns are used; L > T gives n = ceil((L - T) / S) + 1 windows at min(i S, L - T) - the last one shifted inwards, not
 * padded.  The 2-D plan is the outer product, row-major (window t = ty * nx + tx); a pixel lies in at most 3 windows per axis.
 *   plan_count   ny, nx of the plan (host pointers)            plan_axis   origins[0 .. n) of one axis (host), returns n
 * Both are host code (no GPU call).
 *   gather_u8    img (H,W,C) uint8 HWC as decoded -> windows [t0, t0 + n) of the plan as tiles (n,C,T,T) float32 under the
 *                validation transform of the input pipeline (what the denoise-prepare call above gives `noisy` without a warp)
 *   gather_f32   img (C,H,W) float32 -> the same windows, values copied unchanged
 *   blend        tiles (ny nx,C,T,T) float32, the outputs for the WHOLE plan -> out_f32 (C,H,W) and / or out_u8 (H,W,C) (either may
 *                be NULL): per pixel acc += w v, ws += w over the covering windows in ascending plan order, out = acc / ws, all
 *                float32, w = wy wx with w(i) = min(i + 1, T - i, overlap + 1) / (overlap + 1); out_u8 = clamp(floor(255 out + 0.5),
 *                0, 255).  A gather (no atomics): bit-identical on every run.  The outputs must not alias `tiles`.
 * 1 <= C <= 4.  T % 4 == 0 and 16-byte aligned buffers take 16-byte accesses; anything else is handled by scalar ones. */
int vu_tile_plan_count(int H, int W, int T, int overlap, int* ny, int* nx);
int vu_tile_plan_axis(int L, int T, int overlap, int* origins, int capacity);
int vu_tile_gather_u8(const uint8_t* img, float* tiles, int H, int W, int C, int T, int overlap, int t0, int n, float mean,
                      float std, void* stream);
int vu_tile_gather_f32(const float* img, float* tiles, int H, int W, int C, int T, int overlap, int t0, int n, void* stream);
int vu_tile_blend(const float* tiles, float* out_f32, uint8_t* out_u8, int H, int W, int C, int T, int overlap, void* stream);

/* Whole-slice / volume segmentation (csrc/vu_segtile.hip; no reference counterpart): the same sliding-window inference for the
 * 1-channel segmentation configuration.  vol is (D,H,W) int16 (one slice: D = 1); every slice has the plan above (nt = ny nx windows)
 * and windows are numbered over the whole volume, g = z nt + t.
 *   gather_i16   windows [g0, g0 + n) (the range may cross slice boundaries) as tiles (n,1,T,T) float32: the crop, inward shift and
 *                reflection of gather_f32, values under the intensity window of the seg-prepare call above,
 *                x = clip((v - lo) / (hi - lo), 0, 1) (hi - lo in float32; bit for bit what seg-prepare gives the same pixels without
 *                resize and warp).  Refused: hi <= lo, null pointers, a range outside D nt.
 *   seg_blend    tiles (nz nt,1,T,T) float32, the model outputs (logits) for the WHOLE plan of nz consecutive slices.  Per pixel z is the
 *                blended logit with exactly the arithmetic of vu_tile_blend at C = 1 (bit-identical to its out_f32, slice by slice);
 *                  logits (nz,H,W) float32 = z        mask (nz,H,W) uint8 = z >= zthr ? 1 : 0
 *                  counts (nz,3) uint64 per slice: mask pixels, truth pixels, pixels where both are set; a truth pixel is
 *                  truth != 0 when label < 0 and truth == label when 0 <= label <= 255 (truth: (nz,H,W) uint8).
 *                logits, mask and counts may each be NULL, not all three; counts needs truth (refused otherwise; truth without counts
 *                is not read) and scratch >= vu_seg_blend_scratch_bytes(nz, H, W), 4-byte aligned (per-block partial counts, summed
 *                per slice in a fixed order by a second launch: exact integers whatever the launch geometry, no atomics).  The
 *                outputs must not alias `tiles`.  A probability threshold thr in (0,1) is zthr = log(thr / (1 - thr)) (0 for 0.5);
 *                the probability itself is not an output (sigmoid of `logits`).
 * T % 4 == 0 and aligned buffers take 8-byte int16 loads, 16-byte float and 4-byte mask / truth accesses; anything else is scalar. */
int vu_tile_gather_i16(const int16_t* vol, float* tiles, int D, int H, int W, int T, int overlap, long long g0, int n, float lo,
                       float hi, void* stream);
size_t vu_seg_blend_scratch_bytes(int nz, int H, int W);
int vu_seg_blend(const float* tiles, const uint8_t* truth, float* logits, uint8_t* mask, unsigned long long* counts, void* scratch,
                 size_t scratch_bytes, int nz, int H, int W, int T, int overlap, float zthr, int label, void* stream);

/* Native-resolution training patches and the self-ensemble (csrc/vu_patch.hip; no reference counterpart).  Both rest on the dihedral
 * transforms of a T x T window: op in 0 .. 7, k = op & 3 counter-clockwise quarter turns applied after a left-right flip when op & 4,
 *   D_op(p) = np.rot90(np.fliplr(p) if op & 4 else p, k = op & 3),   m = flipped or plain p with m[a,b] = p[a, T-1-b]:
 *   k = 0: out[i,j] = m[i,j]   k = 1: m[j, T-1-i]   k = 2: m[T-1-i, T-1-j]   k = 3: m[T-1-j, i].
 *   dihedral_inverse   the op that undoes `op`: op itself when op & 4, else (4 - op) & 3; negative outside 0 .. 7.  Host code, no GPU call.
 *   patch_pairs_u8     ONE image pair, noisy / clean (H,W,C) uint8 HWC as decoded; crops: (n,3) int32 (y0, x0, op) in DEVICE memory.
 *                      x[i] = D_op(noisy[y0:y0+T, x0:x0+T]) under the validation transform of the input pipeline (Normalize, /255),
 *                      y[i] = the same cut and op of clean, /255 only; both (n,C,T,T) float32: what the denoise-prepare call above
 *                      gives each side without a warp, bit for bit.  A pair may be omitted (noisy == x == NULL or clean == y == NULL).
 *                      1 <= C <= 4, H >= T and W >= T (an image smaller than a patch is refused, not reflected), std > 0, n >= 1.
 *                      The host cannot read the table, so the KERNEL CLAMPS it: y0 to [0, H-T], x0 to [0, W-T], op to op & 7 - no
 *                      table content makes it read outside the image (callers that want an error check the table before uploading).
 *   dihedral_f32       src, dst (n,C,T,T) float32, one op for the call: v = D_op(src plane), r = accumulate ? dst + v : v,
 *                      dst = scale == 1 ? r : r * scale, every operation rounded once in float32.  dst must not overlap src.
 * No atomics: bit-identical on every run.  Any T; T % 4 == 0 and 16-byte aligned buffers take 16-byte accesses, anything else scalar. */
int vu_dihedral_inverse(int op);
int vu_patch_pairs_u8(const uint8_t* noisy, const uint8_t* clean, float* x, float* y, int H, int W, int C, int T, const int* crops,
                      int n, float mean, float std, void* stream);
int vu_dihedral_f32(const float* src, float* dst, int n, int C, int T, int op, int accumulate, float scale, void* stream);

/* Native-resolution segmentation training patches with foreground sampling (csrc/vu_segpatch.hip; no reference counterpart): the
 * int16 / label-mask twin of the patch call above.  vol is (D,H,W) int16, mask (D,H,W) uint8 (one slice: D = 1); a crop is a T x T
 * window of ONE slice.  A foreground pixel is mask != 0 when label < 0 and mask == label when 0 <= label <= 255 (the truth rule of the
 * seg-blend call above).  Everywhere: D H W < 2^32, label <= 255.  All index arithmetic is integer:
 *   fg_index     index (D H + 1) uint32: index[r] = number of foreground pixels in rows [0, r) of the volume taken as D H rows of W
 *                pixels (row q = slice q / H, line q % H), so index[0] = 0 and index[D H] = total.  scratch >= vu_fg_index_bytes(D, H),
 *                4-byte aligned (row counts and the chunk totals of a scan with a fixed geometry: integers, no atomics, the same bits
 *                on every run).  W % 4 == 0 and a 4-byte aligned mask take 4-byte mask loads, anything else byte loads.
 *   draw         rnd (n,4) uint32 and crops (n,4) int32 (z, y0, x0, op), both in DEVICE memory and 16-byte aligned; index as above
 *                (of the same mask and label).  T <= H, W <= 65535.  With total = index[D H], per crop i:
 *                  foreground crop, when rnd[i,0] < fg_thresh and total > 0:
 *                    r = (uint64(rnd[i,1]) * total) >> 32          the r-th foreground pixel in raster order over the volume:
 *                    q = the row with index[q] <= r < index[q+1],   z = q / H,  y = q % H,
 *                    x = the column of the (r - index[q])-th foreground pixel of that row (counted from 0)
 *                    oy = ((rnd[i,2] >> 16) * T) >> 16,            ox = ((rnd[i,2] & 0xffff) * T) >> 16
 *                    y0 = clamp(y - oy, 0, H - T),                 x0 = clamp(x - ox, 0, W - T)
 *                  (so the pixel lies inside the crop); otherwise:
 *                    z  = (uint64(rnd[i,1]) * D) >> 32
 *                    y0 = ((rnd[i,2] >> 16) * (H - T + 1)) >> 16,  x0 = ((rnd[i,2] & 0xffff) * (W - T + 1)) >> 16
 *                  in both cases op = rnd[i,3] & 7.
 *                fg_thresh = 0 never samples foreground; the total is read on the device: no host synchronisation.  An index that
 *                does not belong to the mask cannot make the kernel read outside either buffer (the search is bounded, the walk of a
 *                row ends at x = W - 1).
 *   patch_pairs_i16  crops (n,4) int32 (z, y0, x0, op) in DEVICE memory, 16-byte aligned.  With p = the crop [z, y0:y0+T, x0:x0+T]:
 *                  x[i] = D_op(clip((vol p - lo) / (hi - lo), 0, 1))   the intensity window of the seg-prepare call (hi - lo in float32,
 *                         every operation rounded once): the bits seg-prepare and gather_i16 give the same pixels
 *                  y[i] = D_op(t * (1 - ls) + ls / 2),  t = 1 on a foreground pixel of mask p, else 0 (float32: keep = 1 - ls and
 *                         floor = 0.5 ls are formed first, then one product and one sum, as seg-prepare does; for a {0,1} mask and
 *                         label < 0 bit for bit what seg-prepare gives without resize and warp)
 *                both (n,1,T,T) float32, D_op as defined above.  A pair may be omitted (vol == x == NULL or mask == y == NULL).
 *                The KERNEL CLAMPS the table: z to [0, D-1], y0 to [0, H-T], x0 to [0, W-T], op to op & 7.
 * Refused before any launch: null or inconsistent pointers, hi <= lo, ls outside [0,1), label > 255, H < T or W < T, n < 1, T < 1,
 * the size limits above, a short or misaligned scratch.  T % 4 == 0 and 16-byte aligned outputs take 16-byte stores, anything else
 * scalar ones. */
size_t vu_fg_index_bytes(int D, int H);
int vu_fg_index(const uint8_t* mask, uint32_t* index, void* scratch, size_t scratch_bytes, int D, int H, int W, int label,
                void* stream);
int vu_segpatch_draw(const uint8_t* mask, const uint32_t* index, const uint32_t* rnd, int* crops, int n, int D, int H, int W, int T,
                     uint32_t fg_thresh, int label, void* stream);
int vu_patch_pairs_i16(const int16_t* vol, const uint8_t* mask, float* x, float* y, int D, int H, int W, int T, const int* crops, int n,
                       float lo, float hi, float ls, int label, void* stream);

/* Segmentation mask clean-up: connected components on the device (csrc/vu_segclean.hip; no reference counterpart).  mask is
 * (D,H,W) uint8 (one slice: D = 1), a pixel's linear index is i = (z H + y) W + x, D H W <= 2^31 - 1.
 * Units and connectivity: conn 4 or 8 labels every slice on its own (U = D units; 4: edge neighbours, 8: edge and corner
 * neighbours); conn 6 or 26 labels the volume as one unit (U = 1; 6: face neighbours, 26: face, edge and corner neighbours) and
 * needs D >= 2 - a single slice has no 3-D connectivity and takes 4 or 8.
 *   cc_tile      the tile height and width of the labelling kernel (16 x 64), so that a test can put structures on tile borders.
 *   cc_label     fg = 1 labels the pixels with mask != 0, fg = 0 those with mask == 0 (the background, for hole filling).
 *                  labels (D,H,W) int32: -1 on an unlabelled pixel, else the smallest linear index of the pixel's component
 *                  sizes  (D,H,W) uint32, may be NULL: sizes[r] = pixels of the component whose smallest index is r, 0 elsewhere
 *                scratch >= vu_cc_scratch_bytes(D, H, W), 4-byte aligned; after the call its first uint32 is the overflow word
 *                (below; 0 on every input the bounds cover).  mask, labels, sizes and scratch must not overlap.
 *   seg_clean    the steps, in this fixed order:
 *                  1. label the foreground (mask != 0) with conn;
 *                  2. drop the components with size < min_size;
 *                  3. keep_largest: keep only the unit's largest remaining component, ties to the smallest root index; a unit with
 *                     nothing left stays empty;
 *                  4. fill_holes: label the background of that result with the dual connectivity (8 -> 4, 4 -> 8, 26 -> 6, 6 -> 26)
 *                     and set to 1 every background component that touches no border of its unit: the four slice edges for a
 *                     per-slice unit, the six volume faces for a volume unit.
 *                out (D,H,W) uint8 holds 0 or 1; it may be `mask` itself (any other overlap is refused).
 *                counts (D,3) uint64, ALWAYS per slice: mask pixels, truth pixels, common pixels of the cleaned mask, with the truth
 *                  rule and `label` of the seg-blend call above (truth != 0 when label < 0, truth == label when 0 <= label <= 255)
 *                  and its two-stage fixed-order sum.  counts and truth are given together or both NULL.
 *                stats (U,4) int64, may be NULL: components found by step 1, components kept after step 3, size of the largest
 *                  component step 1 found, overflow.
 *                scratch >= vu_seg_clean_scratch_bytes(D, H, W), 16-byte aligned (labels, sizes, per-unit accumulators, partial counts).
 * Overflow: every data-dependent loop of the labelling (find, union retry) has an iteration cap derived from a bound - the 1024
 * pixels of a tile inside a tile, 1 + tiles of the unit x 512 local components across tiles; a loop that reaches its cap sets the
 * overflow word and leaves, so a wrong bound shows as a non-zero word and a wrong label, never as a hang.
 * Reproducibility: the labelling unites with integer atomicMin, sizes and border flags are integer atomicAdd / atomicOr (summed per
 * tile and local component in LDS first: one global add per tile and local component), the selection is a 64-bit integer
 * atomicMax.  Integer sums, minima, maxima and ors do not depend on the order of arrival, so labels, sizes, out, counts and stats
 * are fully defined by the input: the same bits on every run, whatever the launch order.
 * Refused before any launch (VU_EINVAL): conn outside {4, 8, 6, 26}; conn 6 or 26 with D = 1; D H W > 2^31 - 1 or an empty
 * volume; fg outside {0, 1}; keep_largest or fill_holes outside {0, 1}; label > 255; null mask / labels / out / scratch; a short or
 * misaligned scratch; truth without counts or counts without truth; overlapping buffers.  W % 4 == 0 and aligned buffers take
 * 4-byte mask / out / truth and 16-byte label accesses, anything else scalar ones. */
int vu_cc_tile(int* th, int* tw);
size_t vu_cc_scratch_bytes(int D, int H, int W);
int vu_cc_label(const uint8_t* mask, int32_t* labels, uint32_t* sizes, void* scratch, size_t scratch_bytes, int D, int H, int W,
                int conn, int fg, void* stream);
size_t vu_seg_clean_scratch_bytes(int D, int H, int W);
int vu_seg_clean(const uint8_t* mask, const uint8_t* truth, uint8_t* out, unsigned long long* counts, long long* stats, void* scratch,
                 size_t scratch_bytes, int D, int H, int W, int conn, unsigned min_size, int keep_largest, int fill_holes, int label,
                 void* stream);

/* Surface-distance metrics for segmentation (csrc/vu_segdist.hip; no reference counterpart): an exact Euclidean distance transform,
 * the surface of a mask, and the integers the Hausdorff distance, its percentiles, the average symmetric surface distance and the
 * surface Dice are made of.  mask is (D,H,W) uint8, D H W <= 2^31 - 1.
 * Units: dims 2 treats every slice as a unit (U = D), dims 3 the volume as one unit (U = 1; refused for D = 1, as conn 6 / 26 above).
 * Spacing: three positive integers (sz, sy, sx) in a unit the caller chooses (tenths of a millimetre, say).  The squared distance
 * between two pixels is (sz dz)^2 + (sy dy)^2 + (sx dx)^2, an integer; dz = 0 for dims 2.  A call is refused when
 * (sz (D-1))^2 + (sy (H-1))^2 + (sx (W-1))^2 > 2^31 - 1 (without the sz term for dims 2): every intermediate then fits in 32 bits and
 * 0xffffffff is free to mean "no site".  The truth rule and `label` are those of the seg-blend call above (truth != 0 when label < 0,
 * truth == label when 0 <= label <= 255); a prediction pixel is mask != 0.
 *   edt_sq        fg = 1: the sites are the pixels with mask != 0; fg = 0: those with mask == 0.
 *                   dist2 (D,H,W) uint32 = the minimum squared distance to a site of the same unit: 0 on a site, 0xffffffff
 *                   everywhere in a unit without a site.  The exact minimum (a separable lower-envelope transform, no chamfer or
 *                   jump-flooding approximation).  scratch >= vu_edt_scratch_bytes(D, H, W, dims), 4-byte aligned.
 *   mask_surface  surf (D,H,W) uint8 = 1 on a foreground pixel with at least one of its 4 (dims 2) or 6 (dims 3) axis neighbours in the
 *                   background or outside the unit, else 0 - a foreground pixel on the edge of its unit is surface: the rule
 *                   input ^ binary_erosion(input) of MedPy / SciPy.  Foreground: mask != 0 when label < 0, mask == label otherwise.
 *   surface_dist  P = the surface of pred != 0, T = the surface of the truth under `label`; d(P->T) = the multiset of dist2-to-T over
 *                 the pixels of P, d(T->P) its mirror.  Per unit u:
 *                   stats (U,6) uint64: |P|, |T|, max d(P->T), max d(T->P), elements <= tol2 of d(P->T), of d(T->P)
 *                   sums  (U,2) float64: the sum of sqrt((double) d2) over d(P->T), over d(T->P): per-block partials in a fixed
 *                     geometry (1024 pixels a block), added per unit in a fixed order by a second launch; no floating-point atomics
 *                   order (U,3,2) uint32: order statistics of set 0 = d(P->T), 1 = d(T->P), 2 = their union as multisets.  With n the
 *                     set's size, lo = (qnum (n-1)) / qden in 64-bit integer division and hi = min(lo + 1, n - 1):
 *                     order[u,s,0] = the lo-th smallest element counted from 0, order[u,s,1] = the hi-th - the two neighbours
 *                     numpy.percentile(..., method="linear") interpolates between for q = 100 qnum / qden.  Found by radix select
 *                     (integer histograms, 8 bits a pass) over the device-resident distances.  0 <= qnum <= qden <= 1000000.
 *                   dist_pt, dist_tp (D,H,W) uint32, each may be NULL: the two distance maps, to T and to P.
 *                 A unit in which P or T is empty: stats[0..1] are the counts, the maximum of the non-empty direction is 0xffffffff and
 *                 that of the empty one 0, both "within" counts are 0, sums are 0 and all order entries 0xffffffff.
 *                 pred may be `truth` itself.  scratch >= vu_surface_dist_scratch_bytes(D, H, W, dims), 16-byte aligned (two surfaces,
 *                 two maps, the transform's scratch, per-block partials, selection state and histograms).
 *   segdist_geometry  the lengths the kernels treat specially, so that a test can put sites on either side of each: line_piece = the
 *                 piece of a y / z line one workgroup holds in LDS (128; a longer line is covered piece by piece), lines_per_group = the
 *                 neighbouring lines one workgroup owns (64), row_chunk = the pixels of a row one wave scans per trip (256).
 * Reproducibility: integer minima, maxima, sums and histogram counts plus the fixed-order float64 sum: the same bits on every run.
 * Refused before any launch (VU_EINVAL): dims outside {2, 3}; dims 3 with D = 1; fg outside {0, 1}; a spacing < 1 or the bound above
 * exceeded; D H W > 2^31 - 1 or an empty volume; label > 255; qden < 1 or > 1000000, qnum > qden; null mask / dist2 / surf / pred /
 * truth / stats / sums / order / scratch; a short or misaligned scratch; overlapping buffers.  No size is refused because a line does
 * not fit in LDS.  W % 4 == 0 and aligned buffers take 4-byte mask loads and 16-byte distance accesses in the row pass. */
int vu_segdist_geometry(int* line_piece, int* lines_per_group, int* row_chunk);
size_t vu_edt_scratch_bytes(int D, int H, int W, int dims);
int vu_edt_sq(const uint8_t* mask, uint32_t* dist2, void* scratch, size_t scratch_bytes, int D, int H, int W, int dims, int fg, int sz,
              int sy, int sx, void* stream);
int vu_mask_surface(const uint8_t* mask, uint8_t* surf, int D, int H, int W, int dims, int label, void* stream);
size_t vu_surface_dist_scratch_bytes(int D, int H, int W, int dims);
int vu_surface_dist(const uint8_t* pred, const uint8_t* truth, unsigned long long* stats, double* sums, uint32_t* order,
                    uint32_t* dist_pt, uint32_t* dist_tp, void* scratch, size_t scratch_bytes, int D, int H, int W, int dims, int sz,
                    int sy, int sx, int label, uint32_t tol2, uint32_t qnum, uint32_t qden, void* stream);

/* ---- Volume resampling to a working spacing and back (csrc/vu_resample.hip; Python: segment.VolumeResampler) ----
 * A (Di,Hi,Wi) volume becomes (Do,Ho,Wo).  Resampling is driven by the two shapes alone: an axis of n_in samples becomes n_out
 * samples with half-pixel centres, output i sits at ((2 i + 1) n_in - n_out) / (2 n_out) of the input, edges replicated.  A spacing
 * exists only in Python, where it chooses n_out.  All table arithmetic is exact integer, Q = 2^15 ("//" and "%" floor, on
 * non-negative operands only):
 *   linear table of an axis, (i0[i], w[i]):  num = (2 i + 1) n_in - n_out, den = 2 n_out.  num <= 0 gives (0, 0).  Otherwise
 *       i0 = num // den, r = num % den, w = (2 Q r + den) // (2 den); i0 >= n_in - 1 gives (n_in - 1, 0).  The second tap is
 *       i1 = min(i0 + 1, n_in - 1); 0 <= w <= Q; n_out == n_in gives the identity (i, 0).
 *   nearest table, src[i] = ((2 i + 1) n_in) // (2 n_out), always in 0 .. n_in - 1.
 *   resample_i16         trilinear, staged x, then y, then z.  A stage is (v0 (Q - w) + v1 w + Q / 2) >> 15 with an arithmetic shift
 *                        (round half up); its result is again an int16 value and enters the next stage; |v| <= 2^15 keeps every
 *                        intermediate inside int32.  The kernel does the 4 x-stages, 2 y-stages and 1 z-stage of an output in
 *                        registers: the same bits as three passes.
 *   resample_f32         the same tables and order on float32 (logits): wf = (float) w / Q (exact), a stage is a + (b - a) * wf with the
 *                        subtraction, the product and the sum each rounded to float32 on its own (no fused multiply-add), also where
 *                        w = 0.  out (Do,Ho,Wo) float32; mask uint8 = value >= zthr ? 1 : 0; counts (Do,3) uint64 per output slice:
 *                        mask pixels, truth pixels, pixels where both are set, truth (Do,Ho,Wo) uint8 under the label rule of
 *                        vu_seg_blend (truth != 0 when label < 0, truth == label when 0 .. 255).  out, mask and counts may each be
 *                        NULL, not all three; counts need truth and scratch >= vu_resample_f32_scratch_bytes(Do, Ho, Wo), 4-byte
 *                        aligned: per-workgroup partial counts, summed per slice in a fixed order by a second launch (no atomics).
 *   resample_u8_nearest  out[z,y,x] = in[src_z[z], src_y[y], src_x[x]] for label masks of any values: no value is invented.
 *   resample_axis_linear / _nearest   the tables themselves, host code without a GPU call; `capacity` >= n_out entries; return n_out.
 *   resample_geometry    the tile of outputs one workgroup owns (128 x 8 x 1), so that a test can put shapes on either side of it.
 * Integer results are exact and every output is bit-identical from run to run.  Refused before any launch (VU_EINVAL): a null
 * pointer; a dimension < 1; more than 2^31 - 1 elements on either side; an output that overlaps an input (or, in resample_f32,
 * another output or the scratch); label > 255; a zthr that is not a number; a short or misaligned scratch; counts not 8-byte aligned.
 * Wo % 4 == 0 with an aligned output takes 8-byte (int16), 16-byte (float32) and 4-byte (uint8) stores, anything else scalar ones.
 * No anti-alias filter runs before a strong reduction (nnU-Net's resampling has none either). */
int vu_resample_axis_linear(int n_in, int n_out, int* i0, int* w, int capacity);
int vu_resample_axis_nearest(int n_in, int n_out, int* src, int capacity);
int vu_resample_geometry(int* tile_x, int* tile_y, int* tile_z);
int vu_resample_i16(const int16_t* in, int16_t* out, int Di, int Hi, int Wi, int Do, int Ho, int Wo, void* stream);
int vu_resample_u8_nearest(const uint8_t* in, uint8_t* out, int Di, int Hi, int Wi, int Do, int Ho, int Wo, void* stream);
size_t vu_resample_f32_scratch_bytes(int Do, int Ho, int Wo);
int vu_resample_f32(const float* in, const uint8_t* truth, float* out, uint8_t* mask, unsigned long long* counts, void* scratch,
                    size_t scratch_bytes, int Di, int Hi, int Wi, int Do, int Ho, int Wo, float zthr, int label, void* stream);

/* ---- Per-volume intensity statistics (csrc/vu_intensity.hip; Python: segment.IntensityNormalizer) ----
 * The exact histogram of an int16 volume under a voxel selection, the bounding box of the selected voxels, and the integers a
 * per-volume intensity window is made of.  No float arithmetic anywhere; integer atomics only, whose result does not depend on
 * order: every output is the same bits on every run.
 *   intensity_hist   vol (D,H,W) int16, D H W < 2^32.  hist: 65536 uint32 in device memory; afterwards hist[b] is the number of
 *                    selected voxels with value b - 32768.  The call clears hist itself (stale contents do not matter).  select:
 *                      0  every voxel
 *                      1  voxels with v > floor (strict; the MR "non-air" rule is floor = 0; any int is accepted)
 *                      2  the foreground voxels of mask (D,H,W) uint8 under the label rule of vu_seg_blend: mask != 0 when
 *                         label < 0, mask == label when 0 .. 255.  mask is read for select 2 only.
 *                    bbox: NULL, or 6 int32 in device memory (z0, z1, y0, y1, x0, x1), the inclusive extent of the selected
 *                    voxels; (D, -1, H, -1, W, -1) when none is selected.  Two launches: one clears hist and bbox, one counts.
 *                    A vol that is 16-byte aligned (and, for select 2, a mask that is 8-byte aligned) is read 8 voxels per lane,
 *                    anything else by scalar loads; the last partial chunk always by scalar loads.
 *   intensity_rank   the rank arithmetic alone, host code without a GPU call: for 1 <= N < 2^32, 0 <= pn <= pd, 1 <= pd <= 10^6,
 *                    k = ((N - 1) pn) div pd and r = ((N - 1) pn) mod pd; the product is < 2^52.
 *   intensity_stats  one launch of a fixed geometry over hist.  stats: (8 + 4 nq) int64 in device memory, 0 <= nq <= 4:
 *                      [0] N = the number of selected voxels, [1] min, [2] max, [3] sum of v, [4] sum of v^2 (< 2^62), [5..7] 0
 *                      [8 + 4 j ..] for quantile j = pn[j] / pd[j] (a fraction of 1): k, r as intensity_rank gives them for N, the
 *                      k-th smallest selected value (counted from 0) and the min(k + 1, N - 1)-th smallest.
 *                    With N = 0 every entry but [0] is 0.  pn and pd are HOST arrays of nq entries, read during the call.  N is
 *                    read on the device: the call does not wait for the device.
 *   intensity_geometry   what the histogram kernel was built with: values lds_base .. lds_base + lds_bins - 1 are counted in a
 *                    private LDS sub-histogram per workgroup (lds_bins = 0: the direct measurement form), everything else by
 *                    global atomics; a workgroup takes voxels_per_block voxels per step of its grid-stride loop.
 * Refused before any launch (VU_EINVAL): a null vol, hist or stats (and pn / pd with nq > 0, k / r, a geometry pointer); select
 * outside 0 .. 2; select 2 without a mask; label > 255; a dimension < 1 or D H W >= 2^32; hist or bbox not 4-byte aligned, stats
 * not 8-byte aligned; nq outside 0 .. 4; N, pn or pd outside the ranges of intensity_rank. */
int vu_intensity_geometry(int* lds_base, int* lds_bins, int* voxels_per_block);
int vu_intensity_hist(const int16_t* vol, const uint8_t* mask, uint32_t* hist, int32_t* bbox, int D, int H, int W, int select, int floor,
                      int label, void* stream);
int vu_intensity_rank(unsigned long long N, unsigned pn, unsigned pd, unsigned long long* k, unsigned* r);
int vu_intensity_stats(const uint32_t* hist, const unsigned* pn, const unsigned* pd, int nq, long long* stats, void* stream);

/* ---- ops of the reference's Keras re-implementation (csrc/vu_tfops.hip).  Not on the benchmarked path.
 * n % 4 == 0 everywhere; dropout masks replay from (seed, stream_id) with element index = linear index (vu_dropout) or
 * row * ld + j (softmax rows), as every other dropout site of this library. ---- */
/* out = a + b: the input residual Y = X + unpatch(...) of /root/reference/vit_unet/tf/model.py:208 */
int vu_add(int dtype, const void* a, const void* b, void* out, long long n, void* stream);
/* out = dropout_p(in) (tf/functions.py:176,179 FeedForward.Drop1 / Drop2); the backward is the same call on the gradient */
int vu_dropout(int dtype, const void* in, void* out, long long n, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* exact (erf) GELU and its backward dx = dy * gelu'(x) (tf.keras.activations.gelu, tf/functions.py:175,178) */
int vu_gelu_fwd(int dtype, const void* x, void* y, long long n, void* stream);
int vu_gelu_bwd(int dtype, const void* x, const void* dy, void* dx, long long n, void* stream);
/* Resampling 'max' (mode 0) / 'avg' (mode 1), tf/functions.py:101-124, pool_size 4: (B,N,P) -> (B,N/4,P),
 * y[b, w + s N/8, :] = pool of x[b, 8 w + 2 s + {0,1,4,5}, :] (+ pos[m, :] if pos != NULL: the layer's position embedding). */
int vu_token_pool4_fwd(int dtype, int mode, const void* x, const float* pos, void* y, int B, int N, int P, void* stream);
int vu_token_pool4_bwd(int dtype, int mode, const void* x, const void* dy, void* dx, int B, int N, int P, void* stream);
/* Keras MultiHeadAttention probabilities (tf/functions.py:288-293): p = softmax(scale * s) over the n keys of each of `rows`
 * rows (leading dimension ld), pd = dropout(p).  Backward: ds = scale * p * (g - sum_k p g), g = mask / keep * dpd. */
int vu_softmax_rows_fwd(int dtype, const void* s, void* p, void* pd, long long rows, int n, int ld, float scale, float p_drop,
                        uint64_t seed, uint64_t stream_id, void* stream);
int vu_softmax_rows_bwd(int dtype, const void* p, const void* dpd, void* ds, long long rows, int n, int ld, float scale,
                        float p_drop, uint64_t seed, uint64_t stream_id, void* stream);
/* vu_add_layernorm_fwd with the epsilon as an argument (Keras LayerNormalization: 1e-3, per token: B = rows, P = features) */
int vu_add_layernorm_fwd_eps(int dtype, const void* a, const void* x, void* z, const float* w, const float* b, void* y,
                             float* ws, float* stats, int B, long long P, float eps, void* stream);

/* Which form the re-attention runs in: PROCESS-GLOBAL test / experiment setting (the two forms draw different dropout
 * masks, so a forward and its backward - and a workspace carved for them - must see the same value: set it between
 * steps, never between a forward and its backward).
 *   flash    -1: model path per level by the fill rule (recompute form when the launch fills the chip), stand-alone
 *                op materialised (default);  0: never the recompute form;  1: the recompute form wherever covered
 *   centered  1: the stand-alone op uses the model path's centred-map form when the map itself is not asked for
 * Initial values: the environment variables VU_ATTN_FLASH (0 / 1) and VU_ATTN_CENTERED, read once. */
int vu_set_attn_form(int flash, int centered);
/* Recompute form only: how many waves of a workgroup share one 16-row tile and split the streamed keys / queries between them
 * (csrc/vu_flash.hip): 0 = the default (by launch size: 1, or 3 where the unsplit sweeps would leave one wave per SIMD), 1 = unsplit,
 * 2 = wave pairs in 4-wave workgroups, 3 = wave pairs in 8-wave workgroups (the Base / Large level-2 shape).  Process-level, for
 * tests and measurements; results differ between the forms by the order of the fp32 sums only. */
int vu_set_flash_key_split(int ks);
/* Recompute form, 8 heads: probability cache (csrc/vu_flash.hip "probability cache").  1: the training forward's moments sweep stores
 * the packed sign-tagged bf16 probabilities of every 16 x 16 tile (B h N^2 2 bytes per attention module, part of the workspace) and
 * the apply / dq / dk / dv sweeps stream them instead of rebuilding logits -> exp2 -> mask -> pack; 0: every sweep recomputes (the
 * round 2 - 4 form); -1: the build's default.  Results are bit-identical either way.  Process-level like vu_set_attn_form: it changes
 * vu_model_workspace_bytes / vu_attn_workspace_bytes, so set it before sizing a workspace, never between a forward and its backward.
 * Initial value: VU_FLASH_PCACHE (0 / 1), read once. */
int vu_set_flash_pcache(int on);
/* Byte budget of ONE model workspace for those caches (sum over the attention modules): modules get a cache in execution order while
 * the sum fits, the others recompute (bit-identical).  Default 96 GiB; initial value VU_FLASH_PCACHE_BUDGET_MB, read once.  Same rule
 * as vu_set_flash_pcache: set it before sizing a workspace, never between a forward and its backward. */
int vu_set_flash_pcache_budget(unsigned long long bytes);
/* Weight-gradient tails (csrc/vu_gemm.h: vu_defred).  1 (default): inside vu_model_backward / _backward_units the fixed-order sums over
 * per-workgroup partial rows that end the q / k / v convolutions' weight gradients and the head-mix gradients of the materialised map
 * backward are queued and run as ONE launch at the end of the call (before anything outside it reads the gradients); 0: every kernel
 * launches its own reduce at once.  Same sums in the same order: bit-identical gradients.  Initial value VU_DEFER_RED, read once. */
int vu_set_deferred_reductions(int on);

/* Data-parallel gradient exchange over RCCL (csrc/vu_dp.cpp).  The reference has no collective
 * (/root/reference/run_denoising.py:79,87: one 'cuda' device); the default exchange of this build is torch.distributed (backend
 * "nccl" = RCCL) and these are the same sums for a host without torch.  One communicator per process (one process per GPU), created
 * on the current HIP device.  RCCL is opened with dlopen at vu_dp_unique_id / vu_dp_init (the copy the process already holds, or
 * librccl.so.1 of the ROCm installation): the library has no link-time dependency on it.
 *   vu_dp_unique_id         rank 0 fills 128 bytes (an ncclUniqueId) and hands them to every rank by any channel
 *   vu_dp_init              collective over all `world` ranks; one communicator per process (vu_dp_finalize before another)
 *   vu_dp_allreduce_bucket  in-place SUM over the ranks of ptr[0 .. count), dtype 0 = fp32 / 1 = bf16, enqueued on `stream`; the
 *                           1 / world average is applied by vu_adamw's grad_scale
 *   vu_dp_world             ranks of the communicator (0: none)
 * PROCESS-GLOBAL state (the communicator); not thread-safe against itself. */
int vu_dp_unique_id(void* out128);
int vu_dp_init(int rank, int world, const void* unique_id_128);
int vu_dp_allreduce_bucket(void* ptr, long long count, int dtype, void* stream);
int vu_dp_world(void);
int vu_dp_finalize(void);

/* In-process launch profiler (bench.py's roofline leg): PROCESS-GLOBAL state, meant for one
 * instrumented stream at a time.  After vu_prof_enable(stream) an event is
 * recorded behind every launch; vu_prof_report() stops, waits, and returns a JSON object
 * {"<kernel tag>": {"count","ms","flops","bytes"}} with ALGORITHMIC flops / bytes per tag. */
int vu_prof_enable(void* stream);
const char* vu_prof_report(void);
/* Holds the profiled stream for `usec` microseconds (0 .. 200000) with a one-wave kernel, so that the launches the host enqueues
 * behind it execute back to back: without it an interval between two events also contains the time the GPU waited for the host
 * (small batches: launches of 5 - 20 us are faster than the eager host).  Its own interval is not reported.  The report's
 * "flops_strict" counts the model's own products only (no recomputation, no padding); "flops" is the launch's work. */
int vu_prof_gate(int usec);

#ifdef __cplusplus
}
#endif
#endif
