/*
 * mewzoom_hip.h — C ABI of libmewzoom_hip.so: the MI355X (gfx950) implementation of the
 * MewZoom upscale path of andrewdalpino/UltraZoom v0.3.0.
 *
 * The reference has no FFI / plugin interface of its own: its boundary for this path is the Python
 * API of `MewZoom` (src/ultrazoom/model.py:43-192).  Each entry point below names the reference
 * interface it stands in for; INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative mz_status code and
 *     never throws; mz_last_error() returns a thread-local human-readable message.
 *   - all `dev` pointers are device (HBM) pointers owned by the CALLER (PyTorch-ROCm allocates
 *     them).  The library borrows them for the duration of the call and only keeps its own packed
 *     copy of the weights (allocated in mz_set_weight, freed in mz_destroy).
 *   - compute calls enqueue work on the given HIP stream and never synchronise; a handle must not
 *     be used from two threads at once.
 *   - images are NCHW, contiguous, element type = the handle's dtype, values nominally in [0, 1]
 *     (README.md:72-79 of the reference).
 */
#ifndef MEWZOOM_HIP_H
#define MEWZOOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mz_handle mz_handle;

typedef enum mz_dtype {
    MZ_F32 = 0,  /* exact f32 MFMA (v_mfma_f32_32x32x2_f32): the 1e-3 max-abs verification mode */
    MZ_BF16 = 1, /* bf16 storage, v_mfma_f32_16x16x32_bf16 (3x3 convolutions, mixes) / 32x32x16 (image head, 1x1), f32 accumulate and epilogues */
    MZ_F16 = 2   /* fp16 storage, v_mfma_f32_16x16x32_f16 / 32x32x16, f32 accumulate and epilogues */
} mz_dtype;

typedef enum mz_status {
    MZ_OK = 0,
    MZ_ERR_INVALID_ARGUMENT = -1, /* the reference raises AssertionError for these (model.py:67-69, 218-222, 265-275, 738) */
    MZ_ERR_UNKNOWN_WEIGHT = -2,
    MZ_ERR_SHAPE_MISMATCH = -3,
    MZ_ERR_MISSING_WEIGHTS = -4,
    MZ_ERR_WORKSPACE_TOO_SMALL = -5,
    MZ_ERR_HIP = -6,
    MZ_ERR_NO_DEVICE = -7
} mz_status;

/* The 11 constructor kwargs of MewZoom.__init__ (model.py:51-64), verbatim. */
typedef struct mz_config {
    int32_t upscale_ratio;
    int32_t primary_channels;
    int32_t primary_layers;
    int32_t secondary_channels;
    int32_t secondary_layers;
    int32_t tertiary_channels;
    int32_t tertiary_layers;
    int32_t quaternary_channels;
    int32_t quaternary_layers;
    int32_t hidden_ratio;
    int32_t num_deg_features;
} mz_config;

/* ---- lifetime: replaces MewZoom.__init__ (model.py:51-92) -------------------------------- */

/* Validates the configuration exactly as the reference constructor does (same rejected values)
 * and creates a handle that will compute in `dtype`.  Touches no GPU. */
int mz_create(const mz_config* cfg, int dtype, mz_handle** out);
int mz_destroy(mz_handle* h);

/* ---- weights: replaces load_state_dict / PyTorchModelHubMixin.from_pretrained (model.py:37,43;
 *      SURVEY.md appendix B for the key names) ---------------------------------------------- */

/* Number of state_dict entries the model has, and the name / shape of entry i.
 * `shape` receives up to 4 dims; returns ndim (0 for the scalar `alpha`s). */
int mz_num_weights(const mz_handle* h);
int mz_weight_info(const mz_handle* h, int index, const char** name, int64_t shape[4]);

/* Hands one BAKED parameter (plain conv.weight / bias / alpha — no weight-norm or LoRA
 * parametrisation left, test_compare.py:32-45) to the library.  `dev_f32` points at a contiguous
 * float32 device tensor in the reference layout (OIHW for conv weights).  The library packs it
 * into MFMA-fragment order in the handle's dtype on the given stream; the caller may free its
 * tensor once the stream has passed this call. */
int mz_set_weight(mz_handle* h, const char* name, const float* dev_f32, const int64_t* shape, int ndim,
                  void* hip_stream);

/* 0 when every parameter has been set, else MZ_ERR_MISSING_WEIGHTS (message lists the first one). */
int mz_weights_complete(const mz_handle* h);

/* ---- the hot path: replaces MewZoom.forward / upscale / predict_degredation
 *      (model.py:149-164, 166-179, 181-192) -------------------------------------------------- */

/* Bytes of scratch HBM a call with this batch/shape needs.  The library processes the batch in
 * micro-batches of at most `max_images_in_flight` images (0 = library default), so memory does
 * not grow beyond that.
 *
 * What a call touches (mz_forward, mz_forward_u8, mz_forward_view, mz_metrics, mz_metrics_luma, mz_luma, mz_yuv420_to_rgb, mz_rgb_to_yuv420,
 * mz_ycbcr_to_rgb, mz_rgb_to_ycbcr, mz_resize, mz_interpolate, mz_blur, mz_noise,
 * mz_jpeg, mz_alpha_fill, mz_alpha_merge, mz_feather_paste and the mz_op_* entries alike): it READS only its
 * input tensors -- the elements its shape and strides name, never a byte next to them -- and the workspace bytes it has itself
 * written during that call; it WRITES only its outputs (of a view: the elements of the window) and its workspace, never an input.
 * The workspace needs no initialisation and carries nothing from one call to the next: whatever it holds, NaN patterns included,
 * the results have the same bits.  mz_metrics and mz_metrics_luma write the `out` slots of the metrics `which` selects and leave the
 * others alone.  tests/test_poison_ops_gpu.py, tests/test_poison_forward_gpu.py, tests/test_metrics_gpu.py and
 * tests/test_poison_color_gpu.py, tests/test_poison_yuv_gpu.py, tests/test_poison_ycbcr_gpu.py, tests/test_poison_alpha_gpu.py,
 * tests/test_poison_feather_gpu.py hold every entry to this.
 *
 * Number range (the convolution, mix, stem and head kernels, in every storage type): subnormals of the storage type are operands and
 * results like any other value -- nothing is flushed on the way in, in the matrix unit's operands, or at the store.  Accumulation is
 * f32, f32 subnormals included.  A result is rounded ONCE, to nearest even, into the subnormal range where it lies there and to
 * +-inf from the overflow tie upward (fp16: 65520).  One thing holds instead of the plain formula inside SiLU and the mix's gate:
 * their sigmoid is a hardware reciprocal (v_rcp_f32) whose result is ZERO where it would be an f32 subnormal, so for sigmoid(t) <
 * 2^-126, t < -87.34, SiLU(t) is -0 (not t sigmoid(t), about -88 * 2^-126) and the gate's weight is 0 (the blend returns x; invisible
 * beside x itself).  Not promised beyond that: other f32 intermediates below 2^-126 inside SiLU and the gate may flush, too; SiLU
 * and the blend are accurate to half an ulp of the storage type plus 2^-16 relative, not exact.  Non-finite inputs are out of scope.
 * tests/test_range_gpu.py holds every kernel family to this (data and bounds: tests/range_util.py, tests/test_range_cpu.py). */
int mz_workspace_bytes(const mz_handle* h, int B, int H, int W, int max_images_in_flight, size_t* bytes);

/* x        [B,3,H,W]      input, handle dtype
 * out_sr   [B,3,rH,rW]    s + head(unet(stem(x))) (model.py:162); clamped to [0,1] when clamp != 0
 *                         (model.py:177); must not be NULL
 * out_qa   [B,F] float32  degradation features z_qa (model.py:159,1026-1032), or NULL to skip the
 *                         quality head (upscale() discards it, model.py:175)
 */
int mz_forward(mz_handle* h, const void* x, void* out_sr, float* out_qa, int B, int H, int W, int clamp,
               void* workspace, size_t workspace_bytes, int max_images_in_flight, void* hip_stream);

/* The same path with uint8 images at both ends: every caller of the reference wraps
 * upscale() in `ToDtype(float32, scale=True)` and `save_image` (README.md:72-83, test_compare.py:53-57,89); here the
 * /255 happens in the stem's read and clamp -> *255 + 0.5 -> uint8 in the final store, so the two extra passes over
 * the largest tensors disappear.   x [B,3,H,W] uint8 -> out_sr [B,3,rH,rW] uint8. */
int mz_forward_u8(mz_handle* h, const uint8_t* x, uint8_t* out_sr, float* out_qa, int B, int H, int W,
                  void* workspace, size_t workspace_bytes, int max_images_in_flight, void* hip_stream);

/* Images as VIEWS at both ends: any layout that four element strides describe -- channels-last / interleaved HWC, a crop of a
 * larger frame, every second image of a batch, BGR (a negative channel stride with `data` at channel 2) -- is read and written in
 * place, without a copy on either side.  mz_forward and mz_forward_u8 are the dense NCHW special case.
 *
 * `data` is the address of element (image 0, channel 0, row 0, column 0) and needs the alignment of ONE element only; strides are
 * counted in ELEMENTS and may be negative.  The library reads and writes exactly the elements the view names.  Overlap between x
 * and out, or between elements of out, is the caller's responsibility and is not checked (beyond refusing an output stride of 0;
 * mz_blur, mz_noise and mz_jpeg also compare the two byte ranges).
 *
 * THE VIEW REFUSALS.  Every entry that takes views (mz_forward_view, mz_metrics, mz_metrics_luma, mz_luma, mz_yuv420_to_rgb, mz_rgb_to_yuv420,
 * mz_ycbcr_to_rgb, mz_rgb_to_ycbcr, mz_resize, mz_interpolate, mz_blur,
 * mz_noise, mz_jpeg, mz_dihedral, mz_ensemble_add, mz_ensemble_finish, mz_alpha_fill, mz_alpha_merge, mz_feather_paste) returns
 * MZ_ERR_INVALID_ARGUMENT, before anything touches the GPU, for: a null view or null data; an `elem` outside the entry's codes; a view
 * that is WRITTEN whose channel, row or column stride is 0, or whose image stride is 0 when B > 1 (mz_luma's one-channel output: its
 * channel stride is never used and may be anything; strides of a view that is only read
 * may be 0, and any stride may be negative); where the entry takes a window: one that is empty or not inside the result.  Each entry
 * below lists only what it refuses beyond these.  A workspace that is null or smaller than the entry's *_workspace_bytes is
 * MZ_ERR_WORKSPACE_TOO_SMALL.  (ultrazoom_amd/csrc/mz_view_check.h is the one statement of these checks.)
 *
 * A call within these bounds whose kernel would need more workgroups than one grid holds -- 2^24 - 1 workgroups of 256 threads: a grid
 * dimension counts its work-items in 32 bits, and a larger grid would be launched cut short, without an error -- is refused with
 * MZ_ERR_HIP (hipErrorInvalidValue) and writes nothing.  The streaming entries take one work item per run of a row (mz_luma: 16 bytes of
 * elements; the four YCbCr entries: 16 columns), so this is B * rows * runs < 2^32; mz_noise, one thread an element, splits such a call into
 * several launches and serves 2^42 elements. */
typedef struct mz_image_view {
    void*   data;        /* element (image 0, channel 0, row 0, column 0) */
    int64_t stride[4];   /* in ELEMENTS, signed: image, channel, row, column */
} mz_image_view;

/* x       view of [B,3,H,W]; out: view of the window of [B,3,rH,rW]; out_qa, clamp, workspace, micro-batches as for mz_forward
 *         (micro-batches advance both views by stride[0]; mz_workspace_bytes is the same as for the dense entries).
 * window  {y0, x0, h, w} in OUTPUT pixels of the rH x rW result, or NULL for all of it.  out->data is the element that receives
 *         output pixel (y0, x0); out spans h x w pixels.  The window changes where results are stored, never what is computed: a
 *         window of a result equals that part of the whole result bit for bit (tiling: the haloed slice as x, the core as window).
 * elem    0 = the handle's dtype, 1 = uint8 (scaling and rounding exactly as mz_forward_u8; clamp is implied).
 * Refuses the view refusals above (elem outside {0, 1}; the window inside [0, rH) x [0, rW)), and a null handle, B < 1, H or W < 8. */
int mz_forward_view(mz_handle* h, const mz_image_view* x, const mz_image_view* out, float* out_qa,
                    int B, int H, int W, int clamp, int elem, const int32_t window[4],
                    void* workspace, size_t workspace_bytes, int max_images_in_flight, void* hip_stream);

/* ---- single operators, exported for the parity tests (tests/test_ops_gpu.py) ---------------
 * These run the SAME kernels mz_forward launches, on caller-provided tensors.
 * Activation tensors here are the library's internal layout: plane-major [B][P][H][W][16 bytes], channel count padded
 * to a multiple of 16, element type = dtype.  mz_padded_channels(c) gives that count. */
int mz_padded_channels(int c);

/* kind: 0 conv3x3 pad1 (+SiLU when silu!=0)            w: [cout,cin,3,3]    out [B,H,W,cout_p]
 *       1 conv3x3 + PixelShuffle(2) into [B,Hout,Wout,cout/4] (zero-filled beyond 2H,2W)
 *       2 PixelCrush conv2x2 stride2                   w: [cout,cin,2,2]    out [B,H/2,W/2,cout_p]
 *       3 AdaptiveResidualMix(in0, in1)                w: [c,2c,1,1], alpha out [B,H,W,c_p]
 */
int mz_op_conv(int dtype, int kind, const void* in0, const void* in1, const float* w_dev_f32, float alpha,
               void* out, int B, int H, int W, int cin, int cout, int Hout, int Wout, int silu,
               void* hip_stream);
/* stem: NCHW image -> NHWC features (model.py:239-242) */
int mz_op_stem(int dtype, const void* x, const float* w_dev_f32, const float* b_dev_f32, void* out, int B,
               int H, int W, int cout, void* hip_stream);
/* final: conv3x3 (cin -> 12) + PixelShuffle(2) + bicubic(img, R) + add [+ clamp] -> NCHW image
 * feat [B,H,W,cin_p]; img [B,3,H*2/R,W*2/R]; out [B,3,2H,2W]  (model.py:926-930, 156, 162, 177) */
int mz_op_final(int dtype, const void* feat, const void* img, const float* w_dev_f32, void* out, int B, int H,
                int W, int cin, int R, int clamp, void* hip_stream);

/* conv2 of an Encoder/DecoderBlock + AdaptiveResidualMix with the block input, ONE launch (reference model.py:773-778 second half and
 * 826-839: z = conv3x3(hid, w2); out = x + sigmoid(alpha) sigmoid(Wmix [x ; z]) (z - x)): the fused kernels of C <= 96.
 * hid [B,H,W,cin_p]; x, out [B,H,W,cout_p]; w2 [cout,cin,3,3]; wmix [cout,2 cout,1,1] (float32 on the device) */
int mz_op_conv_mix(int dtype, const void* hid, const void* x, const float* w2_dev_f32, const float* wmix_dev_f32, float alpha,
                   void* out, int B, int H, int W, int cin, int cout, void* hip_stream);

/* a17 of SURVEY.md section 8 -- NO reference counterpart: the snapshot (v0.3.0) has no ControlModule / FiLM (README.md:86-129
 * describes library version 0.2.x, whose source is absent), so this operator is "parity unpinned": it is checked against the
 * build's own CPU restatement (oracle.film_conv) only.   out = act(gamma[b, c] * conv3x3(in0, w)[b, c] + beta[b, c]),
 * act = SiLU when silu != 0.  gamma, beta: float32 [B][cout] on the device.  bf16 / fp16 only (the epilogue lives on the
 * 16x16x32 kernel); other configurations return MZ_ERR_INVALID_ARGUMENT. */
int mz_op_conv_film(int dtype, const void* in0, const float* w_dev_f32, const float* gamma_dev_f32,
                    const float* beta_dev_f32, void* out, int B, int H, int W, int cin, int cout, int silu,
                    void* hip_stream);

/* ---- image-quality metrics: no reference counterpart in `model.py`; stands in for torchmetrics as the reference's
 *      `pretrain.py:209-211, 301-329` uses it (PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure,
 *      VisualInformationFidelity with their defaults; ultrazoom_amd/evaluate.py restates them) ------------------------------------
 * Stateless like the mz_op_* entries (no handle): the calls enqueue on the given stream and never synchronise.  Both images are
 * VIEWS of one logical shape [B,3,H,W] (mz_image_view above: any strides, nothing is copied) and of one element type; a uint8
 * value v means v / 255, as in mz_forward_u8.  All arithmetic is float64; reductions add in a fixed order (no atomics), so two
 * calls give the same bits and the sums of an image do not depend on the batch it is measured in (SSIM with data_range <= 0
 * excepted, by its definition).
 *
 * out_dev[b][slot], float64, MZ_METRIC_SLOTS per image:
 *    0      sum of (p - t)^2 over the image            1      its element count 3 H W            (PSNR, bit 0; also written when
 *    2, 3   min, max of p                              4, 5   min, max of t                       SSIM takes its range from the batch)
 *    6      sum of the SSIM map: the 3 (H-10) (W-10) pixels whose 11 x 11 Gaussian window (sigma 1.5) lies inside the image -- what
 *           torchmetrics keeps after reflect-padding by 5 and cropping 5 again;   7   that pixel count;   14  the data range used   (SSIM, bit 1)
 *    8..10  per channel: sum over the four scales (windows of 17, 9, 5, 3 taps, sigma = taps / 5, "valid" filtering, every second
 *           row and column between scales) of log10(1 + g^2 s_tt / (s_v + sigma_n_sq));   11..13  ... of log10(1 + s_tt / sigma_n_sq)   (VIF, bit 2)
 *    15     reserved
 * The caller divides: MSE = slot 0 / slot 1 (over all updates), SSIM = slot 6 / slot 7, VIF = mean over channels of
 * slot (8 + c) / slot (11 + c) -- 0 / 0 stays NaN exactly where the torch restatement gives NaN.  Slots of metrics that were not
 * requested are left as they were.
 *
 * Refuses the view refusals above (elem outside 0..3; both views are only read), and: which == 0 or with unknown bits; B, H or W < 1
 * (or B > 65535, H or W > 2^28); H or W < 11 with SSIM; H or W < 41 with VIF; a null out_dev. */
#define MZ_METRIC_SLOTS 16
#define MZ_METRIC_PSNR 1
#define MZ_METRIC_SSIM 2
#define MZ_METRIC_VIF 4
/* which: bit 0 PSNR, bit 1 SSIM, bit 2 VIF.  Host only. */
int mz_metrics_workspace_bytes(int B, int H, int W, int which, size_t* bytes);
/* elem: 0..2 = mz_dtype, 3 = uint8.  data_range (SSIM): > 0 fixed; <= 0: max(range of pred, range of target) of THIS batch, found on
 * the device, as torchmetrics' data_range=None.  sigma_n_sq (VIF): the reference's default is 2.0. */
int mz_metrics(const mz_image_view* pred, const mz_image_view* target, int elem, int B, int H, int W, int which,
               double data_range, double sigma_n_sq, double* out_dev, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- luma (Y): no reference counterpart (the reference's validate.py measures RGB over the full frame); the channel every
 *      super-resolution paper reports PSNR / SSIM on.  ultrazoom_amd/csrc/mz_color.h is the one statement of the arithmetic -----------
 * standard   0 "bt601": studio range, MATLAB's rgb2ycbcr and basicsr's bgr2ycbcr(y_only=True), for R, G, B in units of [0, 1]
 *                       Y = 16/255 + (65.481/255) R + (128.553/255) G + (24.966/255) B          (white 235/255, black 16/255)
 *            1 "full":  full range, BT.601 / JFIF / Pillow's "L":   Y = 0.299 R + 0.587 G + 0.114 B
 * The constants are the float64 results of the divisions as written; the sum is float64, acc = off, then acc = fma(k, v, acc) for R, G,
 * B in this order; a uint8 element v is v / 255.0 by true division.
 *
 * mz_luma: x, a view of [B,3,H,W], to out, a view of [B,1,H,W] of the same element type (elem 0..3; out's channel stride is never used).
 * The float64 sum is rounded ONCE on store: a float type by one rounding to nearest even, after a clamp to [0, 1] when clamp != 0 (a NaN
 * becomes 0); uint8 always clamps, then * 255 + 0.5, then truncates, in float64.  Stateless, no workspace; enqueues on the given stream;
 * reads exactly the B 3 H W elements named and writes exactly B H W.
 * Refuses the view refusals above (elem outside 0..3), and: B < 1 or > 65535; H or W < 1 or > 2^28; a standard outside 0..1; ANY overlap
 * of the byte ranges of x and out (the entry does not work in place).
 *
 * mz_metrics_luma: mz_metrics of the Y planes of pred and target.  A first kernel writes both planes UNROUNDED, float64, into the
 * workspace (so the metric sees Y in float64 whatever the element type); the kernels of mz_metrics then run on one plane instead of three.
 * The workspace is that of one plane plus the two Y planes, 2 * 8 B H W bytes (mz_metrics_luma_workspace_bytes).  out_dev has mz_metrics'
 * slots with these differences: slot 1 is H W; slot 7 is (H-10) (W-10); VIF writes slots 8 and 11 only (VIF = slot 8 / slot 11) and
 * slots 9, 10, 12, 13 are left alone.  data_range <= 0 takes the range of the Y planes of the batch.  Everything mz_metrics promises
 * about what a call touches, equal bits of two calls and independence of the batch holds.
 * Refuses what mz_metrics refuses, and: a standard outside 0..1; B H W beyond 2^58 (the two planes would pass 2^62 bytes). */
int mz_luma(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int standard, int clamp,
            void* hip_stream);
int mz_metrics_luma_workspace_bytes(int B, int H, int W, int which, size_t* bytes);
int mz_metrics_luma(const mz_image_view* pred, const mz_image_view* target, int elem, int B, int H, int W, int which, int standard,
                    double data_range, double sigma_n_sq, double* out_dev, void* workspace, size_t workspace_bytes, void* hip_stream);
/* Host only: {off, kr, kg, kb} of a standard, the constants the kernels compile. */
int mz_debug_luma_coeffs(int standard, double out[4]);

/* ---- 8-bit 4:2:0 YCbCr frames: no reference counterpart; what video decoders and encoders exchange (NV12, NV21, I420, YV12).
 *      ultrazoom_amd/csrc/mz_yuv.h is the one statement of the arithmetic -------------------------------------------------------------
 * The planes are three views of uint8 CODE VALUES 0..255: y of [B,1,H,W], cb and cr of [B,1,Hc,Wc] with Hc = ceil(H/2), Wc = ceil(W/2)
 * (their channel strides are never used).  A layout is a choice of views, not of kernels: I420 / YV12 are two planar chroma views
 * (column stride 1), NV12 / NV21 two views with column stride 2 one byte apart.  Odd H and W are legal; indices clamp at the edges.
 * matrix   0 "bt601" (Kr = 0.299, Kb = 0.114), 1 "bt709" (Kr = 0.2126, Kb = 0.0722); Kg = (1 - Kr) - Kb
 * range    0 "limited" (Y 16..235, chroma 16..240: Yoff = 16, Sy = 219, Sc = 224), 1 "full" (Yoff = 0, Sy = Sc = 255)
 * siting   0 "left" (a chroma sample sits on luma column 2i, between luma rows 2j and 2j + 1: MPEG-2, H.264, HEVC),
 *          1 "center" (in the middle of its 2 x 2 luma block: JPEG, MPEG-1)
 * Float64 throughout, sums in a fixed order, one rounding on store.
 *
 * mz_yuv420_to_rgb: chroma is upsampled by the 3/4, 1/4 taps of the siting (vertically; horizontally the same for "center", the sample
 * itself and the mean of two for "left"), then R = yn + a_r crn, B = yn + a_b cbn, G = yn + g_r crn + g_b cbn on yn = (Y - Yoff) / Sy,
 * cbn = (cb - 128) / Sc; out, a view of [B,3,H,W] of element type elem_out (0..3), is stored as mz_luma stores: float types clamped to
 * [0, 1] when clamp != 0, then one rounding; uint8 always clamps, then * 255 + 0.5, then truncates.  Reads exactly the plane elements
 * named, writes exactly B 3 H W elements.
 * mz_rgb_to_yuv420: y = Kr r + Kg g + Kb b of the [B,3,H,W] view x (elem 0..3), pb = (b - y) / (2 (1 - Kb)), pr likewise; the Y code is
 * Sy y + Yoff clamped to [0, 255] (no 16..235 clamp), + 0.5, truncated; a chroma sample is the siting's filter over the UNROUNDED pb, pr
 * of its 2 rows x 2 (center) or 3 (left) columns, Sc f + 128 clamped to [0, 255], + 0.5, truncated.  Writes every plane element once.
 * Both are stateless, need no workspace and enqueue on the given stream.
 * Refuse the view refusals above (the written views: out; y, cb and cr), and: B < 1 or > 65535; H or W < 1 or > 2^28; a matrix, range or
 * siting outside 0..1; ANY overlap of the byte range of the RGB view with that of a plane.  mz_rgb_to_yuv420 also refuses two planes of
 * which an image of one shares bytes with an image of the other -- except that Cb and Cr may INTERLEAVE: identical strides, a column
 * stride of at least 2 and base addresses at least one byte but less than the column stride apart.  The three codes are checked last. */
int mz_yuv420_to_rgb(const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr, const mz_image_view* out, int elem_out,
                     int B, int H, int W, int matrix, int range, int siting, int clamp, void* hip_stream);
int mz_rgb_to_yuv420(const mz_image_view* x, int elem, const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr,
                     int B, int H, int W, int matrix, int range, int siting, void* hip_stream);
/* Host only: {Yoff, 1/Sy, 1/Sc, a_r, a_b, g_r, g_b, Sy, Sc} of a matrix and a range, the constants the kernels compile. */
int mz_debug_yuv_coeffs(int matrix, int range, double out[9]);

/* ---- YCbCr frames of 8, 10, 12 or 16 bits in 4:2:0, 4:2:2 or 4:4:4: the two entries above generalised (P010 / P012 / P016, yuv420p10le
 *      and its kin, NV16 / NV24, I422 / I444, BT.2020).  ultrazoom_amd/csrc/mz_ycbcr.h is the one statement of the arithmetic ------------
 * Where a parameter takes the value of the 4:2:0 entries, every operation and its order are theirs: depth 8, subsampling 0 and matrix 0
 * or 1 give the bits of mz_yuv420_to_rgb / mz_rgb_to_yuv420.
 * depth        8: planes of uint8; 10, 12, 16: planes of host-endian uint16 (strides count ELEMENTS; data aligned to 2 bytes).  With
 *              s = 2^(depth - 8): "limited" Yoff = 16 s, Sy = 219 s, Sc = 224 s; "full" Yoff = 0, Sy = Sc = 2^depth - 1; the chroma
 *              midpoint is 2^(depth - 1); codes clamp to [0, 2^depth - 1]
 * align        of a 16-bit container: 0 "low" -- a code is word & (2^depth - 1), written as it is (yuv420p10le, ..); 1 "high" -- a code
 *              is word >> (16 - depth), written as code << (16 - depth), the low bits zero (P010, P012, P016).  Depth 8 and 16: no difference
 * subsampling  cb and cr are views of [B,1,Hc,Wc]: 0 "420" Hc = ceil(H/2), Wc = ceil(W/2); 1 "422" Hc = H, Wc = ceil(W/2), no vertical
 *              filter; 2 "444" Hc = H, Wc = W, no filter (the siting must still be a valid code)
 * matrix       0, 1 as above; 2 "bt2020" (Kr = 0.2627, Kb = 0.0593, non-constant luminance)
 * Refuse what mz_yuv420_to_rgb and mz_rgb_to_yuv420 refuse (a matrix outside 0..2), and: a depth outside {8, 10, 12, 16}; an align
 * outside 0..1; a subsampling outside 0..2; plane data not aligned to 2 bytes when depth > 8.  Byte ranges are those of the planes'
 * element size, and the interleaving exception counts ELEMENTS: identical strides, a column stride of at least 2, bases a whole number
 * of elements -- at least one, fewer than the column stride -- apart.  Matrix, range and siting are checked last. */
int mz_ycbcr_to_rgb(const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr, int depth, int align, int subsampling,
                    const mz_image_view* out, int elem_out, int B, int H, int W, int matrix, int range, int siting, int clamp, void* hip_stream);
int mz_rgb_to_ycbcr(const mz_image_view* x, int elem, const mz_image_view* y, const mz_image_view* cb, const mz_image_view* cr,
                    int depth, int align, int subsampling, int B, int H, int W, int matrix, int range, int siting, void* hip_stream);
/* Host only: the nine values of mz_debug_yuv_coeffs at a depth, then the chroma midpoint and the largest code. */
int mz_debug_ycbcr_coeffs(int matrix, int range, int depth, double out[11]);

/* ---- antialiased resampling to any size: no reference counterpart in `model.py`; stands in for torchvision's antialiased `Resize`
 *      as the reference's `data.py:91-108` uses it (HR -> LR for validation), and serves "a 3X or a true-4K result from a 4X model"
 *      (ultrazoom_amd/model.py: MewZoom.upscale_to) -------------------------------------------------------------------------------
 * Stateless like mz_metrics (no handle): the call enqueues on the given stream and never synchronises, allocates nothing and copies
 * nothing from the host -- its tap tables are built on the device, in the workspace.  x is a VIEW of [B,3,Hin,Win], out a view of the
 * window {y0, x0, h, w} of the [B,3,Hout,Wout] result, or of all of it when window is NULL (mz_image_view and the window as for
 * mz_forward_view: out->data receives result pixel (y0, x0); the window changes where results are stored, never what is computed).  Both
 * views have one element type; a uint8 value v is read as v / 255 and stored as clamp -> * 255 + 0.5 -> truncate, exactly as
 * mz_forward_u8; clamp != 0 clamps the other types to [0, 1] before the store (bicubic overshoots).  The touch contract of the
 * workspace paragraph above holds: the call reads only the elements of x that the window's outputs need, writes only the window's
 * elements and its workspace, and a workspace full of NaN patterns gives the same bits.
 *
 * The arithmetic is torch.nn.functional.interpolate(..., mode = "bicubic" | "bilinear", antialias=True, align_corners=False).  Per
 * axis, n_in samples to n_out:   scale = n_in / n_out (double, from the two sizes);   support = interp / 2 * max(scale, 1);
 * inv = 1 / max(scale, 1);   center = scale (i + 0.5);   first = max((int)(center - support + 0.5), 0);
 * count = min((int)(center + support + 0.5), n_in) - first;   w_j = f((j + first - center + 0.5) inv) / sum_j f(..), in double;
 * out[i] = sum_j w_j in[first + j].   f: bicubic with A = -0.5 (interp 4; torch's antialiased kernels use the PIL constant, not the
 * -0.75 of the model's skip) or the triangle 1 - |u| (interp 2).  Horizontal pass, then vertical pass; both ACCUMULATE IN FLOAT64 with
 * fma in ascending j from the double weights; the intermediate between them is float32, never the storage type.  An axis with
 * n_out == n_in has the table {0, 1, 0, 0}: finite values pass through it exactly.  Dense and strided views give the same bits, two
 * calls give the same bits (no atomics), and an image does not depend on the batch it is resized in.
 *
 * Refuses the view refusals above (elem outside 0..3), and: a filter outside {0, 1}; B or any size < 1; B > 65535; a size > 2^28;
 * n_in / n_out > 16 on either axis (bounds count at 66; enlarging is not bounded). */
#define MZ_RESIZE_BICUBIC 0
#define MZ_RESIZE_BILINEAR 1
/* Host only. */
int mz_resize_workspace_bytes(int Hin, int Win, int Hout, int Wout, int filter, size_t* bytes);
/* elem: 0..2 = mz_dtype, 3 = uint8. */
int mz_resize(const mz_image_view* x, const mz_image_view* out, int elem, int B, int Hin, int Win, int Hout, int Wout,
              int filter, int clamp, const int32_t window[4], void* workspace, size_t workspace_bytes, void* hip_stream);
/* Host only (no GPU): the table of output index i of one axis, from the source the device compiles too: returns count (<= cap), *first,
 * w[0..count) in double; negative on bad arguments (count > cap among them).  No reference counterpart. */
int mz_debug_resize_taps(int n_in, int n_out, int filter, int i, int* first, double* w, int cap);

/* ---- plain interpolation to any size: the model's own skip connection, `Upsample(scale_factor=r, mode="bicubic")` (model.py:71, 156),
 *      and the bicubic baseline the reference puts next to every result (validate.py:84-118, test_compare.py:61-77) ----------------------
 * NOT mz_resize: no antialiasing, a fixed tap count (1, 2 or 4 an axis) whatever the ratio, and bicubic with A = -0.75.  Stateless like
 * mz_resize: the call enqueues on the given stream, never synchronises, allocates nothing, uses no atomics and needs NO WORKSPACE.  x is a
 * VIEW of [B,3,Hin,Win], out a view of the window {y0, x0, h, w} of the [B,3,Hout,Wout] result, or of all of it when window is NULL (as
 * for mz_resize: the window changes where results are stored, never what is computed).  Any sizes, up or down; no ratio limit.  Both
 * views have one element type.  The touch contract of the workspace paragraph above holds: the call reads only the source elements that
 * the window's outputs name and writes only the window.
 *
 * The arithmetic is torch.nn.functional.interpolate(x, size=(Hout, Wout), mode=..., align_corners=False) without antialiasing
 * (Upsample(scale_factor=r) with an integer r is the same function).  Per axis, n_in samples to n_out, s = n_in / n_out in double:
 *   nearest   (torch's legacy "nearest")  idx = i when n_in == n_out, else min((int)floorf((float)i * sf), n_in - 1) with
 *             sf = (float)n_in / (float)n_out, in float32 as torch does it.  Elements are moved and never changed: bit patterns survive,
 *             NaN payloads and -0 included.
 *   bilinear  src = max(s (i + 0.5) - 0.5, 0);  i0 = (int)src;  i1 = i0 + (i0 < n_in - 1);  w = {1 - (src - i0), src - i0}
 *   bicubic   src = s (i + 0.5) - 0.5;  f = floor(src);  t = src - f;  idx_k = clamp(f - 1 + k, 0, n_in - 1), k = 0..3;
 *             w = {c2(t + 1), c1(t), c1(1 - t), c2(2 - t)};  c1(u) = ((A + 2) u - (A + 3)) u u + 1;  c2(u) = ((A u - 5 A) u + 8 A) u - 4 A;
 *             A = -0.75
 * Bilinear and bicubic: weights in double; each source row an output needs is filtered horizontally, the row results are combined
 * vertically, both in FLOAT64 as acc = fma(w_k, v_k, acc) from 0 in ascending k; ONE rounding to the stored type.  A uint8 value v is
 * read as v / 255 and stored as clamp -> * 255 + 0.5 -> truncate (float64); clamp != 0 clamps the other types to [0, 1] before the store
 * (on 0 / 1 data bicubic reaches -0.32 and 1.32).  An axis with n_out == n_in has the weights {1, 0} / {0, 1, 0, 0} exactly: finite values
 * pass through.  Dense and strided views give the same bits, two calls give the same bits, and an image does not depend on the batch it
 * is interpolated in.  (ultrazoom_amd/csrc/mz_interp.h is the one statement of taps and order, compiled by the kernels and the host.)
 *
 * Refuses the view refusals above (elem outside 0..3), and: a mode outside 0..2; B < 1 or > 65535; a size < 1 or > 2^28; x and out whose
 * byte ranges overlap or do not fit in signed 64-bit addresses; clamp != 0 with nearest. */
#define MZ_INTERP_NEAREST  0
#define MZ_INTERP_BILINEAR 1
#define MZ_INTERP_BICUBIC  2
/* elem 0..2 = mz_dtype, 3 = uint8; window {y0, x0, h, w} of the Hout x Wout result or NULL; no workspace */
int mz_interpolate(const mz_image_view* x, const mz_image_view* out, int elem, int B, int Hin, int Win,
                   int Hout, int Wout, int mode, int clamp, const int32_t window[4], void* hip_stream);
/* host only, no GPU: the taps of output index i of one axis, from the source the kernels compile too:
   returns count (1, 2 or 4), idx[0..count) already clamped to [0, n_in), w[0..count) in double; negative on bad arguments */
int mz_debug_interp_taps(int n_in, int n_out, int mode, int i, int idx[4], double w[4]);

/* ---- the degradation chain: no reference counterpart in `model.py`; stands in for torchvision's `gaussian_blur`, `gaussian_noise`
 *      and `jpeg` as the reference's `transforms.py` calls them (data.py:134-164: blur -> noise -> resize -> JPEG makes the LR input of
 *      an HR image; the three parameters are the quality head's target) ---------------------------------------------------------------
 * Stateless like mz_resize: each call enqueues on the given stream, never synchronises and allocates nothing.  x and out are VIEWS of
 * one logical shape [B,3,H,W] and one element type (elem 0..2 = mz_dtype, 3 = uint8: v means v / 255, stored as clamp -> * 255 + 0.5 ->
 * truncate).  Parameters are scalars of the call: per-image parameters are one call per image, on a view of that image.  Dense and
 * strided views give the same bits; the touch contract of the workspace paragraph above holds.  ultrazoom_amd/csrc/mz_degrade.h states
 * the arithmetic in full; in short:
 *
 * mz_blur   k = 2 * int(3 sigma) + 1 taps (transforms.py:39), w_j = exp(-0.5 (j / sigma)^2) / sum in double, separable, reflect
 *           padding, both passes accumulated in float64 in ascending j, float32 between them.  sigma < 1 / 3 copies.
 * mz_noise  out = clamp(x + sigma n, 0, 1), n from the library's own stream: Philox4x32-10 keyed by `seed`, counter = (element index
 *           (c H + y) W + x, stream id offset + b), Box-Muller on the first two words in float64.  The noise of a pixel depends on
 *           neither layout nor strides nor how a batch is split into calls (pass offset + b for image b).  out may be the SAME view as
 *           x (in place); any other overlap is refused.
 * mz_jpeg   a baseline JPEG round trip at `quality` 1..100, 4:2:0, modelled in arithmetic (no entropy coder, which is lossless):
 *           8-bit RGB -> YCbCr -> 2 x 2 chroma means -> 8 x 8 DCT-II (float64) -> Annex K tables scaled by the quality -> rounding ->
 *           inverse DCT -> triangle chroma upsampling -> RGB.  The workspace holds the decoded planes (1.5 bytes a padded pixel).
 *
 * Refuse the view refusals above (elem outside 0..3), and: B, H or W < 1; B > 65535; H or W > 2^28; x and out whose byte ranges
 * overlap (mz_noise: unless they are the same view) or do not fit in signed 64-bit addresses; mz_blur: sigma negative or not finite,
 * int(3 sigma) > 15, or int(3 sigma) >= min(H, W), where reflect padding is undefined; mz_noise: sigma negative, not finite or
 * > 1e6; mz_jpeg: quality outside 1..100. */
int mz_blur(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, double sigma, void* hip_stream);
int mz_noise(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, double sigma, uint64_t seed,
             uint64_t offset, void* hip_stream);
/* Host only. */
int mz_jpeg_workspace_bytes(int B, int H, int W, size_t* bytes);
int mz_jpeg(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int quality, void* workspace,
            size_t workspace_bytes, void* hip_stream);
/* Host only (no GPU), from the source the kernels are built from: the k weights of a sigma (returns k <= cap); the two quantisation
 * tables of a quality, row-major [64] each; one Philox4x32-10 block.  No reference counterpart. */
int mz_debug_blur_weights(double sigma, double* w, int cap);
int mz_debug_jpeg_qtable(int quality, uint8_t* luma, uint8_t* chroma);
int mz_debug_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/* ---- the dihedral transforms and the geometric self-ensemble: no reference counterpart in `model.py`; the flip is the reference's
 *      `RandomHorizontalFlip` augmentation (pretrain.py:148), the ensemble the "+" variant of the super-resolution papers: the model runs
 *      on the 8 orientations of the input, each result is turned back, the results are averaged (ultrazoom_amd/ensemble.py:
 *      upscale_ensemble; MewZoom.upscale_ensemble) ------------------------------------------------------------------------------------
 * Stateless like mz_resize: every call enqueues on the given stream, never synchronises, allocates nothing and uses no atomics.  Images
 * are VIEWS (mz_image_view above) of one element type, elem 0..2 = mz_dtype, 3 = uint8.  All element offsets are 64-bit: there is no
 * size guard beyond the bounds below.  The touch contract of the workspace paragraph above holds.
 *
 * THE TRANSFORM.  Orientation k = 0..7 has three bits: bit 0 reverses columns, bit 1 reverses rows, bit 2 exchanges rows and columns and
 * is applied LAST.  For x of [B,3,H,W]:   T(x, k)[b, c, i, j] = x[b, c, si, sj]   with (p, q) = (j, i) if k & 4 else (i, j),
 * si = H - 1 - p if k & 2 else p,   sj = W - 1 - q if k & 1 else q;   T(x, k) is [B,3,W,H] when k & 4.  In torch: flip(2) if k & 2,
 * flip(3) if k & 1, then transpose(2, 3) if k & 4.  inverse(k) = k for k < 4, else 4 | (k & 1) << 1 | (k & 2) >> 1, and
 * T(T(x, k), inverse(k)) == x.  The transform moves elements and never changes them: bit patterns survive, NaN payloads and -0
 * included.  (ultrazoom_amd/csrc/mz_dihedral.h is the one statement of it, compiled by the kernels and the host alike.)
 *
 * mz_dihedral          out, a view of [B,3,H',W'], receives T(x, k) of x, a view of [B,3,H,W].  Dense and strided views give the same
 *                      bits.  Refuses the view refusals above (elem outside 0..3), and: B < 1 or > 65535; H or W < 1 or > 2^28; k outside
 *                      0..7; x and out whose byte ranges (each from its own shape) overlap or do not fit in signed 64-bit addresses.
 *
 * THE ENSEMBLE.  The workspace is the accumulator: a dense float32 [B,3,H,W], 12 B H W bytes, where H x W is the size of the RESULT (the
 * orientation-0 shape).  One ensemble is: mz_ensemble_add for each pass result in call order, the first with first != 0; then
 * mz_ensemble_finish.
 *
 * mz_ensemble_add      y is a view of a pass result in ITS orientation: [B,3,W,H] when k & 4, else [B,3,H,W].  acc (+)= value(T(y,
 *                      inverse(k))); first != 0 stores instead of adding, so the workspace may hold anything beforehand, NaN bytes included.
 * mz_ensemble_finish   out, a view of the window {y0, x0, h, w} of the [B,3,H,W] result (or of all of it when window is NULL; as for
 *                      mz_resize), receives the mean of the n = 1, 2, 4 or 8 results added.
 *
 * The arithmetic, fixed so that a torch restatement gives the same bits.  Float types: value = the element as float32; the accumulator is
 * float32, acc_0 = v_0, acc_i = acc_(i-1) + v_i in call order; finish = acc * (1.0f / n) (exact: n is a power of two), then the clamp to
 * [0, 1] when clamp != 0, then one rounding to the stored type.  uint8: value = the raw sample 0..255 as float32 (not v / 255: sums up to
 * 2040 are exact integers); finish = (2 sum + n) / (2 n) in integer arithmetic, which rounds half up; clamp has nothing to do.
 *
 * Both refuse the view refusals above (elem outside 0..3; y is only read, out is written), and: B < 1 or > 65535; H or W < 1 or > 2^28;
 * an accumulator beyond 2^62 bytes; a view whose byte range overlaps the accumulator's or does not fit in signed 64-bit addresses;
 * mz_ensemble_add: k outside 0..7; mz_ensemble_finish: n outside {1, 2, 4, 8}.  A null or short workspace is MZ_ERR_WORKSPACE_TOO_SMALL. */
/* Host only: inverse(k), negative outside 0..7. */
int mz_dihedral_inverse(int k);
int mz_dihedral(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int k, void* hip_stream);
/* Host only. */
int mz_ensemble_workspace_bytes(int B, int H, int W, size_t* bytes);
int mz_ensemble_add(const mz_image_view* y, int elem, int B, int H, int W, int k, int first, void* workspace, size_t workspace_bytes,
                    void* hip_stream);
int mz_ensemble_finish(const mz_image_view* out, int elem, int B, int H, int W, int n, int clamp, const int32_t window[4],
                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- images with an alpha channel: no reference counterpart (the reference's `decode_image(mode="RGB")` drops alpha).  In a straight-alpha
 *      image the colour under a == 0 is arbitrary, and the model's receptive field (hundreds of low-resolution pixels) pulls it into every
 *      visible edge.  mz_alpha_fill extrapolates the visible colour over the WHOLE transparent region by a push-pull pyramid; mz_alpha_merge
 *      enlarges the alpha plane with the bits of the model's own skip and premultiplies the result if asked
 *      (ultrazoom_amd/alpha.py: alpha_fill, alpha_merge, upscale_rgba; MewZoom.upscale_rgba) --------------------------------------------
 * Stateless like mz_resize: every call enqueues on the given stream, never synchronises, allocates nothing and uses no atomics.  All views
 * of a call have one element type, elem 0..2 = mz_dtype, 3 = uint8.  `alpha` and `out_alpha` are ONE-channel views: their channel stride
 * names nothing (as for mz_luma's output).  The rgb and alpha of an interleaved RGBA buffer are two views with the same strides and data
 * pointers three elements apart: nothing is copied on either side.  The touch contract of the workspace paragraph above holds.
 * ultrazoom_amd/csrc/mz_alpha.h is the one statement of the arithmetic (float64, fixed order, stored components rounded once); in short:
 *
 * mz_alpha_fill   a = the alpha element clamped to [0, 1] (NaN: 0); c = the colour (premultiplied != 0: clamp(p / a, 0, 1)).  Texels
 *                 (w, r, g, b) = (a, a c) -- exactly zero where a == 0, by a select: the colour elements there are never used
 *                 arithmetically, whatever they hold -- are summed 2 x 2 down to 1 x 1 (a sum with w > 1 is divided by w) and pulled back
 *                 up: texel' = texel + (1 - w) U, U the bilinear 2x enlargement of the pulled coarser level.  out: pixels with a > 0 keep
 *                 their elements bit for bit (premultiplied: c rounded once); pixels with a == 0 get rgb' / w' clamped to [0, 1], 0 where
 *                 the image has no visible pixel.  The workspace holds the levels from 1 up, 16 bytes a texel.
 * mz_alpha_merge  out_alpha [B,1,Hout,Wout] = the alpha plane [B,1,Hin,Win] interpolated as mz_interpolate does (mode 0..2), clamped to
 *                 [0, 1] (nearest moves elements): the bits of mz_interpolate(clamp = 1) on that plane.  premultiply != 0: out_rgb = rgb *
 *                 A, in float64, rounded once, A the out_alpha element AS STORED; out_rgb may be exactly the rgb view (in place), any
 *                 other overlap of the two is the caller's responsibility.  premultiply == 0: rgb and out_rgb are not looked at (NULL).
 *
 * Both refuse the view refusals above (elem outside 0..3; rgb and alpha are only read), and: B < 1 or > 65535; a size < 1 or > 2^28.
 * mz_alpha_fill: a pyramid beyond 2^62 bytes; out whose byte range overlaps that of rgb or alpha; a null or short workspace
 * (MZ_ERR_WORKSPACE_TOO_SMALL).  mz_alpha_merge: a mode outside 0..2; alpha whose byte range overlaps that of out_alpha or out_rgb. */
/* Host only. */
int mz_alpha_fill_workspace_bytes(int B, int H, int W, size_t* bytes);
int mz_alpha_fill(const mz_image_view* rgb, const mz_image_view* alpha, const mz_image_view* out, int elem, int B, int H, int W,
                  int premultiplied, void* workspace, size_t workspace_bytes, void* hip_stream);
int mz_alpha_merge(const mz_image_view* rgb, const mz_image_view* alpha, const mz_image_view* out_rgb, const mz_image_view* out_alpha,
                   int elem, int B, int Hin, int Win, int Hout, int Wout, int mode, int premultiply, void* hip_stream);
/* Host only: the level count of the pyramid of an H x W image (level 0 = H x W down to 1 x 1); the sizes of the first min(count, cap)
 * levels as hw[2 l] = H_l, hw[2 l + 1] = W_l.  Negative on bad arguments. */
int mz_debug_alpha_levels(int H, int W, int* hw, int cap);   /* the level count and the sizes of the pyramid */

/* ---- feathered tiling: no reference counterpart (the reference has no tiling code).  Tiles cut with a SMALL halo do not agree where
 *      they meet; each tile keeps a band beyond every interior cut and the later tile is pasted onto the earlier one with a linear
 *      cross-fade over the band (ultrazoom_amd/tiling.py: plan_feathered, upscale_feathered, feather_paste; MewZoom.upscale_feathered) ---
 * Stateless like mz_resize: the call enqueues on the given stream, never synchronises, allocates nothing, needs no workspace and uses no
 * atomics.  src and dst are views of [B,3,H,W] of one element type, elem 0..2 = mz_dtype, 3 = uint8.  All element offsets are 64-bit.
 * The touch contract of the workspace paragraph above holds: src is only read, and of dst only the elements under a ramp are read.
 * ultrazoom_amd/csrc/mz_feather.h is the one statement of the arithmetic; in short:
 *
 * mz_feather_paste  A ramp of n positions has the weights omega(n, k) = (2 k + 1) * rho(n) for k < n, rho(n) = 1.0 / (2 n) formed on
 *                   the host, and omega = 1 for k >= n or n == 0: the midpoints of n equal steps, below 1 for every k < n.  Element
 *                   (y, x) has w = omega(ramp_y, y) * omega(ramp_x, x).  Where w == 1, or src and dst hold the same bit pattern, dst
 *                   receives the BITS of src (a select: a NaN, a -0 or uninitialised bytes of dst under w == 1 change nothing).
 *                   Elsewhere v = d + w * (s - d) in float64, contraction off, rounded once to the element type, no clamp; uint8: s and
 *                   d are the codes 0..255, the stored code is (int)(v + 0.5).  A ramp longer than the rectangle is cut by its border.
 *
 * Refuses the view refusals above (elem outside 0..3; dst is written), and: B < 1 or > 65535; H or W < 1 or > 2^28; src and dst whose
 * byte ranges overlap (the same view twice included) or do not fit in signed 64-bit addresses; a ramp outside 0 .. 2^20. */
int mz_feather_paste(const mz_image_view* src, const mz_image_view* dst, int elem, int B, int H, int W, int ramp_y, int ramp_x,
                     void* hip_stream);
/* Host only: omega(n, k) for 0 <= n <= 2^20 and k >= 0. */
int mz_debug_feather_weight(int n, int k, double* w);

/* ---- introspection ------------------------------------------------------------------------ */
const char* mz_last_error(void);
const char* mz_version(void);
/* Algorithmic FLOPs (2 x conv MACs) of one forward on an H x W image. */
double mz_flops_per_image(const mz_handle* h, int H, int W);
/* Enables per-kernel HIP-event timing for bench.py's live roofline leg: after a forward, returns the
 * accumulated device time (ms) and FLOPs of all conv3x3 implicit-GEMM launches since the last reset. */
int mz_profile_enable(mz_handle* h, int on);
/* Writes one CSV row per profiled launch (layer shape, device ms, TFLOP/s) — tuning aid. */
int mz_profile_dump(mz_handle* h, const char* path);
int mz_profile_read(mz_handle* h, double* conv_ms, double* conv_flops, double* conv_launches,
                    double* other_ms, double* conv_bytes);

/* Diagnostics only: copies the in-kernel cycle-stamp buffer (16 x 64 x 8 uint64) to the host.  The buffer exists only
 * when the process was started with MZ_DEBUG_STAMPS=1 and is written only by -DMZ_STAMP builds of the kernels
 * (tools/stamp_probe*.py); returns -1 when it does not exist.  No reference counterpart. */
int mz_debug_read(unsigned long long* host_dst);

/* Kernel family of the calling thread's most recent convolution / mix launch ("conv3r", "conv3r_8x40", "conv3r_fused", "conv3t",
 * "conv3t_fused", "conv3r_ragged", "conv3s", "conv3s_fused", "conv3p", "conv3w", "conv3w_fused", "conv_kernel", "mix16", "mix16b",
 * "conv_kernel_mix"): lets a test that compares two kernels assert that it really ran both.  No reference counterpart. */
const char* mz_debug_last_kernel(void);

/* Host-only (no GPU): the tile list the role-alternating 3x3 kernels (conv3r / conv3t) walk -- B images of tiles_y x tiles_x pixel tiles
 * of th x tw pixels, ntiles N tiles, in groups of gm pixel tiles x gn N tiles (blk4 != 0: the tiles of an image in block rows of four
 * tile rows).  Entry i = out[2 i], out[2 i + 1] = {y0 | x0 << 16, image | N tile << 16}; at most `cap` entries are written.  Returns the
 * number of tiles listed (== B * tiles_y * tiles_x * ntiles), negative on bad arguments.  No reference counterpart. */
int mz_debug_tile_list(int B, int tiles_y, int tiles_x, int ntiles, int gm, int gn, int blk4, int th, int tw, unsigned int* out, int cap);

/* Host-only (no GPU): the kernel family (a name as mz_debug_last_kernel() reports it) that a launch of one layer would run on a device
 * with `cus` compute units, under the MZ_* knobs of the environment.  op: 0 conv1 + SiLU, 1 plain conv3x3,
 * 2 conv3x3 + PixelShuffle(2) into 2H x 2W (cout = 4 x the shuffled channels), 3 image head (cout = 12), 4 quality-head conv,
 * 5 FiLM conv (mz_op_conv_film), 6 a block's conv2 (cin = the hidden channels) as mz_forward runs it: fused with the mix, or alone,
 * 7 the unfused AdaptiveResidualMix (cin = 2 cout).  Returns NULL where the launch would be refused (mz_last_error() says why).
 * No reference counterpart. */
const char* mz_debug_select(int dtype, int op, int cin, int cout, int B, int H, int W, int cus);

/* One step of a forward pass (mz_debug_schedule).  kind: 0 stem, 1 conv3x3, 2 AdaptiveResidualMix, 3 PixelCrush, 4 zero border of an
 * up-sampled tensor, 5 quality-head reduction.  op: mz_debug_select()'s op of a kind 1 / 2 step, else -1.  H x W: the input's pixels;
 * Hout x Wout: the output's where they differ (ops 2 and 3, kinds 3 and 4), else 0.  fused: a block's conv2 with the mix in its epilogue.
 * Operand j = 0 first input, 1 second input (the block input of a fused conv2, z of a mix, the low-resolution image of the image head),
 * 2 output: off[j] = its byte offset in the workspace, or -1 none, -2 the input image, -3 the output image, -4 the quality output;
 * bytes[j] = its extent (the images: as dense tensors of the handle's dtype).  kernel: the family a kind 1 / 2 step runs on, as
 * mz_debug_select() names it; NULL for the other kinds. */
typedef struct mz_debug_step {
    int32_t kind, op, cin, cout, B, H, W, Hout, Wout, fused;
    int64_t off[3];
    uint64_t bytes[3];
    const char* kernel;
} mz_debug_step;

/* Host-only (no GPU, no weights): the steps mz_forward launches for ONE micro-batch of B images of H x W pixels, in launch order, under
 * the knobs the handle read when it was created, on a device of `cus` compute units; want_qa = 0: as upscale() runs it (out_qa NULL).
 * At most `cap` steps are written to out.  Returns the number of steps, negative on bad arguments.  No reference counterpart. */
int mz_debug_schedule(const mz_handle* h, int B, int H, int W, int want_qa, int cus, mz_debug_step* out, int cap);

/* Host-only (no GPU): one packing of one layer's weights as the library plans and packs it.  dtype, op, cin, cout as for
 * mz_debug_select(), and op 8 = the gate weights of a block's mix, packed for the fused conv2 + mix (cin, cout: those of conv2).
 * layout: 0 the 32x32-MFMA packing every layer has, 1 3x3 for conv3s / conv3r, 2 mix16, 3 conv3s's fused gate, 4 mix16b,
 * 5 conv3r's fused gate, 6 3x3 for conv3t, 7 conv3t's fused gate (PackLayout, ultrazoom_amd/csrc/mz_kernels.h).  Element i of the
 * packing holds weight out[i] of the float32 [cout][cin][kh][kw] tensor, -1 = a zero of the padding; at most `cap` entries are
 * written.  Returns the number of elements, negative where the layer does not have that packing (mz_last_error() says so) or on bad
 * arguments.  No reference counterpart. */
long long mz_debug_pack(int dtype, int op, int cin, int cout, int layout, long long* out, long long cap);

/* Hardware probe (ultrazoom_amd/csrc/mz_probe.hip; tests/test_store_hazard_gpu.py): on every CU, 16-byte buffer stores each followed --
 * `wait_states` (0, 1, 2) wait states later -- by a vector instruction that overwrites data register `dword` (0..3) of the store:
 * follower 0 v_mov_b32, 1 v_mul_f32, 2 v_cvt_pk_bf16_f32, 3 v_exp_f32, 4 v_pk_mul_f32, 5 v_mfma_f32_16x16x32_bf16;
 * form 0 = buffer_store_dwordx4 with soffset 0, 1 = ... with soffset in an SGPR, 2 = global_store_dwordx4 with a 64-bit vaddr, 3 = ... with
 * saddr.  `iters` (a multiple of 8) stores per wave,
 * `blocks` workgroups of four waves.  counts_out[0] = 16-byte entries that reached memory with anything but the register contents at
 * issue, counts_out[1..4] = per dword.  Returns 0, negative on bad arguments / HIP errors.  No reference counterpart. */
int mz_debug_store_hazard(int follower, int form, int wait_states, int dword, int iters, int blocks, unsigned int* counts_out);

#ifdef __cplusplus
}
#endif
#endif /* MEWZOOM_HIP_H */
