// Operator-level entry points of libmewzoom_hip.so (the mz_op_* of include/mewzoom_hip.h): one layer of the model on tensors the caller
// names, planned, chosen and launched as mz_forward does it (the role functions of mz_select.h, the Runner of mz_runner.h).  For tests.
#include "mz_runner.h"

using namespace mz;

extern "C" int mz_padded_channels(int c) { return pad16(c); }

// What an mz_op_* entry runs its layer on, built after the entry's own argument checks: a launch context of its own -- the zero page, the
// knobs read now -- and a Runner on it.  rc says whether making the context, then pack() of a layer's weights, worked; an entry returns it
// where it is set, before it touches run (which exists either way).  finish() waits for the stream and gives the entry's return code.
struct OpRun {
    LaunchCtx ctx;
    int rc;
    Runner run;
    OpRun(int dtype, void* hip_stream) : rc(ctx.init((hipStream_t)hip_stream)), run{ctx, (hipStream_t)hip_stream, dtype} {}
    int pack(ConvW& c, const float* w_dev_f32) { return rc = rc ? rc : pack_conv(c, run.dtype, w_dev_f32, run.s); }
    // the entry's return code: a failed wait for the stream is reported ahead of the Runner's own code
    int finish() { HIPCHK(hipStreamSynchronize(run.s)); return run.rc; }
};

extern "C" int mz_op_conv(int dtype, int kind, const void* in0, const void* in1, const float* w_dev_f32, float alpha,
                          void* out, int B, int H, int W, int cin, int cout, int Hout, int Wout, int silu,
                          void* hip_stream) {
    if (int rc = device_cus(); rc < 0) return rc;
    ConvW c;
    switch (kind) {
        case 0: plan_conv(c, dtype, MODE_CONV3, cout, cin, 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0); break;
        case 1: plan_conv(c, dtype, MODE_CONV3, cout, cin, 3, 3, OUT_D2S, SRC_PLAIN, 0, 0); break;
        case 2: plan_conv(c, dtype, MODE_GEMM1, cout, cin, 2, 2, OUT_PLAIN, SRC_CRUSH, 0, 0); break;
        case 3: plan_conv(c, dtype, MODE_GEMM1, cout, 2 * cout, 1, 1, OUT_PLAIN, SRC_CONCAT, cout, cout); break;
        default: return fail(MZ_ERR_INVALID_ARGUMENT, "bad op kind %d", kind);
    }
    OpRun op(dtype, hip_stream);
    if (op.pack(c, w_dev_f32)) return op.rc;
    Runner& run = op.run;
    switch (kind) {
        case 0: run.conv3(silu ? conv1_call(c, in0, out, B, H, W) : plain_call(c, in0, out, B, H, W)); break;
        case 1:
            run.conv3(d2s_call(c, in0, out, B, H, W, Hout, Wout));
            if (!run.rc) run.rc = hip_rc(launch_zero_border(dtype, out, B, Hout, Wout, c.cq_p, 2 * H, 2 * W, run.s), "zero border");
            break;
        case 2: run.crush(c, in0, out, B, H, W); break;
        case 3: run.mix(c, alpha, in0, in1, out, B, H, W); break;
    }
    return op.finish();
}

// conv2 of a block + AdaptiveResidualMix with the block input in ONE launch (model.py:773-778 second half, 826-839): the fused
// kernels of the 16-bit modes (conv3r_kernel / conv3s_kernel / conv3w_kernel with FUSE), for C <= 96.
//   hid [B, cin, H, W] (conv1's activated output), x [B, cout, H, W] (the block input), w2 [cout, cin, 3, 3], wmix [cout, 2 cout, 1, 1]
extern "C" int mz_op_conv_mix(int dtype, const void* hid, const void* x, const float* w2_dev_f32, const float* wmix_dev_f32, float alpha,
                              void* out, int B, int H, int W, int cin, int cout, void* hip_stream) {
    if (int rc = device_cus(); rc < 0) return rc;
    if (!hid || !x || !w2_dev_f32 || !wmix_dev_f32 || !out) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    BlockW b;
    plan_block(b, dtype, cout, cin);
    if (!b.fused) return fail(MZ_ERR_INVALID_ARGUMENT, "the fused conv2 + mix needs all output channels in one N tile (cout <= 96)");
    b.alpha = alpha;  // (nobody set this block's skip.alpha)
    OpRun op(dtype, hip_stream);
    if (op.pack(b.conv2, w2_dev_f32) || op.pack(b.mixf, wmix_dev_f32)) return op.rc;
    op.run.conv3(fused_call(b, hid, x, out, B, H, W));  // whatever MZ_NO_FUSE / MZ_NO_WIDE say: this entry IS the fused launch
    return op.finish();
}

// a17: conv3x3 -> gamma[b, c] * y + beta[b, c] -> optional SiLU, the per-channel modulation of a FiLM /
// control module.  The reference snapshot has no such module (README.md:86-129 describes library version 0.2.x): nothing to
// be parity-checked against, so this operator is checked against the build's own CPU restatement only ("parity unpinned").
extern "C" int mz_op_conv_film(int dtype, const void* in0, const float* w_dev_f32, const float* gamma_dev_f32,
                               const float* beta_dev_f32, void* out, int B, int H, int W, int cin, int cout, int silu,
                               void* hip_stream) {
    if (int rc = device_cus(); rc < 0) return rc;
    if (!in0 || !w_dev_f32 || !gamma_dev_f32 || !beta_dev_f32 || !out) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (dtype != DT_BF16 && dtype != DT_F16) return fail(MZ_ERR_INVALID_ARGUMENT, "the FiLM epilogue is implemented for bf16 / fp16");
    ConvW c;
    plan_conv(c, dtype, MODE_CONV3, cout, cin, 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0);
    OpRun op(dtype, hip_stream);
    if (op.pack(c, w_dev_f32)) return op.rc;
    // gamma / beta [B][cout] -> [B][padded cout], pad channels zero
    const int cp = pad16(cout);
    DevBuf gpad, bpad;
    HIPCHK(gpad.alloc(sizeof(float) * (size_t)B * cp));
    HIPCHK(bpad.alloc(sizeof(float) * (size_t)B * cp));
    HIPCHK(hipMemsetAsync(gpad.p, 0, sizeof(float) * (size_t)B * cp, op.run.s));
    HIPCHK(hipMemsetAsync(bpad.p, 0, sizeof(float) * (size_t)B * cp, op.run.s));
    HIPCHK(hipMemcpy2DAsync(gpad.p, sizeof(float) * cp, gamma_dev_f32, sizeof(float) * cout, sizeof(float) * cout, B, hipMemcpyDeviceToDevice, op.run.s));
    HIPCHK(hipMemcpy2DAsync(bpad.p, sizeof(float) * cp, beta_dev_f32, sizeof(float) * cout, sizeof(float) * cout, B, hipMemcpyDeviceToDevice, op.run.s));
    Conv3Call k = film_call(c, in0, out, B, H, W, silu);
    k.gamma = (const float*)gpad.p; k.beta = (const float*)bpad.p;
    op.run.conv3(k);
    return op.finish();
}

extern "C" int mz_op_stem(int dtype, const void* x, const float* w_dev_f32, const float* b_dev_f32, void* out, int B,
                          int H, int W, int cout, void* hip_stream) {
    if (int rc = device_cus(); rc < 0) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const int cp = pad16(cout);
    DevBuf w4;
    HIPCHK(w4.alloc(sizeof(float) * 4 * cp));
    HIPCHK(hipMemsetAsync(w4.p, 0, sizeof(float) * 4 * cp, s));
    HIPCHK(launch_pack_stem(w_dev_f32, b_dev_f32, (float*)w4.p, cout, cp, s));
    HIPCHK(launch_stem(dtype, x, (const float*)w4.p, out, B, H, W, cp, s));
    HIPCHK(hipStreamSynchronize(s));
    return MZ_OK;
}

extern "C" int mz_op_final(int dtype, const void* feat, const void* img, const float* w_dev_f32, void* out, int B, int H,
                           int W, int cin, int R, int clamp, void* hip_stream) {
    if (int rc = device_cus(); rc < 0) return rc;
    ConvW c;
    plan_conv(c, dtype, MODE_CONV3, 12, cin, 3, 3, OUT_FINAL, SRC_PLAIN, 0, 0);
    OpRun op(dtype, hip_stream);
    if (op.pack(c, w_dev_f32)) return op.rc;
    Conv3Call k = head_call(c, feat, out, B, H, W);
    k.img = img; k.R = R; k.clamp = clamp;
    op.run.conv3(k);
    return op.finish();
}
