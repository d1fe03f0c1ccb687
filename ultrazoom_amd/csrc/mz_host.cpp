// Model runtime of libmewzoom_hip.so: configuration checks, weight registry + packing, running the schedule of the MewZoom forward pass,
// the profiler, and their part of the C ABI (include/mewzoom_hip.h).  Planning, kernel selection and the schedule: mz_plan.h, mz_select.h,
// mz_schedule.h; launching a layer: mz_runner.h; the mz_op_* entries: mz_ops.cpp; metrics, resize, degradations: mz_image.cpp;
// introspection: mz_debug.cpp.
#include <cstdio>

#include "mz_host.h"

using namespace mz;

// ------------------------------------------------------------------------------------------------
// model description
// ------------------------------------------------------------------------------------------------
// Registers a parameter under its state_dict name; returns its slot for the caller to name what receives the value
static Slot& add_slot(mz_handle* h, const std::string& name, int kind, std::initializer_list<int64_t> shape) {
    Slot s;
    s.name = name;
    s.kind = kind;
    s.ndim = (int)shape.size();
    int i = 0;
    for (auto d : shape) s.shape[i++] = d;
    h->slot_index[name] = (int)h->slots.size();
    h->slots.push_back(s);
    return h->slots.back();
}
// the weight of a planned layer (also: a second layer packed from the same weight, a fused block's gate)
static void add_conv_slot(mz_handle* h, const std::string& name, ConvW& c, ConvW* also = nullptr) {
    Slot& s = add_slot(h, name, SK_CONV, {c.cout, c.cin, c.kh, c.kw});
    s.conv = &c;
    s.also = also;
}
static void add_alpha_slot(mz_handle* h, const std::string& name, float* alpha) { add_slot(h, name, SK_ALPHA, {}).alpha = alpha; }

static void add_block_slots(mz_handle* h, BlockW& b, const std::string& prefix) {
    add_conv_slot(h, prefix + ".convnet.conv1.weight", b.conv1);
    add_conv_slot(h, prefix + ".convnet.conv2.weight", b.conv2);
    add_alpha_slot(h, prefix + ".skip.alpha", &b.alpha);  // a module's own parameters precede its children's
    add_conv_slot(h, prefix + ".skip.conv.weight", b.mix, b.fused ? &b.mixf : nullptr);
}

static int validate(const mz_config& c) {
    // Same rejected values as the reference constructor (AssertionError there).
    if (!(c.upscale_ratio == 2 || c.upscale_ratio == 4 || c.upscale_ratio == 8))  // model.py:67-69
        return fail(MZ_ERR_INVALID_ARGUMENT, "Upscale ratio must be one of {2, 4, 8}, but got %d.", c.upscale_ratio);
    if (c.primary_channels <= 3)  // model.py:218-222
        return fail(MZ_ERR_INVALID_ARGUMENT, "Output channels must be greater than input channels.");
    const int ch[4] = {c.primary_channels, c.secondary_channels, c.tertiary_channels, c.quaternary_channels};
    const int ly[4] = {c.primary_layers, c.secondary_layers, c.tertiary_layers, c.quaternary_layers};
    const char* nm[4] = {"primary", "secondary", "tertiary", "quaternary"};
    for (int i = 0; i < 4; ++i) {
        if (ly[i] <= 1)  // model.py:265-275
            return fail(MZ_ERR_INVALID_ARGUMENT, "Number of %s layers must be greater than 1.", nm[i]);
        if (ch[i] <= 0) return fail(MZ_ERR_INVALID_ARGUMENT, "Number of channels must be greater than 0.");  // :737
    }
    if (!(c.hidden_ratio == 1 || c.hidden_ratio == 2 || c.hidden_ratio == 4))  // model.py:738
        return fail(MZ_ERR_INVALID_ARGUMENT, "Hidden ratio must be either 1, 2, or 4.");
    if (c.num_deg_features <= 0)  // model.py:356-358 (intent)
        return fail(MZ_ERR_INVALID_ARGUMENT, "Number of quality assessor features must be greater than 0.");
    return MZ_OK;
}

extern "C" int mz_create(const mz_config* cfg, int dtype, mz_handle** out) {
    if (!cfg || !out) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (dtype != MZ_F32 && dtype != MZ_BF16 && dtype != MZ_F16) return fail(MZ_ERR_INVALID_ARGUMENT, "bad dtype %d", dtype);
    if (int rc = validate(*cfg)) return rc;
    auto* h = new mz_handle();
    h->cfg = *cfg;
    const int ch[4] = {cfg->primary_channels, cfg->secondary_channels, cfg->tertiary_channels, cfg->quaternary_channels};
    const int ly[4] = {cfg->primary_layers, cfg->secondary_layers, cfg->tertiary_layers, cfg->quaternary_layers};
    const int nhead = cfg->upscale_ratio == 2 ? 1 : (cfg->upscale_ratio == 4 ? 2 : 3);  // model.py:945
    h->dims = {dtype, {ch[0], ch[1], ch[2], ch[3]}, cfg->hidden_ratio, nhead, cfg->num_deg_features};
    Model<ConvW>& m = h->model;
    plan_model(m, h->dims, ly);

    // Registry: the planned layers by their names, in the reference's state_dict order.
    const auto n = [](int i) { return std::to_string(i); };
    h->slots.reserve(1024);
    add_slot(h, "stem.conv.weight", SK_STEM_W, {ch[0], 3, 1, 1});
    add_slot(h, "stem.conv.bias", SK_STEM_B, {ch[0]});
    for (int s = 0; s < 4; ++s)
        for (int i = 0; i < m.enc[s]; ++i) add_block_slots(h, m.enc_blocks[s][i], "unet.encoder.stage" + n(s + 1) + "." + n(i));
    for (int s = 0; s < 3; ++s) add_conv_slot(h, "unet.encoder.downsample" + n(s + 1) + ".conv.weight", m.crush[s]);
    add_conv_slot(h, "unet.encoder.qa_head.conv.weight", m.qa_conv);
    add_slot(h, "unet.encoder.qa_head.conv.bias", SK_QA_B, {cfg->num_deg_features});
    for (int d = 0; d < 4; ++d)  // decoder stage1 = coarsest level (model.py:290-300)
        for (int i = 0; i < m.dec[3 - d]; ++i) add_block_slots(h, m.dec_blocks[d][i], "unet.decoder.stage" + n(d + 1) + "." + n(i));
    for (int d = 0; d < 3; ++d) add_conv_slot(h, "unet.decoder.upsample" + n(d + 1) + ".conv.weight", m.up[d]);
    for (int d = 0; d < 3; ++d) {
        add_alpha_slot(h, "unet.decoder.skip" + n(d + 1) + ".alpha", &m.skip_alpha[d]);
        add_conv_slot(h, "unet.decoder.skip" + n(d + 1) + ".conv.weight", m.skipmix[d]);
    }
    for (int i = 0; i < nhead; ++i) {  // model.py:945-954, 981-983
        add_block_slots(h, m.head_blocks[i], "head.layers." + n(i) + ".refiner");
        add_conv_slot(h, "head.layers." + n(i) + ".upscale.conv.weight", m.head_up[i]);
    }
    *out = h;
    return MZ_OK;
}

extern "C" int mz_destroy(mz_handle* h) {
    delete h;
    return MZ_OK;
}

extern "C" int mz_num_weights(const mz_handle* h) { return h ? (int)h->slots.size() : 0; }

extern "C" int mz_weight_info(const mz_handle* h, int index, const char** name, int64_t shape[4]) {
    if (!h || index < 0 || index >= (int)h->slots.size()) return fail(MZ_ERR_INVALID_ARGUMENT, "bad weight index");
    const Slot& s = h->slots[index];
    if (name) *name = s.name.c_str();
    if (shape)
        for (int i = 0; i < 4; ++i) shape[i] = s.shape[i];
    return s.ndim;
}

// the handle's buffers, on the first weight that is set
static int prepare_device(mz_handle* h, hipStream_t st) {
    if (h->qa_bias.p) return MZ_OK;  // the last of them
    if (int rc = device_cus(); rc < 0) return rc;
    if (int rc = h->ctx.init(st)) return rc;  // zero fills go to the CALLER's stream (LaunchCtx::init says why)
    const int cp0 = pad16(h->dims.ch[0]);
    HIPCHK(h->stem_w4.alloc(sizeof(float) * 4 * cp0));
    HIPCHK(hipMemsetAsync(h->stem_w4.p, 0, sizeof(float) * 4 * cp0, st));
    HIPCHK(h->qa_bias.alloc(sizeof(float) * std::max(1, h->cfg.num_deg_features)));
    return MZ_OK;
}

// the slot's value into what the forward pass reads
static int load_slot(mz_handle* h, const Slot& s, const float* dev_f32, hipStream_t st) {
    const int c0 = h->dims.ch[0];
    switch (s.kind) {
        case SK_CONV:
            if (int rc = pack_conv(*s.conv, h->dims.dtype, dev_f32, st)) return rc;
            return s.also ? pack_conv(*s.also, h->dims.dtype, dev_f32, st) : MZ_OK;
        case SK_ALPHA:
            // sigmoid(alpha) is folded on the host (model.py:833); one 4-byte read at load time.
            HIPCHK(hipMemcpyAsync(s.alpha, dev_f32, sizeof(float), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            return MZ_OK;
        case SK_STEM_W: HIPCHK(launch_pack_stem(dev_f32, nullptr, (float*)h->stem_w4.p, c0, pad16(c0), st)); return MZ_OK;
        case SK_STEM_B: HIPCHK(launch_pack_stem(nullptr, dev_f32, (float*)h->stem_w4.p, c0, pad16(c0), st)); return MZ_OK;
        case SK_QA_B:
            HIPCHK(hipMemcpyAsync(h->qa_bias.p, dev_f32, sizeof(float) * h->cfg.num_deg_features, hipMemcpyDeviceToDevice, st));
            return MZ_OK;
    }
    return fail(MZ_ERR_INVALID_ARGUMENT, "bad slot");
}

extern "C" int mz_set_weight(mz_handle* h, const char* name, const float* dev_f32, const int64_t* shape, int ndim,
                             void* hip_stream) {
    if (!h || !name || !dev_f32) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    auto it = h->slot_index.find(name);
    if (it == h->slot_index.end()) return fail(MZ_ERR_UNKNOWN_WEIGHT, "unknown parameter '%s'", name);
    Slot& s = h->slots[it->second];
    if (ndim != s.ndim) return fail(MZ_ERR_SHAPE_MISMATCH, "'%s': expected %d dims, got %d", name, s.ndim, ndim);
    for (int i = 0; i < ndim; ++i)
        if (shape[i] != s.shape[i])
            return fail(MZ_ERR_SHAPE_MISMATCH, "'%s': dim %d is %lld, expected %lld", name, i, (long long)shape[i], (long long)s.shape[i]);
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = prepare_device(h, st);
    if (rc) return rc;
    rc = load_slot(h, s, dev_f32, st);
    if (rc == MZ_OK) s.set = true;
    return rc;
}

extern "C" int mz_weights_complete(const mz_handle* h) {
    if (!h) return fail(MZ_ERR_INVALID_ARGUMENT, "null handle");
    for (const Slot& s : h->slots)
        if (!s.set) return fail(MZ_ERR_MISSING_WEIGHTS, "parameter '%s' has not been set", s.name.c_str());
    return MZ_OK;
}

extern "C" int mz_workspace_bytes(const mz_handle* h, int B, int H, int W, int max_images_in_flight, size_t* bytes) {
    if (!h || !bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (B <= 0 || H < 8 || W < 8) return fail(MZ_ERR_INVALID_ARGUMENT, "need B >= 1 and H, W >= 8 (got %d, %d, %d)", B, H, W);
    Plan p;
    make_plan(h->dims, default_micro_batch(h->dims, B, H, W, max_images_in_flight), H, W, p);
    *bytes = p.total;
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// One micro-batch: the steps of make_schedule (mz_schedule.h), their operands resolved against the workspace and the caller's tensors.
// views: x and out_sr are the first elements of image views (out_sr: of the window) instead of dense NCHW tensors
static int forward_micro(mz_handle* h, const char* x, char* out_sr, float* out_qa, int nb, int H, int W, int clamp,
                         char* ws, hipStream_t s, int io_u8, const ImageViews* views) {
    Plan p;
    make_plan(h->dims, nb, H, W, p);
    Runner run{h->ctx, s, h->dims.dtype};
    run.io_u8 = io_u8;
    const int dtype = h->dims.dtype;
    auto at = [&](const BufRef& b) -> char* {
        switch (b.where) {
            case BUF_WS: return ws + b.off;
            case BUF_IMAGE_IN: return const_cast<char*>(x);
            case BUF_IMAGE_OUT: return out_sr;
            case BUF_QA_OUT: return (char*)out_qa;
        }
        return nullptr;
    };
    for (const Step<ConvW>& st : make_schedule(h->model, h->dims, p, run.knobs, out_qa != nullptr, h->cfg.upscale_ratio, clamp)) {
        const char *in = at(st.in), *in1 = at(st.in1);
        char* out = at(st.out);
        switch (st.kind) {
            case ST_CONV3: {
                Conv3Call c = step_call(run.knobs, st, in, in1, out);
                if (st.role == ROLE_HEAD) c.views = views;
                run.conv3(c);
                break;
            }
            case ST_MIX: run.mix(*st.layer, st.alpha, in, in1, out, st.B, st.H, st.W); break;
            case ST_CRUSH: run.crush(*st.layer, in, out, st.B, st.H, st.W); break;
            case ST_STEM:
                if (int rc = hip_rc(launch_stem(dtype, in, (const float*)h->stem_w4.p, out, st.B, st.H, st.W, pad16(st.cout), s, io_u8, views ? views->in : nullptr), "stem launch"))
                    return rc;
                break;
            case ST_ZERO_BORDER:
                if (run.rc) return run.rc;
                if (int rc = hip_rc(launch_zero_border(dtype, out, st.B, st.Hout, st.Wout, st.layer->cq_p, 2 * st.H, 2 * st.W, s), "zero border launch"))
                    return rc;
                break;
            case ST_QA_REDUCE:
                if (run.rc) return run.rc;
                if (int rc = hip_rc(launch_qa_reduce(dtype, in, (const float*)h->qa_bias.p, (float*)out, st.B, st.H * st.W, pad16(st.cout), st.cout, s), "qa reduce launch"))
                    return rc;
                break;
        }
    }
    return run.rc;
}

static int forward_impl(mz_handle* h, const void* x, void* out_sr, float* out_qa, int B, int H, int W, int clamp,
                        void* workspace, size_t workspace_bytes, int max_images_in_flight, void* hip_stream, int io_u8,
                        const ImageViews* views = nullptr) {
    if (!h || !x || !out_sr || !workspace) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (B <= 0 || H < 8 || W < 8) return fail(MZ_ERR_INVALID_ARGUMENT, "need B >= 1 and H, W >= 8 (got %d, %d, %d)", B, H, W);
    int rc = mz_weights_complete(h);
    if (rc) return rc;
    const int nbmax = default_micro_batch(h->dims, B, H, W, max_images_in_flight);
    Plan p;
    make_plan(h->dims, nbmax, H, W, p);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, p.total)) return fail(r);
    const size_t sz = io_u8 ? 1 : dtype_size(h->dims.dtype);
    const int r = h->cfg.upscale_ratio;
    // bytes from one image to the next: dense NCHW, or the views' image strides (signed)
    const long long in_img = views ? views->in[0] * (long long)sz : (long long)((size_t)3 * H * W * sz);
    const long long out_img = views ? views->out[0] * (long long)sz : (long long)((size_t)3 * H * r * W * r * sz);
    for (int b0 = 0; b0 < B; b0 += nbmax) {
        const int nb = std::min(nbmax, B - b0);
        rc = forward_micro(h, (const char*)x + b0 * in_img, (char*)out_sr + b0 * out_img,
                           out_qa ? out_qa + (size_t)b0 * h->cfg.num_deg_features : nullptr, nb, H, W, clamp,
                           (char*)workspace, (hipStream_t)hip_stream, io_u8, views);
        if (rc) return rc;
    }
    return MZ_OK;
}

extern "C" int mz_forward(mz_handle* h, const void* x, void* out_sr, float* out_qa, int B, int H, int W, int clamp,
                          void* workspace, size_t workspace_bytes, int max_images_in_flight, void* hip_stream) {
    return forward_impl(h, x, out_sr, out_qa, B, H, W, clamp, workspace, workspace_bytes, max_images_in_flight, hip_stream, 0);
}

extern "C" int mz_forward_u8(mz_handle* h, const uint8_t* x, uint8_t* out_sr, float* out_qa, int B, int H, int W,
                             void* workspace, size_t workspace_bytes, int max_images_in_flight, void* hip_stream) {
    return forward_impl(h, x, out_sr, out_qa, B, H, W, /*clamp (implied by the uint8 store)*/ 1, workspace, workspace_bytes,
                        max_images_in_flight, hip_stream, 1);
}

// Images as views at both ends: every check before the weights check and before any HIP call, so that a bad call is refused on a
// machine without a GPU as well.  mz_forward / mz_forward_u8 are the dense special case and keep their own kernels.
extern "C" int mz_forward_view(mz_handle* h, const mz_image_view* x, const mz_image_view* out, float* out_qa, int B, int H, int W,
                               int clamp, int elem, const int32_t window[4], void* workspace, size_t workspace_bytes,
                               int max_images_in_flight, void* hip_stream) {
    if (!h) return fail(MZ_ERR_INVALID_ARGUMENT, "null handle");
    static const ViewRules rules = {1, "0 (the handle's dtype) or 1 (uint8)", /*second_is_output*/ true, /*batch_bound*/ false, /*side_bound*/ false};
    StridedView xv, ov;
    if (const Refusal r = check_views(x, out, rules, elem, B, H, W, &xv, &ov)) return fail(r);
    if (B <= 0 || H < 8 || W < 8) return fail(MZ_ERR_INVALID_ARGUMENT, "need B >= 1 and H, W >= 8 (got %d, %d, %d)", B, H, W);
    const long long rH = (long long)h->cfg.upscale_ratio * H, rW = (long long)h->cfg.upscale_ratio * W;
    if (rH > 0x7fffffffLL || rW > 0x7fffffffLL) return fail(MZ_ERR_INVALID_ARGUMENT, "the output of %d x %d is too large", H, W);
    ImageViews v;
    if (const Refusal r = check_window(window, (int)rH, (int)rW, &v.y0, &v.x0, &v.h, &v.w)) return fail(r);
    for (int i = 0; i < 4; ++i) {
        v.in[i] = xv.s[i];
        v.out[i] = ov.s[i];
    }
    return forward_impl(h, x->data, out->data, out_qa, B, H, W, elem == 1 ? 1 : clamp, workspace, workspace_bytes,
                        max_images_in_flight, hip_stream, elem, &v);
}

extern "C" int mz_profile_enable(mz_handle* h, int on) {
    if (!h) return fail(MZ_ERR_INVALID_ARGUMENT, "null handle");
    h->ctx.prof = on != 0;
    h->ctx.recs_used = 0;
    return MZ_OK;
}

extern "C" int mz_profile_dump(mz_handle* h, const char* path) {
    // One CSV row per profiled launch since the last reset (does not reset).
    if (!h || !path) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    FILE* f = fopen(path, "w");
    if (!f) return fail(MZ_ERR_INVALID_ARGUMENT, "cannot open %s", path);
    fprintf(f, "kind,B,H,W,cin,cout,nt,ntiles,mtiles,n_fast,ms,gflop,tflops,alg_GBps\n");
    for (size_t i = 0; i < h->ctx.recs_used; ++i) {
        ProfRec& r = h->ctx.recs[i];
        if (hipEventSynchronize(r.b) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
        const char* kn = r.kind == 0 ? "conv3" : (r.kind == 1 ? "mix" : "crush");
        fprintf(f, "%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%.4f,%.3f,%.1f,%.1f\n", kn, r.B, r.H, r.W, r.cin, r.cout, r.nt, r.ntiles,
                r.mtiles, r.n_fast, ms, r.flops / 1e9, r.flops / (ms * 1e-3) / 1e12, r.bytes / (ms * 1e-3) / 1e9);
    }
    fclose(f);
    return MZ_OK;
}

extern "C" int mz_profile_read(mz_handle* h, double* conv_ms, double* conv_flops, double* conv_launches, double* other_ms,
                               double* conv_bytes) {
    if (!h) return fail(MZ_ERR_INVALID_ARGUMENT, "null handle");
    double cm = 0, cf = 0, cl = 0, om = 0, cb = 0;
    for (size_t i = 0; i < h->ctx.recs_used; ++i) {
        ProfRec& r = h->ctx.recs[i];
        HIPCHK(hipEventSynchronize(r.b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        if (r.kind == 0) { cm += ms; cf += r.flops; cl += 1; cb += r.bytes; }
        else om += ms;
    }
    if (conv_ms) *conv_ms = cm;
    if (conv_flops) *conv_flops = cf;
    if (conv_launches) *conv_launches = cl;
    if (other_ms) *other_ms = om;
    if (conv_bytes) *conv_bytes = cb;
    h->ctx.recs_used = 0;
    return MZ_OK;
}
