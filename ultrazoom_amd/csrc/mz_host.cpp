// Host runtime of libmewzoom_hip.so: configuration checks, weight registry + packing, workspace
// planning, the layer schedule of the MewZoom forward pass, and the C ABI (include/mewzoom_hip.h).
//
// The schedule follows the reference's MewZoom.forward (src/ultrazoom/model.py:149-164) and its
// sub-modules; each step cites the reference lines it replaces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mewzoom_hip.h"
#include "mz_geo.h"
#include "mz_metrics.h"
#include "mz_pack.h"
#include "mz_resize.h"
#include "mz_degrade.h"
#include "mz_view_check.h"

using namespace mz;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
// kernel family of this thread's most recent convolution / mix launch (mz_debug_last_kernel(): the tests assert WHICH kernel they compare)
static thread_local const char* g_last_kernel = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int fail(const Refusal& r) { return fail(r.code, "%s", r.msg); }  // what a check of mz_view_check.h refused
#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(MZ_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Per-device state: the CU count (kMaxDevices: mz_kernels.h; the launchers raise their kernels' dynamic-LDS limits themselves)
static int g_dev_ready[kMaxDevices];  // 0 unknown, 1 ok
static int g_dev_cus[kMaxDevices];

static int ensure_device_ready() {
    int n = 0, dev = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MZ_ERR_NO_DEVICE, "no HIP device visible");
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return fail(MZ_ERR_NO_DEVICE, "bad current device");
    if (g_dev_ready[dev] == 1) return MZ_OK;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    g_dev_cus[dev] = cus / 8 * 8;
    g_dev_ready[dev] = 1;
    return MZ_OK;
}

// Environment knobs (A/B timing and test coverage of every kernel variant).  Read ONCE, when a
// handle is created (or per mz_op_* call), never on the launch path.
struct Knobs {
    bool wide = true;       // MZ_NO_WIDE=1: force the 256-pixel kernel
    bool fuse = true;       // MZ_NO_FUSE=1: conv2 and the mix as two launches
    bool s16 = true;        // MZ_NO_S16=1: keep 16-bit types on the 32x32x16 kernels
    bool fuse16 = true;     // MZ_NO_FUSE16=1: the fused mix stays on the 32x32x16 kernel
    bool mix16b = true;     // MZ_NO_MIX16B=1: C = 192 mixes on mix16_kernel (blend in accumulator layout, x and z read twice) instead of mix16b_kernel
    int persist = -1;       // MZ_NO_PERSIST=1 -> 0 (one workgroup per tile); MZ_PERSIST_WGS=n -> n; -1 = one per CU
    int kpad_pct = 12;      // MZ_KPAD_PCT=n: the 16x16x32 kernels take Cin whose padding to whole 32-channel chunks is <= n %
    int blk4 = 1;           // MZ_NO_BLK4=1: row-major tile walk inside an image (A/B of the L2 sharing of vertical halos)
    int r = 1;              // MZ_NO_R=1: never use conv3r_kernel (96-channel N tiles, 8 x 48 / 8 x 40 pixel tiles, role-alternating waves: epilogues under the next K loop)
    int r2 = 1;             // MZ_NO_R2=1: Cin = 48 -> 96-channel N tiles (conv1 of the 48-channel models' level-1 block) stays off conv3r_kernel's ragged variant
    int t = 1;              // MZ_NO_T=1: never use conv3t_kernel (the same structure for ONE N tile of <= 48 channels, 12 x 64 tiles)
};
static Knobs read_knobs() {
    Knobs k;
    k.wide = getenv("MZ_NO_WIDE") == nullptr;
    k.fuse = getenv("MZ_NO_FUSE") == nullptr;
    k.s16 = getenv("MZ_NO_S16") == nullptr;
    k.fuse16 = getenv("MZ_NO_FUSE16") == nullptr;
    k.mix16b = getenv("MZ_NO_MIX16B") == nullptr;
    k.r = getenv("MZ_NO_R") == nullptr;
    k.t = getenv("MZ_NO_T") == nullptr;
    k.r2 = getenv("MZ_NO_R2") == nullptr;
    k.blk4 = getenv("MZ_NO_BLK4") == nullptr;
    if (const char* e = getenv("MZ_KPAD_PCT")) k.kpad_pct = atoi(e);
    if (getenv("MZ_NO_PERSIST") != nullptr) k.persist = 0;
    else if (const char* e = getenv("MZ_PERSIST_WGS")) { const int n = atoi(e) / 8 * 8; k.persist = n > 0 ? n : 0; }
    return k;
}

// ------------------------------------------------------------------------------------------------
// model description
// ------------------------------------------------------------------------------------------------
// A device allocation that frees itself.
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return p ? hipSuccess : hipMalloc(&p, bytes); }  // once: a weight set again is packed in place
};

struct ConvW {
    // logical (reference) shape
    int cout = 0, cin = 0, kh = 0, kw = 0;
    // kernel selection
    int mode = MODE_CONV3, taps = 9, nt = 1, ntiles = 1, nchunks = 1, nchunks_real = 1;
    int out_map = OUT_PLAIN, cq = 0, cq_p = 0;
    int in_map = SRC_PLAIN, c0 = 0, cp0 = 0, c1 = 0;
    int n_logical_padded = 0;
    int nchunks32 = 0;     // 32-channel chunks of in0: the K steps of the 16x16x32 kernels over cp0
    unsigned layouts = 0;  // the planned packings, one bit per PackLayout
    DevBuf packed[PK_COUNT];
    bool set = false;
    bool has(int layout) const { return layouts >> layout & 1u; }
};

// One packing of a layer: fragments per tap and N tile, N tiles, K chunks (PackArgs; ConvArgs::nchunks16 of the 16-bit layouts)
struct PackShape {
    int frags, ntiles, nchunks;
};
static PackShape pack_shape(const ConvW& c, int layout) {
    switch (layout) {
        case PK_MAIN: return {c.nt, c.ntiles, c.nchunks};
        case PK_CONV16: return {2 * c.nt, c.ntiles, c.nchunks32};
        case PK_MIX16: case PK_MIX16B: return {12, c.cout / 192, 2 * c.cout / 32};  // 192-channel N tiles over [x ; z]
        case PK_GATE16: case PK_GATE16R: return {2 * c.nt, 1, c.nchunks32 + c.nt};   // x K steps, then one per pair of z fragments
        case PK_CONV16T: return {3, 1, c.nchunks32};
        default: return {3, 1, 3};  // PK_GATE16T: three K steps x three fragments
    }
}
static size_t pack_bytes(const ConvW& c, int layout) {
    const PackShape sh = pack_shape(c, layout);
    return packed_bytes(c.taps, sh.frags, sh.ntiles, sh.nchunks);
}

static void plan_conv(ConvW& c, int dtype, int mode, int cout, int cin, int kh, int kw, int out_map, int in_map,
                      int c0, int c1) {
    const int ck = chunk_channels(dtype);
    c.cout = cout; c.cin = cin; c.kh = kh; c.kw = kw;
    c.mode = mode;
    c.taps = mode == MODE_CONV3 ? 9 : 1;
    c.out_map = out_map;
    c.in_map = in_map;
    if (out_map == OUT_D2S) {
        c.cq = cout / 4;
        c.cq_p = pad16(c.cq);
        c.n_logical_padded = 4 * c.cq_p;
    } else if (out_map == OUT_FINAL) {
        c.n_logical_padded = 16;
    } else {
        c.n_logical_padded = pad16(cout);
    }
    c.nt = choose_nt(c.n_logical_padded);
    c.ntiles = (c.n_logical_padded + 32 * c.nt - 1) / (32 * c.nt);
    if (in_map == SRC_PLAIN) {
        c.c0 = cin; c.cp0 = pad16(cin); c.c1 = 0;
        c.nchunks = c.cp0 / ck;
    } else if (in_map == SRC_CONCAT) {
        c.c0 = c0; c.cp0 = pad16(c0); c.c1 = c1;
        c.nchunks = (c.cp0 + pad16(c1)) / ck;
    } else {  // CRUSH
        c.c0 = cin; c.cp0 = pad16(cin); c.c1 = 0;
        c.nchunks = 4 * c.cp0 / ck;
    }
    c.nchunks_real = c.nchunks;
    if (mode == MODE_GEMM1) {  // the 1x1 kernel consumes S chunks per stage: pad K with zero weights
        const int S = gemm1_chunks_per_stage();
        c.nchunks = (c.nchunks + S - 1) / S * S;
    }
    c.nchunks32 = (c.cp0 + 31) / 32;
    c.layouts = 1u << PK_MAIN;
    const bool s16 = dtype != DT_F32;
    // wide 3x3 convolutions that are not the image head: the 16x16x32 kernels
    if (mode == MODE_CONV3 && s16 && in_map == SRC_PLAIN && out_map != OUT_FINAL && c.nt <= 3) c.layouts |= 1u << PK_CONV16;
    // one N tile of 33..48 channels over whole 32-channel chunks: conv3t_kernel
    if (mode == MODE_CONV3 && s16 && in_map == SRC_PLAIN && out_map == OUT_PLAIN && c.n_logical_padded == 48 && c.cp0 % 32 == 0)
        c.layouts |= 1u << PK_CONV16T;
    // AdaptiveResidualMix with C = k * 192: mix16_kernel; C = 192: mix16b_kernel too
    if (mode == MODE_GEMM1 && s16 && in_map == SRC_CONCAT && cout % 192 == 0 && c0 == cout && c1 == cout) {
        c.layouts |= 1u << PK_MIX16;
        if (cout == 192) c.layouts |= 1u << PK_MIX16B;
    }
}

struct BlockW {
    ConvW conv1, conv2, mix;
    ConvW mixf;          // the gate weights once more, packed for the fused conv2 + mix epilogue (SRC_MIXF)
    bool fused = false;  // conv2 keeps all its output channels in one workgroup (<= 96): the mix runs in its epilogue
    float alpha = 0.f;
    bool alpha_set = false;
};

enum SlotKind { SK_CONV, SK_ALPHA, SK_STEM_W, SK_STEM_B, SK_QA_B };
struct Slot {
    std::string name;
    int kind;
    ConvW* conv = nullptr;
    BlockW* block = nullptr;  // for alpha (or skip mixes: alpha stored in skip_alpha)
    float* alpha = nullptr;
    bool* flag = nullptr;
    int64_t shape[4] = {0, 0, 0, 0};
    int ndim = 0;
};

struct ProfRec {
    hipEvent_t a, b;
    double flops, bytes;
    int kind, B, H, W, cin, cout, nt, ntiles, mtiles, n_fast;  // kind: 0 conv3, 1 mix, 2 crush
};

struct mz_handle {
    mz_config cfg;
    int dtype;
    int ch[4], enc[4], dec[4];
    int nhead;
    // weights
    std::vector<std::unique_ptr<BlockW>> enc_blocks[4], dec_blocks[4], head_blocks;
    ConvW crush[3], up[3], skipmix[3];
    float skip_alpha[3] = {0, 0, 0};
    bool skip_alpha_set[3] = {false, false, false};
    std::vector<std::unique_ptr<ConvW>> head_up;
    ConvW qa_conv;
    DevBuf stem_w4;  // float [cp0][4]
    DevBuf qa_bias;  // float [F]
    bool stem_w_set = false, stem_b_set = false, qa_b_set = false;
    DevBuf zero_page;
    std::vector<Slot> slots;
    std::unordered_map<std::string, int> slot_index;
    bool device_ready = false;
    Knobs knobs;
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    size_t recs_used = 0;
    // tile lists of the role-alternating kernels (Runner::tile_table): one per launch geometry, built on first use
    std::map<std::vector<int>, std::pair<DevBuf, int>> tile_tabs;
};

static void add_slot(mz_handle* h, const std::string& name, int kind, std::initializer_list<int64_t> shape) {
    Slot s;
    s.name = name;
    s.kind = kind;
    s.ndim = (int)shape.size();
    int i = 0;
    for (auto d : shape) s.shape[i++] = d;
    h->slot_index[name] = (int)h->slots.size();
    h->slots.push_back(s);
}

// The gate weights of a block's mix once more, packed for the fused conv2 + mix epilogue (SRC_MIXF) in conv2's N tile
static void plan_mixf(ConvW& f, int dtype, const ConvW& conv2) {
    const int c = conv2.cout;
    f.cout = c; f.cin = 2 * c; f.kh = f.kw = 1;
    f.mode = MODE_GEMM1; f.taps = 1;
    f.nt = conv2.nt; f.ntiles = 1;
    f.out_map = OUT_PLAIN; f.in_map = SRC_MIXF;
    f.c0 = c; f.cp0 = pad16(c); f.c1 = c;
    const int zg = dtype == DT_F32 ? 4 : 2;
    f.nchunks = f.nchunks_real = f.cp0 / chunk_channels(dtype) + f.nt * zg;
    f.nchunks32 = (f.cp0 + 31) / 32;
    f.layouts = 1u << PK_MAIN;
    if (dtype != DT_F32) {  // the fused epilogues of the 16x16x32 kernels: conv3s, conv3r (three fragments), conv3t (48 channels)
        f.layouts |= 1u << PK_GATE16;
        if (f.nt == 3) f.layouts |= 1u << PK_GATE16R;
        if (f.cp0 == 48) f.layouts |= 1u << PK_GATE16T;
    }
}

// EncoderBlock / DecoderBlock of c channels with `hidden` channels between its two convolutions
static void plan_block(BlockW& b, int dtype, int c, int hidden) {
    plan_conv(b.conv1, dtype, MODE_CONV3, hidden, c, 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0);      // model.py:742-744
    plan_conv(b.conv2, dtype, MODE_CONV3, c, hidden, 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0);      // model.py:746-748
    plan_conv(b.mix, dtype, MODE_GEMM1, c, 2 * c, 1, 1, OUT_PLAIN, SRC_CONCAT, c, c);        // model.py:805
    b.fused = b.conv2.ntiles == 1 && b.conv2.nt <= 3;
    if (b.fused) plan_mixf(b.mixf, dtype, b.conv2);
}

static void add_block(mz_handle* h, BlockW* b, const std::string& prefix, int c) {
    const int hr = h->cfg.hidden_ratio;
    plan_block(*b, h->dtype, c, hr * c);
    add_slot(h, prefix + ".convnet.conv1.weight", SK_CONV, {hr * c, c, 3, 3});
    h->slots.back().conv = &b->conv1;
    add_slot(h, prefix + ".convnet.conv2.weight", SK_CONV, {c, hr * c, 3, 3});
    h->slots.back().conv = &b->conv2;
    add_slot(h, prefix + ".skip.alpha", SK_ALPHA, {});  // a module's own parameters precede its children's
    h->slots.back().alpha = &b->alpha;
    h->slots.back().flag = &b->alpha_set;
    add_slot(h, prefix + ".skip.conv.weight", SK_CONV, {c, 2 * c, 1, 1});
    h->slots.back().conv = &b->mix;
    h->slots.back().block = b;
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
    int rc = validate(*cfg);
    if (rc) return rc;
    auto* h = new mz_handle();
    h->cfg = *cfg;
    h->dtype = dtype;
    const int ch[4] = {cfg->primary_channels, cfg->secondary_channels, cfg->tertiary_channels, cfg->quaternary_channels};
    const int ly[4] = {cfg->primary_layers, cfg->secondary_layers, cfg->tertiary_layers, cfg->quaternary_layers};
    for (int i = 0; i < 4; ++i) {
        h->ch[i] = ch[i];
        h->enc[i] = (ly[i] + 1) / 2;  // ceil, model.py:277-288
        h->dec[i] = ly[i] / 2;        // floor, model.py:290-300
    }
    h->nhead = cfg->upscale_ratio == 2 ? 1 : (cfg->upscale_ratio == 4 ? 2 : 3);  // model.py:945
    h->knobs = read_knobs();

    // Registry in the reference's state_dict order.
    h->slots.reserve(1024);
    add_slot(h, "stem.conv.weight", SK_STEM_W, {ch[0], 3, 1, 1});
    add_slot(h, "stem.conv.bias", SK_STEM_B, {ch[0]});
    for (int s = 0; s < 4; ++s) {
        for (int i = 0; i < h->enc[s]; ++i) {
            h->enc_blocks[s].emplace_back(new BlockW());
            add_block(h, h->enc_blocks[s].back().get(), "unet.encoder.stage" + std::to_string(s + 1) + "." + std::to_string(i), ch[s]);
        }
    }
    for (int s = 0; s < 3; ++s) {  // model.py:388-390, 857-863
        plan_conv(h->crush[s], dtype, MODE_GEMM1, ch[s + 1], ch[s], 2, 2, OUT_PLAIN, SRC_CRUSH, 0, 0);
        add_slot(h, "unet.encoder.downsample" + std::to_string(s + 1) + ".conv.weight", SK_CONV, {ch[s + 1], ch[s], 2, 2});
        h->slots.back().conv = &h->crush[s];
    }
    plan_conv(h->qa_conv, dtype, MODE_CONV3, cfg->num_deg_features, ch[3], 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0);  // :1010
    add_slot(h, "unet.encoder.qa_head.conv.weight", SK_CONV, {cfg->num_deg_features, ch[3], 3, 3});
    h->slots.back().conv = &h->qa_conv;
    add_slot(h, "unet.encoder.qa_head.conv.bias", SK_QA_B, {cfg->num_deg_features});
    for (int d = 0; d < 4; ++d) {  // decoder stage1 = coarsest level (model.py:290-300)
        const int lvl = 3 - d;
        for (int i = 0; i < h->dec[lvl]; ++i) {
            h->dec_blocks[d].emplace_back(new BlockW());
            add_block(h, h->dec_blocks[d].back().get(), "unet.decoder.stage" + std::to_string(d + 1) + "." + std::to_string(i), ch[lvl]);
        }
    }
    for (int d = 0; d < 3; ++d) {
        const int cin = ch[3 - d], cout = ch[2 - d];
        plan_conv(h->up[d], dtype, MODE_CONV3, 4 * cout, cin, 3, 3, OUT_D2S, SRC_PLAIN, 0, 0);  // model.py:569-571, 900-911
        add_slot(h, "unet.decoder.upsample" + std::to_string(d + 1) + ".conv.weight", SK_CONV, {4 * cout, cin, 3, 3});
        h->slots.back().conv = &h->up[d];
    }
    for (int d = 0; d < 3; ++d) {
        const int cout = ch[2 - d];
        plan_conv(h->skipmix[d], dtype, MODE_GEMM1, cout, 2 * cout, 1, 1, OUT_PLAIN, SRC_CONCAT, cout, cout);  // model.py:573-575
        add_slot(h, "unet.decoder.skip" + std::to_string(d + 1) + ".alpha", SK_ALPHA, {});
        h->slots.back().alpha = &h->skip_alpha[d];
        h->slots.back().flag = &h->skip_alpha_set[d];
        add_slot(h, "unet.decoder.skip" + std::to_string(d + 1) + ".conv.weight", SK_CONV, {cout, 2 * cout, 1, 1});
        h->slots.back().conv = &h->skipmix[d];
    }
    for (int i = 0; i < h->nhead; ++i) {  // model.py:945-954, 981-983
        h->head_blocks.emplace_back(new BlockW());
        add_block(h, h->head_blocks.back().get(), "head.layers." + std::to_string(i) + ".refiner", ch[0]);
        const bool last = i == h->nhead - 1;
        const int cout = last ? 3 : ch[0];
        h->head_up.emplace_back(new ConvW());
        plan_conv(*h->head_up.back(), dtype, MODE_CONV3, 4 * cout, ch[0], 3, 3, last ? OUT_FINAL : OUT_D2S, SRC_PLAIN, 0, 0);
        add_slot(h, "head.layers." + std::to_string(i) + ".upscale.conv.weight", SK_CONV, {4 * cout, ch[0], 3, 3});
        h->slots.back().conv = h->head_up.back().get();
    }
    *out = h;
    return MZ_OK;
}

extern "C" int mz_destroy(mz_handle* h) {
    if (!h) return MZ_OK;
    for (auto& r : h->recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
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

static int prepare_device(mz_handle* h, hipStream_t st) {
    if (h->device_ready) return MZ_OK;
    int rc = ensure_device_ready();
    if (rc) return rc;
    // zero fills go to the CALLER's stream, like every later use of these buffers (a blocking memset on the NULL stream
    // is not ordered with work on a non-blocking stream)
    HIPCHK(h->zero_page.alloc(4096));
    HIPCHK(hipMemsetAsync(h->zero_page.p, 0, 4096, st));
    const int cp0 = pad16(h->ch[0]);
    HIPCHK(h->stem_w4.alloc(sizeof(float) * 4 * cp0));
    HIPCHK(hipMemsetAsync(h->stem_w4.p, 0, sizeof(float) * 4 * cp0, st));
    HIPCHK(h->qa_bias.alloc(sizeof(float) * std::max(1, h->cfg.num_deg_features)));
    h->device_ready = true;
    return MZ_OK;
}

static PackArgs pack_args(const ConvW& c, int layout, int dtype, const float* w_dev, void* dst) {
    const PackShape sh = pack_shape(c, layout);
    PackArgs p;
    p.w = w_dev; p.dst = dst; p.dtype = dtype; p.layout = layout;
    p.cout = c.cout; p.cin = c.cin; p.kh = c.kh; p.kw = c.kw;
    p.taps = c.taps; p.frags = sh.frags; p.ntiles = sh.ntiles; p.nchunks = sh.nchunks;
    p.out_map = c.out_map; p.cq = c.cq; p.cq_p = c.cq_p;
    p.in_map = c.in_map; p.c0 = c.c0; p.cp0 = c.cp0; p.c1 = c.c1;
    return p;
}

// every planned packing, in PackLayout order
static int pack_conv(ConvW& c, int dtype, const float* w_dev, hipStream_t s) {
    for (int l = 0; l < PK_COUNT; ++l) {
        if (!c.has(l)) continue;
        HIPCHK(c.packed[l].alloc(pack_bytes(c, l)));
        HIPCHK(launch_pack(pack_args(c, l, dtype, w_dev, c.packed[l].p), s));
    }
    c.set = true;
    return MZ_OK;
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
    switch (s.kind) {
        case SK_CONV: {
            int rc2 = pack_conv(*s.conv, h->dtype, dev_f32, st);
            if (rc2 == MZ_OK && s.block && s.block->fused && s.conv == &s.block->mix)
                rc2 = pack_conv(s.block->mixf, h->dtype, dev_f32, st);
            return rc2;
        }
        case SK_ALPHA: {
            // sigmoid(alpha) is folded on the host (model.py:833); one 4-byte read at load time.
            float v = 0.f;
            HIPCHK(hipMemcpyAsync(&v, dev_f32, sizeof(float), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            *s.alpha = v;
            *s.flag = true;
            return MZ_OK;
        }
        case SK_STEM_W:
            HIPCHK(launch_pack_stem(dev_f32, nullptr, (float*)h->stem_w4.p, h->ch[0], pad16(h->ch[0]), st));
            h->stem_w_set = true;
            return MZ_OK;
        case SK_STEM_B:
            HIPCHK(launch_pack_stem(nullptr, dev_f32, (float*)h->stem_w4.p, h->ch[0], pad16(h->ch[0]), st));
            h->stem_b_set = true;
            return MZ_OK;
        case SK_QA_B:
            HIPCHK(hipMemcpyAsync(h->qa_bias.p, dev_f32, sizeof(float) * h->cfg.num_deg_features, hipMemcpyDeviceToDevice, st));
            h->qa_b_set = true;
            return MZ_OK;
    }
    return fail(MZ_ERR_INVALID_ARGUMENT, "bad slot");
}

extern "C" int mz_weights_complete(const mz_handle* h) {
    if (!h) return fail(MZ_ERR_INVALID_ARGUMENT, "null handle");
    for (const Slot& s : h->slots) {
        bool ok = true;
        switch (s.kind) {
            case SK_CONV: ok = s.conv->set; break;
            case SK_ALPHA: ok = *s.flag; break;
            case SK_STEM_W: ok = h->stem_w_set; break;
            case SK_STEM_B: ok = h->stem_b_set; break;
            case SK_QA_B: ok = h->qa_b_set; break;
        }
        if (!ok) return fail(MZ_ERR_MISSING_WEIGHTS, "parameter '%s' has not been set", s.name.c_str());
    }
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// workspace plan
// ------------------------------------------------------------------------------------------------
struct Plan {
    int nb;                // images per micro-batch
    int hs[4], ws[4];      // level sizes
    size_t R[4][3], HID[4], Z[4], U[3];
    size_t HR[3][2], HHID[3], HZ[3];  // head levels 1..nhead-1 (index j-1... stored at j)
    size_t QA;
    size_t total;
};

static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

static void make_plan(const mz_handle* h, int nb, int H, int W, Plan& p) {
    const size_t sz = dtype_size(h->dtype);
    const int hr = h->cfg.hidden_ratio;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes);
        return o;
    };
    p.nb = nb;
    p.hs[0] = H; p.ws[0] = W;
    for (int i = 1; i < 4; ++i) { p.hs[i] = p.hs[i - 1] / 2; p.ws[i] = p.ws[i - 1] / 2; }
    for (int l = 0; l < 4; ++l) {
        const size_t px = (size_t)nb * p.hs[l] * p.ws[l];
        const size_t c = px * pad16(h->ch[l]) * sz;
        for (int k = 0; k < 3; ++k) p.R[l][k] = take(c);
        p.HID[l] = take(px * pad16(hr * h->ch[l]) * sz);
        p.Z[l] = take(c);
        if (l < 3) p.U[l] = take(c);
    }
    for (int j = 1; j < h->nhead; ++j) {
        const size_t px = (size_t)nb * (H << j) * (W << j);
        const size_t c = px * pad16(h->ch[0]) * sz;
        p.HR[j][0] = take(c);
        p.HR[j][1] = take(c);
        p.HHID[j] = take(px * pad16(hr * h->ch[0]) * sz);
        p.HZ[j] = take(c);
    }
    p.QA = take((size_t)nb * p.hs[3] * p.ws[3] * pad16(h->cfg.num_deg_features) * sz);
    p.total = off;
}

static int default_micro_batch(const mz_handle* h, int B, int H, int W, int requested) {
    if (requested > 0) return std::min(B, requested);
    // keep a micro-batch's workspace around <= 48 GiB by default (288 GB of HBM per GPU)
    Plan p;
    make_plan(h, 1, H, W, p);
    const size_t budget = (size_t)48 << 30;
    int nb = (int)std::max<size_t>(1, budget / std::max<size_t>(1, p.total));
    return std::max(1, std::min(B, nb));
}

extern "C" int mz_workspace_bytes(const mz_handle* h, int B, int H, int W, int max_images_in_flight, size_t* bytes) {
    if (!h || !bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (B <= 0 || H < 8 || W < 8) return fail(MZ_ERR_INVALID_ARGUMENT, "need B >= 1 and H, W >= 8 (got %d, %d, %d)", B, H, W);
    Plan p;
    make_plan(h, default_micro_batch(h, B, H, W, max_images_in_flight), H, W, p);
    *bytes = p.total;
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
// Diagnostic stamp buffer (only -DMZ_DIAG kernel builds write to it, mz_diag.h; MZ_DEBUG_STAMPS=1 allocates it).
static unsigned long long* debug_buffer() {
    static unsigned long long* buf = nullptr;
    static bool tried = false;
    if (!tried) {
        tried = true;
        if (getenv("MZ_DEBUG_STAMPS")) {
            if (hipMalloc((void**)&buf, 16 * 64 * 8 * sizeof(unsigned long long)) != hipSuccess) buf = nullptr;
            else (void)hipMemset(buf, 0, 16 * 64 * 8 * sizeof(unsigned long long));
        }
    }
    return buf;
}
extern "C" int mz_debug_read(unsigned long long* host_dst) {
    unsigned long long* b = debug_buffer();
    if (!b) return -1;
    return hipMemcpy(host_dst, b, 16 * 64 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -6;
}

// CUs of the CURRENT device, a multiple of 8 (one equal share per XCD); 0 if unknown
static int current_cus() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
    return g_dev_cus[dev];
}

// 1 / sigmoid(alpha) = 1 + e^-alpha for blend_() (mz_device.h), which folds the scale into the reciprocal of the gate's sigmoid:
// rcp(fma(e^-beta, inv_s, inv_s)).  Kept finite: for alpha < -88.7 the exact value overflows to +inf and fma(0, inf, inf) (a gate
// whose e^-beta flushed to 0) would be NaN where the reference (model.py:833-837) returns x; with FLT_MAX the weight is ~0 instead.
static float inv_sigmoid(float alpha) {
    const float v = 1.0f + std::exp(-alpha);
    return std::isfinite(v) ? v : 3.402823466e+38f;
}

// The tiles of a launch in walk order, two words each: {y0 | x0 << 16, image | N tile << 16}.  The order is the group walk of
// mz_device.h (tile_of / tile_rc): ids 0 .. a.grid - 1 in groups of gm pixel tiles x gn N tiles, the tiles of an image in block rows of
// four tile rows where a.blk4 is set, padding ids of partial groups dropped.
static void tile_list(const ConvArgs& a, int th, int tw, std::vector<uint32_t>& t) {
    const int tpi = a.tiles_x * a.tiles_y, gsz = a.gm * a.gn;
    for (int L = 0; L < a.grid; ++L) {
        const int group = L / gsz, within = L % gsz;
        const int gi_n = group / a.groups_m, gi_m = group % a.groups_m;
        const int mt = gi_m * a.gm + within / a.gn, nt = gi_n * a.gn + within % a.gn;
        if (mt >= a.mtiles || nt >= a.ntiles) continue;
        const int b = mt / tpi, trem = mt % tpi;
        int tyi, txi;
        if (!a.blk4) {
            tyi = trem / a.tiles_x; txi = trem % a.tiles_x;
        } else {
            const int bsz = 4 * a.tiles_x, br = trem / bsz, rem = trem % bsz;
            const int rows = std::min(4, a.tiles_y - 4 * br);
            txi = rem / rows; tyi = 4 * br + rem % rows;
        }
        t.push_back((uint32_t)(tyi * th) | (uint32_t)(txi * tw) << 16);
        t.push_back((uint32_t)b | (uint32_t)nt << 16);
    }
}

// The walk of a launch in groups of a.gm pixel tiles x a.gn N tiles (a.mtiles, a.ntiles set): whole groups, padding ids included
static void set_walk(ConvArgs& a) {
    a.groups_m = (a.mtiles + a.gm - 1) / a.gm;
    a.grid = (int)((long long)a.groups_m * ((a.ntiles + a.gn - 1) / a.gn) * a.gm * a.gn);
}

// Tile groups of gm pixel tiles x gn N tiles (gm * gn ~ the workgroups resident on one XCD): inside a group both operands are shared
// through the XCD's L2; per group the activations are re-read ntiles/gn times and the weights mtiles/gm times in total.  Picks the shape
// with the least total re-read traffic and sets the walk of a (a.mtiles, a.ntiles, a.tiles_x, a.tiles_y set): a.grid and its divisors.
static void pick_order(ConvArgs& a, const ConvW& c, double act_bytes, const Knobs& k, int resident_per_xcd = 32) {
    const double W = (double)pack_bytes(c, PK_MAIN), A = act_bytes;
    int best_gm = a.mtiles, best_gn = 1;
    double best = 1e300;
    for (int gn = 1; gn <= a.ntiles; ++gn) {
        if (gn > resident_per_xcd) break;
        if (a.ntiles % gn != 0 && gn != a.ntiles) continue;
        int gm = resident_per_xcd / gn;
        if (gm < 1) gm = 1;
        if (gm > a.mtiles) gm = a.mtiles;
        const double groups_n = std::ceil((double)a.ntiles / gn), groups_m = std::ceil((double)a.mtiles / gm);
        const double traffic = A * groups_n + W * groups_m;
        if (traffic < best) { best = traffic; best_gm = gm; best_gn = gn; }
    }
    a.gm = best_gm; a.gn = best_gn;
    set_walk(a);
    a.inv_gsz = 1.0f / (float)(a.gm * a.gn);
    a.inv_groups_m = 1.0f / (float)a.groups_m;
    a.inv_gn = 1.0f / (float)a.gn;
    a.inv_tpi = a.tiles_x > 0 ? 1.0f / (float)(a.tiles_x * a.tiles_y) : 1.0f;
    a.inv_tiles_x = a.tiles_x > 0 ? 1.0f / (float)a.tiles_x : 1.0f;
    a.inv_bsz = a.tiles_x > 0 ? 1.0f / (float)(4 * a.tiles_x) : 1.0f;
    a.blk4 = k.blk4 && a.tiles_x > 0 && 4 * a.tiles_x < 65536 ? 1 : 0;  // the tile walk inside an image: conv3s_kernel, and the tile lists of conv3r / conv3t
}

// ------------------------------------------------------------------------------------------------
// kernel selection: which kernel runs a 3x3 convolution or a mix, in which geometry.  Functions of the plan (ConvW::has(), never
// whether a buffer happens to be allocated), the knobs, the shape and the CU count only -- no HIP call: mz_debug_select() runs them
// without a GPU, and tests/test_select_cpu.py pins their table.
// ------------------------------------------------------------------------------------------------
struct KernelChoice {
    bool ok = false;             // false = the launch is refused (mz_last_error() says why)
    int kernel = K_CONV256;      // Kernel (mz_kernels.h): the family Runner::launch launches
    int mode = MODE_GEMM1;       // ConvMode of the 256 / 512-pixel kernels; 3x3: theirs even where conv3r / conv3t run (it also sizes the
                                 // fused mix's x ring, ConvArgs::x_via_lds)
    bool fused = false;          // 3x3: conv2 + AdaptiveResidualMix in one launch (EPI_FUSEDMIX)
    bool mix = false;            // an unfused AdaptiveResidualMix (choose_mix)
    int th = 0, tw = 0;          // 3x3: pixel tile
    int geo = 0;                 // conv3r_kernel: 1 = 8 x 40 tiles
    int ragged_planes = 0;       // conv3r_kernel's ragged variant (Cin = 48)
    int layout = PK_MAIN;        // the packing the kernel reads; any other than PK_MAIN: a 16x16x32-MFMA kernel (ConvArgs::wpk16)
    int gate = PK_MAIN;          // EPI_FUSEDMIX on those: the packing of the gate weights (ConvArgs::wmix16)
    bool tile_list = false;      // walks a tile table (conv3r / conv3t, Runner::tile_table)
    int persist = 0;             // persistent workgroups at most; 0 = one workgroup per tile
};

// What mz_debug_last_kernel() and mz_debug_select() report for a choice: the family that is launched and its variant.
static const char* kernel_name(const KernelChoice& ch) {
    if (!ch.ok) return nullptr;
    switch (ch.kernel) {
        case K_CONV256: return ch.mix ? "conv_kernel_mix" : "conv_kernel";
        // A fused layer that qualifies for a persistent launch but not for the 16x16x32 kernels (MZ_NO_S16=1, or K padding beyond
        // MZ_KPAD_PCT) runs conv3w_kernel<.., FUSE> -- conv3p has no fused variant -- and has always been REPORTED as "conv3p": rows of
        // tests/test_select_cpu.py pin that string.  Renaming it to "conv3w_fused" changes those rows and is a change of its own.
        case K_CONV3W: return ch.fused ? (ch.persist > 0 ? "conv3p" : "conv3w_fused") : "conv3w";
        case K_CONV3P: return "conv3p";
        case K_CONV3S: return ch.fused ? "conv3s_fused" : "conv3s";
        case K_CONV3R: return ch.fused ? "conv3r_fused" : ch.ragged_planes ? "conv3r_ragged" : ch.geo ? "conv3r_8x40" : "conv3r";
        case K_CONV3T: return ch.fused ? "conv3t_fused" : "conv3t";
        case K_MIX16: return "mix16";
        case K_MIX16B: return "mix16b";
    }
    return nullptr;
}

// workgroups of a persistent launch: one per CU, a multiple of 8 (one equal share per XCD).  Knobs::persist overrides: 0 = one
// workgroup per tile everywhere (A/B timing); n = force n (tests use 8 / 16 so that small images walk several tiles per workgroup).
static int persistent_workgroups(const Knobs& k, int cus) { return k.persist >= 0 ? k.persist : cus; }

// 32-bit buffer offsets: `planes` 16-byte channel planes of `pixels` pixels stay below 4 GiB
static bool offsets_fit(double planes, double pixels) { return planes * pixels * 16.0 < 4294967296.0; }

// conv2 + AdaptiveResidualMix of a block in one launch: all output channels in one workgroup (BlockW::fused), on the 512-pixel kernels
static bool fuse_mix(const Knobs& k, const BlockW& b) { return b.fused && k.wide && k.fuse; }

// One 3x3 layer call (conv3x3, pad 1): choose_conv3 reads the fields down to Wout, Runner::conv3 all of them.  The role functions below
// are the ONE place that says what a conv1, a block's conv2, a sub-pixel conv, .. is -- for mz_forward, the mz_op_* entries and
// mz_debug_select (which names no buffers) alike.
struct Conv3Call {
    const ConvW* c = nullptr;
    const ConvW* mixf = nullptr;  // EPI_FUSEDMIX: the block's gate weights
    int epi = EPI_STORE, silu = 0;
    bool film = false;            // FiLM epilogue: gamma[b, c] * y + beta[b, c] ahead of the SiLU
    int B = 0, H = 0, W = 0, Hout = 0, Wout = 0;  // D2S / FINAL: into Hout x Wout
    const void* in = nullptr;
    void* out = nullptr;
    const void* xin = nullptr;    // EPI_FUSEDMIX: the block input and the mix's alpha
    float alpha = 0.f;
    const void* img = nullptr;    // EPI_FINAL: the low-resolution image, the total upscale ratio, clamp to [0, 1]
    int R = 0, clamp = 0;
    const ImageViews* views = nullptr;  // EPI_FINAL: img and out are strided image views, stored inside a window (mz_forward_view)
    const float *gamma = nullptr, *beta = nullptr;  // film: float [B][padded cout] each
};
// a plain 3x3 convolution: a block's unfused conv2 (model.py:746-748), the quality head's (:1010)
static Conv3Call plain_call(const ConvW& c, const void* in, void* out, int B, int H, int W) {
    Conv3Call k;
    k.c = &c; k.in = in; k.out = out; k.B = B; k.H = H; k.W = W;
    return k;
}
// conv1 of a block + SiLU (model.py:742-744)
static Conv3Call conv1_call(const ConvW& c, const void* in, void* out, int B, int H, int W) {
    Conv3Call k = plain_call(c, in, out, B, H, W);
    k.silu = 1;
    return k;
}
// SubpixelConv2d: 3x3 + PixelShuffle(2) into Hout x Wout (model.py:900-911)
static Conv3Call d2s_call(const ConvW& c, const void* in, void* out, int B, int H, int W, int Hout, int Wout) {
    Conv3Call k = plain_call(c, in, out, B, H, W);
    k.epi = EPI_D2S; k.Hout = Hout; k.Wout = Wout;
    return k;
}
// the image head: 3x3 to 12 channels + PixelShuffle(2) + bicubic skip + add (+ clamp) into 2H x 2W (model.py:926-930, 156, 162, 177);
// the caller names img, R and clamp
static Conv3Call head_call(const ConvW& c, const void* in, void* out, int B, int H, int W) {
    Conv3Call k = plain_call(c, in, out, B, H, W);
    k.epi = EPI_FINAL; k.Hout = 2 * H; k.Wout = 2 * W;
    return k;
}
// 3x3 + FiLM + optional SiLU (mz_op_conv_film); the caller names gamma and beta
static Conv3Call film_call(const ConvW& c, const void* in, void* out, int B, int H, int W, int silu) {
    Conv3Call k = plain_call(c, in, out, B, H, W);
    k.film = true; k.silu = silu;
    return k;
}
// conv2 of a block + AdaptiveResidualMix with the block input xin in one launch (model.py:746-748, 826-839)
static Conv3Call fused_call(const BlockW& b, const void* in, const void* xin, void* out, int B, int H, int W) {
    Conv3Call k = plain_call(b.conv2, in, out, B, H, W);
    k.epi = EPI_FUSEDMIX; k.mixf = &b.mixf; k.xin = xin; k.alpha = b.alpha;
    return k;
}
// conv2 of a block as mz_forward runs it: fused with the mix (mixf set), or plain and the caller runs the mix.  Where the output goes
// depends on which: the caller names out
static Conv3Call conv2_call(const Knobs& knobs, const BlockW& b, const void* in, const void* xin, int B, int H, int W) {
    return fuse_mix(knobs, b) ? fused_call(b, in, xin, nullptr, B, H, W) : plain_call(b.conv2, in, nullptr, B, H, W);
}

static KernelChoice choose_conv3(const Knobs& k, int dtype, const Conv3Call& call, int cus) {
    KernelChoice ch;
    const ConvW& c = *call.c;
    const ConvW* mixf = call.mixf;
    const int epi = call.epi, B = call.B, H = call.H, W = call.W;
    const bool fused = epi == EPI_FUSEDMIX;
    const int wgs = persistent_workgroups(k, cus);
    const double px = (double)H * W;  // the offset guards hold inside one image
    // tile shape: the 512-pixel kernels (NT <= 3) in the shape that wastes fewer padded pixels, else 8 x 32
    int mode = MODE_CONV3, th = 8, tw = 32;
    if (c.nt <= 3 && k.wide) {
        const long long waste16 = (long long)((H + 15) / 16 * 16) * ((W + 31) / 32 * 32);
        const long long waste8 = (long long)((H + 7) / 8 * 8) * ((W + 63) / 64 * 64);
        if (waste8 <= waste16) { mode = MODE_C3W8; th = 8; tw = 64; }
        else { mode = MODE_C3W16; th = 16; tw = 32; }
    }
    // The image head (12 output channels + PixelShuffle + bicubic skip + clamp) is a per-tile kernel whose load, K loop and long
    // epilogue run one after the other: on 512-pixel tiles (183 KB of LDS) a CU holds ONE workgroup and nothing overlaps; on the
    // 256-pixel kernel several fit and one tile's epilogue runs under another's loads (2160 x 3840, Cin = 96: 2.34 -> 1.60 ms per 3
    // images).  Chosen by dtype only, never by the image size.
    if (epi == EPI_FINAL && dtype != DT_F32) { mode = MODE_CONV3; th = 8; tw = 32; }
    ch.mode = mode;

    // what every 16x16x32-MFMA kernel needs: a 16-bit type, a persistent launch
    const bool s16 = k.s16 && dtype != DT_F32 && wgs > 0;
    // ... and (all but conv3t) padding K to whole 32-channel chunks only where that wastes less than the shape gains (~12 %)
    const bool k_fits = c.nchunks32 * 32 * 100 <= c.cp0 * (100 + k.kpad_pct);
    const bool halo_fits = offsets_fit(4, px);  // 32-bit halo offsets span four planes
    const int p0 = c.cp0 * dtype_size(dtype) / 16;
    // conv3r / conv3t walk a tile list whose entries hold image, N tile and pixel coordinates in 16 bits each
    auto listed = [&](int kernel, int lth, int ltw, int layout, int gate) {
        ch.kernel = kernel; ch.fused = fused; ch.th = lth; ch.tw = ltw;
        ch.layout = layout; ch.gate = gate;
        ch.tile_list = true;
        ch.persist = wgs;
        ch.ok = B < 65536 && c.ntiles < 65536 && (H + lth - 1) / lth * lth < 65536 && (W + ltw - 1) / ltw * ltw < 65536;
        if (!ch.ok) fail(MZ_ERR_INVALID_ARGUMENT, "tile table: image, batch or N-tile index beyond 16 bits");
        return ch;
    };

    // conv3t_kernel: ONE N tile of 33..48 channels (the level-1 block of the 48-channel models), whole 32-channel chunks, three or six
    // and more of them; 12 x 64 pixel tiles; stores and x loads carry 32-bit offsets inside six planes.  The choice depends on channel
    // counts only (never on H or W): its fused variant sums the gate in another order than conv3s_kernel<.., FUSE> -- equal to <= 1 ulp,
    // not bit for bit --, and a tile of upscale_tiled() must run the kernel the whole image runs.
    const bool t_fuse = epi == EPI_FUSEDMIX && k.fuse16 && mixf && mixf->has(PK_GATE16T);
    if (k.t && s16 && !call.film && c.has(PK_CONV16T) && c.ntiles == 1 && (c.nchunks32 == 3 || c.nchunks32 >= 6) &&
        (epi == EPI_STORE || t_fuse) && halo_fits && offsets_fit(6, px))
        return listed(K_CONV3T, 12, 64, PK_CONV16T, t_fuse ? PK_GATE16T : PK_MAIN);

    // conv3r_kernel's ragged variant: conv1 + SiLU with Cin = 48 (two 32-channel chunks, the second with two real planes) into 96-channel
    // N tiles.  The kernel it replaces (conv3p_kernel: 32x32x16 MFMA, exact 16-channel chunks) sums in another order, so the choice
    // depends on channel counts, dtype and knobs only -- never on H or W.
    if (k.r && k.r2 && s16 && !call.film && c.nt == 3 && c.has(PK_CONV16) && epi == EPI_STORE && call.silu && c.nchunks32 == 2 && c.cp0 == 48 &&
        halo_fits && offsets_fit(12, px)) {
        ch.ragged_planes = (c.cp0 - 32) / 8;
        return listed(K_CONV3R, 8, 48, PK_CONV16, PK_MAIN);
    }

    // conv3r_kernel's fused variant (conv2 + AdaptiveResidualMix, C = 96): six or more chunks (one pixel fragment's gate GEMM and blend
    // per chunk), the gate weights packed in accumulator-row order, x and out within 32-bit offsets.  NOT a function of H and W: this
    // kernel and conv3s_kernel<.., FUSE> sum the x half of the gate in different orders inside a 32-wide K step -- equal to <= 1 ulp, not
    // bit for bit -- and a tile of upscale_tiled() must run the kernel the whole image runs, or "tiled == untiled bit for bit"
    // (ultrazoom_amd/tiling.py) breaks.
    if (k.r && k.fuse16 && epi == EPI_FUSEDMIX && s16 && c.nt == 3 && c.ntiles == 1 && c.has(PK_CONV16) && mixf && mixf->has(PK_GATE16R) &&
        mixf->nchunks32 == c.nt && c.nchunks32 >= 6 && p0 % 4 == 0 && k_fits && halo_fits && offsets_fit(12, px))
        return listed(K_CONV3R, 8, 48, PK_CONV16, PK_GATE16R);

    // conv3r_kernel: 96-channel N tiles, any chunk count >= 3 of four whole planes (its halo loads carry the plane in the scalar offset,
    // which the hardware's range check does not cover); its stores carry 32-bit offsets inside 12 output planes / one D2S target image.
    // Its tiles are 8 x 48, or 8 x 40 (five pixel fragments per wave: widths like 120 that 48 does not divide) where those pad fewer
    // pixels, and it runs where they pad no more than the better of the 8 x 64 / 16 x 32 tiles.  (The plain variants accumulate in the
    // same order as conv3s_kernel whatever the tile shape: bit-identical, so this choice may follow H and W.)
    if (k.r && s16 && !call.film && c.nt == 3 && c.has(PK_CONV16) && (epi == EPI_STORE || epi == EPI_D2S) && k_fits && halo_fits &&
        c.nchunks32 >= 3 && p0 % 4 == 0 &&
        (epi == EPI_D2S ? offsets_fit(c.cq_p * dtype_size(dtype) / 16, (double)call.Hout * call.Wout) : offsets_fit(12, px))) {
        const long long rows8 = (long long)((H + 7) / 8 * 8);
        const long long pad48 = rows8 * ((W + 47) / 48 * 48), pad40 = rows8 * ((W + 39) / 40 * 40);
        const long long pads = (long long)((H + th - 1) / th) * th * ((W + tw - 1) / tw) * tw;
        const int geo = pad40 < pad48 ? 1 : 0;
        if ((geo ? pad40 : pad48) <= pads) {
            ch.geo = geo;
            return listed(K_CONV3R, 8, geo ? 40 : 48, PK_CONV16, PK_MAIN);
        }
    }

    // the 512-pixel kernels (per tile: conv3w; persistent: conv3p, or conv3s on the 16x16x32 MFMA) and the 256-pixel conv_kernel
    ch.th = th; ch.tw = tw;
    ch.fused = fused;
    const bool fuse16 = fused && mixf && mixf->has(PK_GATE16) && k.fuse16 &&
                        mixf->nchunks32 == c.nt;  // x K-steps == z K-steps (always so for C <= 96)
    if (mode != MODE_CONV3 && (epi == EPI_STORE || epi == EPI_D2S || fuse16) && wgs > 0) {
        ConvArgs g;  // the per-tile grid
        memset(&g, 0, sizeof(g));
        g.tiles_x = (W + tw - 1) / tw; g.tiles_y = (H + th - 1) / th;
        g.mtiles = B * g.tiles_x * g.tiles_y; g.ntiles = c.ntiles;
        pick_order(g, c, (double)B * H * W * c.cp0 * (double)dtype_size(dtype), k);
        if (s16 && c.has(PK_CONV16) && k_fits && halo_fits) {  // conv3s: 32-bit halo offsets span four planes
            ch.layout = PK_CONV16;
            ch.gate = fused ? PK_GATE16 : PK_MAIN;
            ch.persist = wgs;
        } else if (g.grid > wgs && offsets_fit(2, px)) {
            // conv3p_kernel: 32-bit halo offsets span the two planes of a 16-channel stage; larger images stay on the per-tile
            // kernel (64-bit addresses)
            ch.persist = wgs;
        }
    }
    if (call.film && ch.layout == PK_MAIN) {
        fail(MZ_ERR_INVALID_ARGUMENT, "the FiLM epilogue exists on the 16x16x32 kernel only: bf16 / fp16, at most 96 output channels per "
                                      "N tile, input channels within 12.5 %% of a multiple of 32");
        return ch;
    }
    // conv3p has no fused variant: a fused layer off the 16x16x32 kernels stays on the per-tile kernel (kernel_name() has the history)
    ch.kernel = mode == MODE_CONV3 ? K_CONV256 : ch.persist == 0 || (fused && ch.layout == PK_MAIN) ? K_CONV3W : ch.layout != PK_MAIN ? K_CONV3S : K_CONV3P;
    ch.ok = true;
    return ch;
}

// AdaptiveResidualMix of C channels (c: the [C, 2C] gate weights, SRC_CONCAT) over B x H x W pixels
static KernelChoice choose_mix(const Knobs& k, int dtype, const ConvW& c, int B, int H, int W, int cus) {
    KernelChoice ch;
    ch.ok = ch.mix = true;
    ch.mode = MODE_GEMM1;
    // mix16_kernel: C = k * 192 (192-channel N tiles, x / z straight into MFMA operands), 32-bit buffer offsets inside each tensor;
    // mix16b_kernel (C = 192) is persistent, also under MZ_NO_PERSIST=1: it has no per-tile form
    const bool mix16 = c.has(PK_MIX16) && offsets_fit(c.cp0 * dtype_size(dtype) / 16.0, (double)B * H * W);
    const int wgs = k.persist > 0 ? k.persist : cus;
    if (mix16 && k.mix16b && c.has(PK_MIX16B) && wgs > 0) {
        ch.kernel = K_MIX16B; ch.layout = PK_MIX16B; ch.persist = wgs;
    } else if (mix16) {
        ch.kernel = K_MIX16; ch.layout = PK_MIX16;
    } else {
        ch.kernel = K_CONV256;
    }
    return ch;
}

struct Runner {
    mz_handle* h;
    hipStream_t s;
    int dtype;
    int rc = MZ_OK;
    const Knobs knobs = h->knobs;
    int io_u8 = 0;                                        // images at both ends are uint8 (mz_forward_u8)
    int cus = current_cus();

    // the profiling record of one launch (kind: 0 conv3, 1 mix, 2 crush); nullptr unless the handle profiles
    ProfRec* prof_begin(int kind, const ConvArgs& a, const ConvW& c, double flops, double bytes) {
        if (!h->prof) return nullptr;
        if (h->recs_used == h->recs.size()) {
            ProfRec n;
            if (hipEventCreate(&n.a) != hipSuccess || hipEventCreate(&n.b) != hipSuccess) return nullptr;
            h->recs.push_back(n);
        }
        ProfRec* r = &h->recs[h->recs_used++];
        r->flops = flops; r->bytes = bytes;
        r->kind = kind; r->B = a.B; r->H = a.H; r->W = a.W; r->cin = c.cin; r->cout = c.cout; r->nt = c.nt; r->ntiles = a.ntiles;
        r->mtiles = a.mtiles; r->n_fast = a.gm * 1000 + a.gn;
        (void)hipEventRecord(r->a, s);
        return r;
    }

    void prof_end(ProfRec* r) {
        if (r) (void)hipEventRecord(r->b, s);
    }

    int check(hipError_t e, const char* what) {
        if (e != hipSuccess && rc == MZ_OK) rc = fail(MZ_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
        return rc;
    }

    // what every launch says alike: the layer's main packing and chunk counts, its first input over B x H x W pixels, its output of
    // cp_out channels per pixel
    void base_args(ConvArgs& a, const ConvW& c, const void* in0, void* out, int B, int H, int W, int cp_out) {
        memset(&a, 0, sizeof(a));
        a.wpk = c.packed[PK_MAIN].p;
        a.zero = h->zero_page.p;
        a.dbg = debug_buffer();
        a.nchunks = c.nchunks;
        a.nchunks_real = c.nchunks_real;
        a.ntiles = c.ntiles;
        a.in0 = in0; a.out = out;
        a.B = B; a.H = H; a.W = W; a.Ho = H; a.Wo = W;
        a.p0 = c.cp0 * dtype_size(dtype) / 16;
        a.cp_out = cp_out;
        a.p_out = a.cp_out * dtype_size(dtype) / 16;
    }

    // conv3r_kernel / conv3t_kernel: the launch's tiles in walk order as a table in HBM (ConvArgs::tile_tab), so that the kernels'
    // helper role -- the critical path of their short tiles -- reads a tile's coordinates with one scalar load instead of running
    // the divisions of the group walk (tile_of / tile_rc, mz_device.h) three times per phase.  The order IS that walk's: ids
    // 0 .. grid - 1 in gm x gn groups, the tiles of an image in block rows of four tile rows (blk4), padding ids dropped.  Needs
    // pick_order() done; sets a.tile_tab and a.grid (= tiles listed), padded for up to wgs workgroups.  One table per geometry, kept
    // with the handle.
    void tile_table(ConvArgs& a, int th, int tw, int wgs) {
        const int pad = 4 * ((wgs > 256 ? wgs : 256) / 8) + 8;
        const std::vector<int> key = {th, tw, a.B, a.tiles_x, a.tiles_y, a.ntiles, a.gm, a.gn, a.grid, a.blk4, pad};
        auto it = h->tile_tabs.find(key);
        if (it == h->tile_tabs.end()) {
            std::vector<uint32_t> t;
            t.reserve(2 * ((size_t)a.mtiles * a.ntiles + pad));
            tile_list(a, th, tw, t);
            const int n = (int)(t.size() / 2);
            t.resize(t.size() + 2 * (size_t)pad, 0u);
            DevBuf d;
            if (check(d.alloc(t.size() * 4), "tile table")) return;
            if (check(hipMemcpy(d.p, t.data(), t.size() * 4, hipMemcpyHostToDevice), "tile table upload")) return;
            it = h->tile_tabs.emplace(key, std::make_pair(std::move(d), n)).first;
        }
        a.tile_tab = it->second.first.p;
        a.grid = it->second.second;
    }

    hipError_t launch_kernel(const KernelChoice& ch, const ConvArgs& a, int nt) {
        switch (ch.kernel) {
            case K_CONV256: return launch_conv256(dtype, ch.mode, nt, a, s);
            case K_CONV3W: return launch_conv3w(dtype, ch.mode, nt, a, s);
            case K_CONV3P: return launch_conv3p(dtype, ch.mode, nt, a, s);
            case K_CONV3S: return launch_conv3s(dtype, ch.mode, nt, a, s);
            case K_CONV3R: return launch_conv3r(dtype, a, s);
            case K_CONV3T: return launch_conv3t(dtype, a, s);
            case K_MIX16: return launch_mix16(dtype, a, s);
            case K_MIX16B: return launch_mix16b(dtype, a, s, ch.persist);
        }
        return hipErrorInvalidValue;
    }
    void launch(const KernelChoice& ch, const ConvArgs& a, int nt, ProfRec* r, const char* what = nullptr) {
        if (!what) what = g_last_kernel = kernel_name(ch);  // `what` given: a launch that is neither a 3x3 convolution nor a mix
        check(launch_kernel(ch, a, nt), what);
        prof_end(r);
    }

    // conv3x3, pad 1 (model.py:742-748, 900-909, 1010)
    void conv3(const Conv3Call& k) {
        if (rc) return;
        const KernelChoice ch = choose_conv3(knobs, dtype, k, cus);
        if (!ch.ok) { rc = MZ_ERR_INVALID_ARGUMENT; return; }
        const ConvW& c = *k.c;
        const int B = k.B, H = k.H, W = k.W;
        ConvArgs a;
        base_args(a, c, k.in, k.out, B, H, W, k.epi == EPI_D2S ? c.cq_p : pad16(c.cout));
        a.src = SRC_PLAIN;
        a.tiles_x = (W + ch.tw - 1) / ch.tw; a.tiles_y = (H + ch.th - 1) / ch.th;
        a.mtiles = B * a.tiles_x * a.tiles_y;
        a.epi = k.epi; a.silu = k.silu;
        a.Hout = k.Hout; a.Wout = k.Wout;
        a.img = k.img; a.R = k.R; a.clamp = k.clamp;
        if (k.epi == EPI_FINAL) { a.Hi = k.Hout / k.R; a.Wi = k.Wout / k.R; a.io_u8 = io_u8; }
        if (k.epi == EPI_FINAL && k.views) {  // the kernel chosen above, in its VIEW instantiation
            a.view = 1;
            for (int i = 0; i < 4; ++i) { a.vin[i] = k.views->in[i]; a.vout[i] = k.views->out[i]; }
            a.win_y0 = k.views->y0; a.win_x0 = k.views->x0; a.win_h = k.views->h; a.win_w = k.views->w;
        }
        const bool fused = ch.fused;
        if (fused) {
            a.in1 = k.xin;
            a.p1 = pad16(c.cout) * dtype_size(dtype) / 16;
            a.wmix = k.mixf->packed[PK_MAIN].p;
            a.mix_pieces = k.mixf->nchunks * k.mixf->nt;
            {   // room for the 8 compute waves' x fragments next to the gate weights in ring slots 1-2?
                const int slot = ch.mode == MODE_C3W16 ? stage_bytes<MODE_C3W16>(c.nt) : stage_bytes<MODE_C3W8>(c.nt);
                const int ncx = a.p1 / 2;
                a.x_via_lds = (a.mix_pieces * 1024 + 8 * ncx * 1024 <= 2 * slot) ? 1 : 0;
            }
            a.mix_scale = 1.0f / (1.0f + std::exp(-k.alpha));
            a.inv_mix_scale = inv_sigmoid(k.alpha);
        }
        a.geo = ch.geo;
        a.ragged_planes = ch.ragged_planes;
        const double sz = dtype_size(dtype);
        const double px = (double)B * H * W;
        pick_order(a, c, px * c.cp0 * sz, knobs);
        if (ch.layout != PK_MAIN) {
            a.wpk16 = c.packed[ch.layout].p;
            a.nchunks16 = pack_shape(c, ch.layout).nchunks;
            if (fused) a.wmix16 = k.mixf->packed[ch.gate].p;
        }
        if (ch.tile_list) tile_table(a, ch.th, ch.tw, ch.persist);
        if (rc) return;
        a.persist = std::min((a.grid + 7) / 8 * 8, ch.persist);
        a.film_gamma = k.gamma; a.film_beta = k.beta;
        // algorithmic flops and bytes: input once, output once, weights once; a fused conv2 + mix also runs the gate GEMM and reads the
        // block input x once
        const double flops = 2.0 * px * 9.0 * c.cin * c.cout + (fused ? 2.0 * px * 2.0 * c.cout * c.cout : 0.0);
        const double bytes = px * (c.cin + c.cout) * sz + 9.0 * c.cin * c.cout * sz + (fused ? px * c.cout * sz : 0.0);
        launch(ch, a, c.nt, prof_begin(0, a, c, flops, bytes));
    }

    // AdaptiveResidualMix (model.py:826-839): out = x + sigmoid(alpha)*sigmoid(W[x;z])*(z - x)
    void mix(const ConvW& c, float alpha, const void* x, const void* z, void* out, int B, int H, int W) {
        if (rc) return;
        const KernelChoice ch = choose_mix(knobs, dtype, c, B, H, W, cus);
        ConvArgs a;
        base_args(a, c, x, out, B, H, W, pad16(c.cout));
        const int sz = dtype_size(dtype);
        a.in1 = z; a.p1 = pad16(c.c1) * sz / 16;
        a.nchunks0 = c.cp0 / chunk_channels(dtype);
        a.src = SRC_CONCAT;
        const long long npix = (long long)B * H * W;
        a.mtiles = (int)((npix + 255) / 256);
        a.epi = EPI_MIX;
        a.mix_scale = 1.0f / (1.0f + std::exp(-alpha));
        a.inv_mix_scale = inv_sigmoid(alpha);
        if (ch.layout != PK_MAIN) {  // 192-channel N tiles, x / z straight into MFMA operands (mix16_kernel / mix16b_kernel)
            const PackShape sh = pack_shape(c, ch.layout);
            a.ntiles = sh.ntiles;
            a.wpk16 = c.packed[ch.layout].p;
            a.nchunks16 = sh.nchunks;
        }
        pick_order(a, c, (double)npix * (c.cp0 + pad16(c.c1)) * sz, knobs, ch.layout != PK_MAIN ? 32 : 64);
        launch(ch, a, c.nt, prof_begin(1, a, c, 2.0 * (double)npix * c.cin * c.cout, (double)npix * 3.0 * c.cout * sz));
    }

    // PixelCrush (model.py:857-863, 881-882): conv 2x2 stride 2, floors odd sizes
    void crush(const ConvW& c, const void* in, void* out, int B, int H, int W) {
        if (rc) return;
        ConvArgs a;
        base_args(a, c, in, out, B, H, W, pad16(c.cout));
        a.Ho = H / 2; a.Wo = W / 2;
        a.nchunks0 = c.cp0 / chunk_channels(dtype);
        a.src = SRC_CRUSH;
        const long long npix = (long long)B * a.Ho * a.Wo;
        a.mtiles = (int)((npix + 255) / 256);
        a.epi = EPI_STORE;
        const double sz = dtype_size(dtype);
        pick_order(a, c, (double)B * H * W * c.cp0 * sz, knobs, 64);
        ProfRec* r = prof_begin(2, a, c, 2.0 * (double)npix * 4.0 * c.cin * c.cout, ((double)B * H * W * c.cin + (double)npix * c.cout) * sz);
        KernelChoice ch;  // conv_kernel's 1x1 mode is the only kernel that gathers the 2x2 patches
        ch.ok = true; ch.kernel = K_CONV256; ch.mode = MODE_GEMM1;
        launch(ch, a, c.nt, r, "crush launch");
    }
};

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// views: x and out_sr are the first elements of image views (out_sr: of the window) instead of dense NCHW tensors
static int forward_micro(mz_handle* h, const char* x, char* out_sr, float* out_qa, int nb, int H, int W, int clamp,
                         char* ws, hipStream_t s, int io_u8, const ImageViews* views) {
    Plan p;
    make_plan(h, nb, H, W, p);
    Runner run{h, s, h->dtype};
    run.io_u8 = io_u8;
    const int r = h->cfg.upscale_ratio;

    auto block = [&](const BlockW& b, const void* xin, void* hid, void* z, void* yout, int hh, int ww) {
        // EncoderBlock / DecoderBlock (model.py:507-511): conv1 -> SiLU -> conv2 -> adaptive mix with the input
        run.conv3(conv1_call(b.conv1, xin, hid, nb, hh, ww));
        // conv2 + AdaptiveResidualMix in one launch (all output channels live in one workgroup), or in two
        Conv3Call c2 = conv2_call(run.knobs, b, hid, xin, nb, hh, ww);
        c2.out = c2.mixf ? yout : z;
        run.conv3(c2);
        if (!c2.mixf) run.mix(b.mix, b.alpha, xin, z, yout, nb, hh, ww);
    };

    // stem (model.py:158): NCHW image -> NHWC features
    char* cur = ws + p.R[0][0];
    if (hipError_t e = launch_stem(h->dtype, x, (const float*)h->stem_w4.p, cur, nb, H, W, pad16(h->ch[0]), s, io_u8, views ? views->in : nullptr);
        e != hipSuccess)
        return fail(MZ_ERR_HIP, "stem launch: %s", hipGetErrorString(e));

    // encoder (model.py:461-484)
    char* feat[4];
    int feat_slot[4];
    for (int l = 0; l < 4; ++l) {
        int slot = 0;
        if (l > 0) {
            cur = ws + p.R[l][0];
            run.crush(h->crush[l - 1], feat[l - 1], cur, nb, p.hs[l - 1], p.ws[l - 1]);
        }
        for (auto& b : h->enc_blocks[l]) {
            char* nxt = ws + p.R[l][slot ^ 1];
            block(*b, cur, ws + p.HID[l], ws + p.Z[l], nxt, p.hs[l], p.ws[l]);
            cur = nxt;
            slot ^= 1;
        }
        feat[l] = cur;
        feat_slot[l] = slot;
    }

    // quality head (model.py:482, 1026-1032); upscale() discards it (model.py:175)
    if (out_qa) {
        const int F = h->cfg.num_deg_features;
        run.conv3(plain_call(h->qa_conv, feat[3], ws + p.QA, nb, p.hs[3], p.ws[3]));
        if (run.rc) return run.rc;
        if (hipError_t e = launch_qa_reduce(h->dtype, ws + p.QA, (const float*)h->qa_bias.p, out_qa, nb, p.hs[3] * p.ws[3], pad16(F), F, s);
            e != hipSuccess)
            return fail(MZ_ERR_HIP, "qa reduce launch: %s", hipGetErrorString(e));
    }

    // decoder (model.py:691-724)
    cur = feat[3];
    int slot = feat_slot[3];
    for (int d = 0; d < 4; ++d) {
        const int l = 3 - d;
        if (d > 0) {
            // SubpixelConv2d (model.py:926-930) + crop_feature_maps zero pad (model.py:650-689) + skip mix (:701)
            const ConvW& up = h->up[d - 1];
            char* u = ws + p.U[l];
            run.conv3(d2s_call(up, cur, u, nb, p.hs[l + 1], p.ws[l + 1], p.hs[l], p.ws[l]));
            if (run.rc) return run.rc;
            if (hipError_t e = launch_zero_border(h->dtype, u, nb, p.hs[l], p.ws[l], up.cq_p, 2 * p.hs[l + 1], 2 * p.ws[l + 1], s);
                e != hipSuccess)
                return fail(MZ_ERR_HIP, "zero border launch: %s", hipGetErrorString(e));
            // pick a level-l buffer that is not the saved encoder feature
            slot = (feat_slot[l] + 1) % 3;
            char* dst = ws + p.R[l][slot];
            run.mix(h->skipmix[d - 1], h->skip_alpha[d - 1], feat[l], u, dst, nb, p.hs[l], p.ws[l]);
            cur = dst;
        }
        for (auto& b : h->dec_blocks[d]) {
            int nslot = (slot + 1) % 3;
            if (d > 0 && nslot == feat_slot[l]) nslot = (nslot + 1) % 3;  // (the encoder feature is dead after the skip mix, but keep it simple)
            char* nxt = ws + p.R[l][nslot];
            block(*b, cur, ws + p.HID[l], ws + p.Z[l], nxt, p.hs[l], p.ws[l]);
            cur = nxt;
            slot = nslot;
        }
    }

    // head (model.py:968-972, 997-1001) + bicubic skip + residual add + clamp (model.py:156,162,177)
    int hh = H, ww = W;
    for (int i = 0; i < h->nhead; ++i) {
        char *hid, *z, *y;
        if (i == 0) {
            hid = ws + p.HID[0]; z = ws + p.Z[0];
            int nslot = (slot + 1) % 3;
            y = ws + p.R[0][nslot];
        } else {
            hid = ws + p.HHID[i]; z = ws + p.HZ[i]; y = ws + p.HR[i][1];
        }
        block(*h->head_blocks[i], cur, hid, z, y, hh, ww);
        const bool last = i == h->nhead - 1;
        if (last) {
            Conv3Call head = head_call(*h->head_up[i], y, out_sr, nb, hh, ww);
            head.img = x; head.R = r; head.clamp = clamp; head.views = views;
            run.conv3(head);
        } else {
            char* nxt = ws + p.HR[i + 1][0];
            run.conv3(d2s_call(*h->head_up[i], y, nxt, nb, hh, ww, 2 * hh, 2 * ww));
            cur = nxt;
            hh *= 2; ww *= 2;
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
    const int nbmax = default_micro_batch(h, B, H, W, max_images_in_flight);
    Plan p;
    make_plan(h, nbmax, H, W, p);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, p.total)) return fail(r);
    const size_t sz = io_u8 ? 1 : dtype_size(h->dtype);
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

// ------------------------------------------------------------------------------------------------
// operator-level entry points (tests)
// ------------------------------------------------------------------------------------------------
extern "C" int mz_padded_channels(int c) { return pad16(c); }

// What an mz_op_* entry runs its layer on, built after the entry's own argument checks: a throw-away handle -- the zero page, the knobs
// read now -- and a Runner on it.  rc says whether making the handle, then pack() of a layer's weights, worked; an entry returns it
// where it is set, before it touches run (which exists either way).  finish() waits for the stream and gives the entry's return code.
static int op_handle(mz_handle& fake, hipStream_t s) {
    HIPCHK(fake.zero_page.alloc(4096));
    HIPCHK(hipMemsetAsync(fake.zero_page.p, 0, 4096, s));
    fake.knobs = read_knobs();
    return MZ_OK;
}
struct OpRun {
    mz_handle fake;
    int rc;
    Runner run;
    OpRun(int dtype, void* hip_stream) : rc(op_handle(fake, (hipStream_t)hip_stream)), run{&fake, (hipStream_t)hip_stream, dtype} {}
    int pack(ConvW& c, const float* w_dev_f32) { return rc = rc ? rc : pack_conv(c, run.dtype, w_dev_f32, run.s); }
    // the entry's return code: a failed wait for the stream is reported ahead of the Runner's own code
    int finish() { HIPCHK(hipStreamSynchronize(run.s)); return run.rc; }
};

extern "C" int mz_op_conv(int dtype, int kind, const void* in0, const void* in1, const float* w_dev_f32, float alpha,
                          void* out, int B, int H, int W, int cin, int cout, int Hout, int Wout, int silu,
                          void* hip_stream) {
    int rc = ensure_device_ready();
    if (rc) return rc;
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
            if (!run.rc) {
                hipError_t e = launch_zero_border(dtype, out, B, Hout, Wout, c.cq_p, 2 * H, 2 * W, run.s);
                if (e != hipSuccess) run.rc = fail(MZ_ERR_HIP, "zero border: %s", hipGetErrorString(e));
            }
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
    int rc = ensure_device_ready();
    if (rc) return rc;
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
    int rc = ensure_device_ready();
    if (rc) return rc;
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
    int rc = ensure_device_ready();
    if (rc) return rc;
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
    int rc = ensure_device_ready();
    if (rc) return rc;
    ConvW c;
    plan_conv(c, dtype, MODE_CONV3, 12, cin, 3, 3, OUT_FINAL, SRC_PLAIN, 0, 0);
    OpRun op(dtype, hip_stream);
    if (op.pack(c, w_dev_f32)) return op.rc;
    Conv3Call k = head_call(c, feat, out, B, H, W);
    k.img = img; k.R = R; k.clamp = clamp;
    op.run.conv3(k);
    return op.finish();
}

// ------------------------------------------------------------------------------------------------
// image-quality metrics (mz_metrics.h): no reference counterpart in model.py; stands in for torchmetrics as the reference's
// pretrain.py:209-211, 301-329 uses it.  Stateless like the mz_op_* entries.
// ------------------------------------------------------------------------------------------------
static int check_metrics_shape(int B, int H, int W, int which) {
    if (which <= 0 || (which & ~(MET_PSNR | MET_SSIM | MET_VIF)))
        return fail(MZ_ERR_INVALID_ARGUMENT, "which must be a non-empty combination of 1 (PSNR), 2 (SSIM), 4 (VIF), got %d", which);
    if (B < 1 || H < 1 || W < 1) return fail(MZ_ERR_INVALID_ARGUMENT, "need B, H, W >= 1 (got %d, %d, %d)", B, H, W);
    if (B > 65535 || H > (1 << 28) || W > (1 << 28))
        return fail(MZ_ERR_INVALID_ARGUMENT, "at most 65535 images of at most 2^28 pixels a side (got %d, %d, %d)", B, H, W);
    if ((which & MET_SSIM) && (H < 11 || W < 11))
        return fail(MZ_ERR_INVALID_ARGUMENT, "SSIM needs images of at least 11 x 11 pixels, got %d x %d", H, W);
    if ((which & MET_VIF) && (H < 41 || W < 41))
        return fail(MZ_ERR_INVALID_ARGUMENT, "VIF needs images of at least 41 x 41 pixels, got %d x %d", H, W);
    return MZ_OK;
}

extern "C" int mz_metrics_workspace_bytes(int B, int H, int W, int which, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_metrics_shape(B, H, W, which)) return rc;
    *bytes = metrics_plan(B, H, W, which).total;
    return MZ_OK;
}

extern "C" int mz_metrics(const mz_image_view* pred, const mz_image_view* target, int elem, int B, int H, int W, int which,
                          double data_range, double sigma_n_sq, double* out_dev, void* workspace, size_t workspace_bytes,
                          void* hip_stream) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ false, /*batch_bound*/ false, /*side_bound*/ false};
    MetricsArgs a = {};
    if (const Refusal r = check_views(pred, target, rules, elem, B, H, W, &a.pred, &a.target)) return fail(r);
    if (int rc = check_metrics_shape(B, H, W, which)) return rc;
    if (!out_dev) return fail(MZ_ERR_INVALID_ARGUMENT, "null out_dev");
    a.plan = metrics_plan(B, H, W, which);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, a.plan.total)) return fail(r);
    if (int rc = ensure_device_ready()) return rc;
    a.elem = elem; a.B = B; a.H = H; a.W = W;
    a.which = which;
    a.data_range = data_range;
    a.sigma_n_sq = sigma_n_sq;
    a.out = out_dev;
    a.ws = (char*)workspace;
    const hipError_t e = launch_metrics(a, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(MZ_ERR_HIP, "metrics launch: %s", hipGetErrorString(e));
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// antialiased resampling to any size (mz_resize.h): no reference counterpart in model.py; stands in for torchvision's Resize as the
// reference's data.py:91-108 uses it.  Stateless like mz_metrics.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static int check_resize_shape(int Hin, int Win, int Hout, int Wout, int filter) {
    if (filter != RF_BICUBIC && filter != RF_BILINEAR)
        return fail(MZ_ERR_INVALID_ARGUMENT, "filter must be 0 (bicubic) or 1 (bilinear), got %d", filter);
    if (Hin < 1 || Win < 1 || Hout < 1 || Wout < 1)
        return fail(MZ_ERR_INVALID_ARGUMENT, "need sizes >= 1 (got %d x %d -> %d x %d)", Hin, Win, Hout, Wout);
    if (Hin > (1 << 28) || Win > (1 << 28) || Hout > (1 << 28) || Wout > (1 << 28))
        return fail(MZ_ERR_INVALID_ARGUMENT, "at most 2^28 pixels a side (got %d x %d -> %d x %d)", Hin, Win, Hout, Wout);
    if ((long long)Hin > (long long)kResizeMaxRatio * Hout || (long long)Win > (long long)kResizeMaxRatio * Wout)
        return fail(MZ_ERR_INVALID_ARGUMENT, "%d x %d -> %d x %d shrinks an axis by more than %d", Hin, Win, Hout, Wout, kResizeMaxRatio);
    return MZ_OK;
}

extern "C" int mz_resize_workspace_bytes(int Hin, int Win, int Hout, int Wout, int filter, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_resize_shape(Hin, Win, Hout, Wout, filter)) return rc;
    *bytes = resize_plan(Hin, Win, Hout, Wout, filter).total;
    return MZ_OK;
}

extern "C" int mz_resize(const mz_image_view* x, const mz_image_view* out, int elem, int B, int Hin, int Win, int Hout, int Wout, int filter,
                         int clamp, const int32_t window[4], void* workspace, size_t workspace_bytes, void* hip_stream) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ false};
    ResizeArgs a = {};
    if (const Refusal r = check_views(x, out, rules, elem, B, Hout, Wout, &a.x, &a.out)) return fail(r);
    if (int rc = check_resize_shape(Hin, Win, Hout, Wout, filter)) return rc;
    if (const Refusal r = check_window(window, Hout, Wout, &a.y0, &a.x0, &a.h, &a.w)) return fail(r);
    a.plan = resize_plan(Hin, Win, Hout, Wout, filter);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, a.plan.total)) return fail(r);
    if (int rc = ensure_device_ready()) return rc;
    a.elem = elem;
    a.B = B;
    a.Hin = Hin; a.Win = Win; a.Hout = Hout; a.Wout = Wout;
    a.filter = filter;
    a.clamp = clamp != 0;
    a.ws = (char*)workspace;
    const hipError_t e = launch_resize(a, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(MZ_ERR_HIP, "resize launch: %s", hipGetErrorString(e));
    return MZ_OK;
}

// Host only: resize_taps() (mz_resize.h) of one output index, the source the device's table kernel compiles too
extern "C" int mz_debug_resize_taps(int n_in, int n_out, int filter, int i, int* first, double* w, int cap) {
    if (!first || !w || cap < 0) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument or negative cap");
    if (int rc = check_resize_shape(n_in, 1, n_out, 1, filter)) return rc;
    if (i < 0 || i >= n_out) return fail(MZ_ERR_INVALID_ARGUMENT, "output index %d is not in [0, %d)", i, n_out);
    const int count = resize_taps(n_in, n_out, filter, i, first, cap, [&](int j, double v) { w[j] = v; });
    if (count > cap) return fail(MZ_ERR_INVALID_ARGUMENT, "output %d has %d taps, room for %d", i, count, cap);
    return count;
}

// ------------------------------------------------------------------------------------------------
// the degradation chain (mz_degrade.h): no reference counterpart in model.py; stands in for torchvision's gaussian_blur, gaussian_noise
// and jpeg as the reference's transforms.py uses them.  Stateless like mz_resize.  Every check comes before anything touches the GPU.
// ------------------------------------------------------------------------------------------------
static int check_degrade_views(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int in_place_ok, DegradeArgs* a) {
    static const ViewRules rules = {3, MZ_ELEM_NAMES_0_3, /*second_is_output*/ true, /*batch_bound*/ true, /*side_bound*/ true};
    if (const Refusal r = check_views(x, out, rules, elem, B, H, W, &a->x, &a->out)) return fail(r);
    if (const Refusal r = check_overlap(x, out, elem, B, H, W, in_place_ok != 0)) return fail(r);
    a->elem = elem; a->B = B; a->H = H; a->W = W;
    return MZ_OK;
}

extern "C" int mz_blur(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, double sigma, void* hip_stream) {
    DegradeArgs a = {};
    if (int rc = check_degrade_views(x, out, elem, B, H, W, 0, &a)) return rc;
    BlurWeights bw = {};
    const int half = blur_weights(sigma, &bw);
    if (half < 0) return fail(MZ_ERR_INVALID_ARGUMENT, "sigma %g: need 0 <= sigma and int(3 sigma) <= %d", sigma, kBlurMaxHalf);
    if (half >= (H < W ? H : W))
        return fail(MZ_ERR_INVALID_ARGUMENT, "sigma %g needs %d pixels of reflect padding, a %d x %d image has no such reflection", sigma, half, H, W);
    if (int rc = ensure_device_ready()) return rc;
    const hipError_t e = launch_blur(a, bw, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(MZ_ERR_HIP, "blur launch: %s", hipGetErrorString(e));
    return MZ_OK;
}

extern "C" int mz_noise(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, double sigma, uint64_t seed,
                        uint64_t offset, void* hip_stream) {
    DegradeArgs a = {};
    if (int rc = check_degrade_views(x, out, elem, B, H, W, 1, &a)) return rc;
    if (!(sigma >= 0.0) || !(sigma <= 1e6)) return fail(MZ_ERR_INVALID_ARGUMENT, "sigma %g: need 0 <= sigma <= 1e6", sigma);
    if (int rc = ensure_device_ready()) return rc;
    const hipError_t e = launch_noise(a, sigma, seed, offset, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(MZ_ERR_HIP, "noise launch: %s", hipGetErrorString(e));
    return MZ_OK;
}

extern "C" int mz_jpeg_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 28) || W > (1 << 28))
        return fail(MZ_ERR_INVALID_ARGUMENT, "need 1 <= B <= 65535 and 1 <= H, W <= 2^28 (got %d, %d, %d)", B, H, W);
    *bytes = jpeg_plan(B, H, W).total;
    return MZ_OK;
}

extern "C" int mz_jpeg(const mz_image_view* x, const mz_image_view* out, int elem, int B, int H, int W, int quality, void* workspace,
                       size_t workspace_bytes, void* hip_stream) {
    DegradeArgs a = {};
    if (int rc = check_degrade_views(x, out, elem, B, H, W, 0, &a)) return rc;
    if (quality < 1 || quality > 100) return fail(MZ_ERR_INVALID_ARGUMENT, "quality must be 1..100, got %d", quality);
    const JpegPlan plan = jpeg_plan(B, H, W);
    if (const Refusal r = check_workspace(workspace, workspace_bytes, plan.total)) return fail(r);
    JpegTables t;
    jpeg_qtable(quality, &t);
    if (int rc = ensure_device_ready()) return rc;
    const hipError_t e = launch_jpeg(a, t, plan, (char*)workspace, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(MZ_ERR_HIP, "jpeg launch: %s", hipGetErrorString(e));
    return MZ_OK;
}

// Host only: what the kernels are handed and compile -- the blur weights of a sigma, the quantisation tables of a quality, one Philox block
extern "C" int mz_debug_blur_weights(double sigma, double* w, int cap) {
    BlurWeights bw = {};
    const int half = blur_weights(sigma, &bw);
    if (!w || half < 0 || 2 * half + 1 > cap) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument, a bad sigma (%g) or room for fewer than k weights", sigma);
    for (int j = 0; j <= 2 * half; ++j) w[j] = bw.w[j];
    return 2 * half + 1;
}
extern "C" int mz_debug_jpeg_qtable(int quality, uint8_t* luma, uint8_t* chroma) {
    if (!luma || !chroma || quality < 1 || quality > 100) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument or quality %d outside 1..100", quality);
    JpegTables t;
    jpeg_qtable(quality, &t);
    memcpy(luma, t.q[0], 64);
    memcpy(chroma, t.q[1], 64);
    return MZ_OK;
}
extern "C" int mz_debug_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    if (!counter || !key || !out) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], out);
    return MZ_OK;
}

// ------------------------------------------------------------------------------------------------
// introspection
// ------------------------------------------------------------------------------------------------
extern "C" const char* mz_last_error(void) { return g_err; }
extern "C" const char* mz_debug_last_kernel(void) { return g_last_kernel; }

// Host-only (no GPU): the tile list Runner::tile_table() uploads for a launch of B images of tiles_y x tiles_x tiles of th x tw pixels,
// ntiles N tiles, walked in groups of gm x gn (blk4: block rows of four tile rows).  Writes at most cap entries of two words to out
// and returns the number of tiles listed (tests/test_cabi_cpu.py checks that every tile appears exactly once).
extern "C" int mz_debug_tile_list(int B, int tiles_y, int tiles_x, int ntiles, int gm, int gn, int blk4, int th, int tw, unsigned int* out, int cap) {
    if (B < 1 || tiles_x < 1 || tiles_y < 1 || ntiles < 1 || gm < 1 || gn < 1 || th < 1 || tw < 1 || !out || cap < 0) return MZ_ERR_INVALID_ARGUMENT;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.mtiles = B * tiles_x * tiles_y; a.ntiles = ntiles;
    a.gm = gm < a.mtiles ? gm : a.mtiles; a.gn = gn < ntiles ? gn : ntiles; a.blk4 = blk4 ? 1 : 0;
    set_walk(a);
    std::vector<uint32_t> t;
    tile_list(a, th, tw, t);
    const int n = (int)(t.size() / 2);
    for (int i = 0; i < n && i < cap; ++i) { out[2 * i] = t[2 * i]; out[2 * i + 1] = t[2 * i + 1]; }
    return n;
}
// The layer that op (mz_debug_select's, include/mewzoom_hip.h; 8: the fused gate of a block's conv2) names, planned as the model and
// the mz_op_* entries plan it, inside b.  nullptr (mz_last_error() says why) for a bad op, a mix whose cin is not 2 cout, or the gate of
// a block that does not fuse.
static const ConvW* plan_debug_layer(BlockW& b, int dtype, int op, int cin, int cout) {
    switch (op) {
        case 0: case 1: case 4: case 5:  // conv1 + SiLU, plain 3x3, QA head, FiLM conv
            plan_conv(b.conv1, dtype, MODE_CONV3, cout, cin, 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0);
            return &b.conv1;
        case 2:  // SubpixelConv2d: 3x3 + PixelShuffle(2) into 2H x 2W
            plan_conv(b.conv1, dtype, MODE_CONV3, cout, cin, 3, 3, OUT_D2S, SRC_PLAIN, 0, 0);
            return &b.conv1;
        case 3:  // image head
            plan_conv(b.conv1, dtype, MODE_CONV3, cout, cin, 3, 3, OUT_FINAL, SRC_PLAIN, 0, 0);
            return &b.conv1;
        case 6: case 8:  // a block's conv2 (cin = the hidden channels), its fused gate
            plan_block(b, dtype, cout, cin);
            if (op == 6) return &b.conv2;
            if (b.fused) return &b.mixf;
            fail(MZ_ERR_INVALID_ARGUMENT, "the block does not fuse conv2 and the mix");
            return nullptr;
        case 7:  // unfused AdaptiveResidualMix of cout channels (cin = 2 cout)
            if (cin != 2 * cout) {
                fail(MZ_ERR_INVALID_ARGUMENT, "a mix has cin = 2 cout");
                return nullptr;
            }
            plan_conv(b.mix, dtype, MODE_GEMM1, cout, cin, 1, 1, OUT_PLAIN, SRC_CONCAT, cout, cout);
            return &b.mix;
    }
    fail(MZ_ERR_INVALID_ARGUMENT, "bad op %d", op);
    return nullptr;
}

// Host-only (no GPU): the kernel family Runner::conv3 / Runner::mix would launch for one layer -- the same role functions make the call,
// the same choose_* choose -- with the knobs read from the environment as the mz_op_* entries read them.
extern "C" const char* mz_debug_select(int dtype, int op, int cin, int cout, int B, int H, int W, int cus) {
    if ((dtype != MZ_F32 && dtype != MZ_BF16 && dtype != MZ_F16) || cin < 1 || cout < 1 || B < 1 || H < 1 || W < 1 || cus < 0) {
        fail(MZ_ERR_INVALID_ARGUMENT, "bad arguments");
        return nullptr;
    }
    if (op == 5 && dtype != DT_BF16 && dtype != DT_F16) {
        fail(MZ_ERR_INVALID_ARGUMENT, "the FiLM epilogue is implemented for bf16 / fp16");
        return nullptr;
    }
    if (op == 8) {  // the gate is no launch of its own
        fail(MZ_ERR_INVALID_ARGUMENT, "bad op %d", op);
        return nullptr;
    }
    const Knobs k = read_knobs();
    BlockW b;
    const ConvW* c = plan_debug_layer(b, dtype, op, cin, cout);
    if (!c) return nullptr;
    if (op == 7) return kernel_name(choose_mix(k, dtype, *c, B, H, W, cus));
    Conv3Call call;  // no launch: no buffers
    switch (op) {    // the public op codes -> the layer roles that mz_forward and the mz_op_* entries run
        case 0: call = conv1_call(*c, nullptr, nullptr, B, H, W); break;
        case 2: call = d2s_call(*c, nullptr, nullptr, B, H, W, 2 * H, 2 * W); break;
        case 3: call = head_call(*c, nullptr, nullptr, B, H, W); break;
        case 5: call = film_call(*c, nullptr, nullptr, B, H, W, 0); break;
        case 6: call = conv2_call(k, b, nullptr, nullptr, B, H, W); break;
        default: call = plain_call(*c, nullptr, nullptr, B, H, W); break;  // 1 plain, 4 the quality head's
    }
    return kernel_name(choose_conv3(k, dtype, call, cus));
}

// Host-only (no GPU): packing `layout` of one layer (mz_debug_select's ops; 8 = the fused gate of a block's conv2), as pack_kernel writes
// it: the OIHW source index of each packed element, -1 for padding.  Writes at most cap of them to out.
extern "C" long long mz_debug_pack(int dtype, int op, int cin, int cout, int layout, long long* out, long long cap) {
    if ((dtype != MZ_F32 && dtype != MZ_BF16 && dtype != MZ_F16) || cin < 1 || cout < 1 || layout < 0 || layout >= PK_COUNT || cap < 0 ||
        (cap > 0 && !out)) {
        fail(MZ_ERR_INVALID_ARGUMENT, "bad arguments");
        return -1;
    }
    BlockW b;
    const ConvW* c = plan_debug_layer(b, dtype, op, cin, cout);
    if (!c) return -1;
    if (!c->has(layout)) {
        fail(MZ_ERR_INVALID_ARGUMENT, "the layer has no packing %d", layout);
        return -1;
    }
    const PackArgs p = pack_args(*c, layout, dtype, nullptr, nullptr);
    const long long n = (long long)(packed_bytes(p.taps, p.frags, p.ntiles, p.nchunks) / dtype_size(dtype));
    for (long long i = 0; i < n && i < cap; ++i) out[i] = dtype == DT_F32 ? pack_source<4>(p, i) : pack_source<2>(p, i);
    return n;
}
extern "C" const char* mz_version(void) { return "mewzoom_hip 0.1 (gfx950)"; }

extern "C" double mz_flops_per_image(const mz_handle* h, int H, int W) {
    if (!h) return 0.0;
    const int hr = h->cfg.hidden_ratio;
    int hs[4] = {H, 0, 0, 0}, ws[4] = {W, 0, 0, 0};
    for (int i = 1; i < 4; ++i) { hs[i] = hs[i - 1] / 2; ws[i] = ws[i - 1] / 2; }
    double macs = 3.0 * h->ch[0] * H * W;
    auto blk = [&](double c) { return (18.0 * hr + 2.0) * c * c; };
    for (int l = 0; l < 4; ++l) macs += (h->enc[l] + h->dec[l]) * blk(h->ch[l]) * hs[l] * ws[l];
    for (int l = 0; l < 3; ++l) {
        macs += 4.0 * h->ch[l] * h->ch[l + 1] * hs[l + 1] * ws[l + 1];
        macs += 9.0 * h->ch[l + 1] * 4.0 * h->ch[l] * hs[l + 1] * ws[l + 1];
        macs += 2.0 * h->ch[l] * h->ch[l] * hs[l] * ws[l];
    }
    macs += 9.0 * h->ch[3] * h->cfg.num_deg_features * hs[3] * ws[3];
    double hh = H, ww = W;
    for (int i = 0; i < h->nhead; ++i) {
        const double cout = (i == h->nhead - 1) ? 3 : h->ch[0];
        macs += blk(h->ch[0]) * hh * ww + 9.0 * h->ch[0] * 4.0 * cout * hh * ww;
        hh *= 2; ww *= 2;
    }
    return 2.0 * macs;
}

extern "C" int mz_profile_enable(mz_handle* h, int on) {
    if (!h) return fail(MZ_ERR_INVALID_ARGUMENT, "null handle");
    h->prof = on != 0;
    h->recs_used = 0;
    return MZ_OK;
}

extern "C" int mz_profile_dump(mz_handle* h, const char* path) {
    // One CSV row per profiled launch since the last reset (does not reset).
    if (!h || !path) return fail(MZ_ERR_INVALID_ARGUMENT, "null argument");
    FILE* f = fopen(path, "w");
    if (!f) return fail(MZ_ERR_INVALID_ARGUMENT, "cannot open %s", path);
    fprintf(f, "kind,B,H,W,cin,cout,nt,ntiles,mtiles,n_fast,ms,gflop,tflops,alg_GBps\n");
    for (size_t i = 0; i < h->recs_used; ++i) {
        ProfRec& r = h->recs[i];
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
    for (size_t i = 0; i < h->recs_used; ++i) {
        ProfRec& r = h->recs[i];
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
    h->recs_used = 0;
    return MZ_OK;
}
