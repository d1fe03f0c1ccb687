// Running a planned layer: the device buffers of its weights (ConvW), what a launch needs beside the layer (LaunchCtx), and the Runner
// that turns a Conv3Call / a mix / a PixelCrush into ConvArgs and launches the kernel chosen.  Shared by the model runtime
// (mz_host.cpp) and the operator entries (mz_ops.cpp).
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <utility>

#include "mz_err.h"
#include "mz_select.h"

namespace mz {

// A device allocation that frees itself.
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }  // (so: no copies)
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return p ? hipSuccess : hipMalloc(&p, bytes); }  // once: a weight set again is packed in place
};

// a planned layer and its packed weights
struct ConvW : LayerPlan {
    DevBuf packed[PK_COUNT];
};
using BlockW = Block<ConvW>;
// every layer of a call that is run has its weights: the role functions (mz_select.h) were handed a ConvW / a BlockW
inline const ConvW& weights(const LayerPlan* c) { return *static_cast<const ConvW*>(c); }

// every planned packing, in PackLayout order
inline int pack_conv(ConvW& c, int dtype, const float* w_dev, hipStream_t s) {
    for (int l = 0; l < PK_COUNT; ++l) {
        if (!c.has(l)) continue;
        HIPCHK(c.packed[l].alloc(pack_bytes(c, l)));
        HIPCHK(launch_pack(pack_args(c, l, dtype, w_dev, c.packed[l].p), s));
    }
    return MZ_OK;
}

struct ProfRec {
    hipEvent_t a, b;
    double flops, bytes;
    int kind, B, H, W, cin, cout, nt, ntiles, mtiles, n_fast;  // kind: 0 conv3, 1 mix, 2 crush
};

// What a launch needs beside its layer and tensors; a model handle has one, an mz_op_* call makes one
struct LaunchCtx {
    DevBuf zero_page;
    Knobs knobs = read_knobs();
    // tile lists of the role-alternating kernels (Runner::tile_table): one per launch geometry, built on first use
    std::map<std::vector<int>, std::pair<DevBuf, int>> tile_tabs;
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    size_t recs_used = 0;
    // the zero page, filled on the CALLER's stream like every later use of it (a blocking memset on the NULL stream is not ordered
    // with work on a non-blocking stream)
    int init(hipStream_t s) {
        HIPCHK(zero_page.alloc(4096));
        HIPCHK(hipMemsetAsync(zero_page.p, 0, 4096, s));
        return MZ_OK;
    }
    ~LaunchCtx() {
        for (auto& r : recs) {
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
    }
};

// Diagnostic stamp buffer (only -DMZ_DIAG kernel builds write to it, mz_diag.h; MZ_DEBUG_STAMPS=1 allocates it).
inline unsigned long long* debug_buffer() {
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

// 1 / sigmoid(alpha) = 1 + e^-alpha for blend_() (mz_device.h), which folds the scale into the reciprocal of the gate's sigmoid:
// rcp(fma(e^-beta, inv_s, inv_s)).  Kept finite: for alpha < -88.7 the exact value overflows to +inf and fma(0, inf, inf) (a gate
// whose e^-beta flushed to 0) would be NaN where the reference (model.py:833-837) returns x; with FLT_MAX the weight is ~0 instead.
inline float inv_sigmoid(float alpha) {
    const float v = 1.0f + std::exp(-alpha);
    return std::isfinite(v) ? v : 3.402823466e+38f;
}

struct Runner {
    LaunchCtx& ctx;
    hipStream_t s;
    int dtype;
    int rc = MZ_OK;
    const Knobs knobs = ctx.knobs;
    int io_u8 = 0;                                        // images at both ends are uint8 (mz_forward_u8)
    int cus = std::max(0, device_cus());                  // 0 if unknown: no persistent launches

    // the profiling record of one launch (kind: 0 conv3, 1 mix, 2 crush); nullptr unless the context profiles
    ProfRec* prof_begin(int kind, const ConvArgs& a, const LayerPlan& c, double flops, double bytes) {
        if (!ctx.prof) return nullptr;
        if (ctx.recs_used == ctx.recs.size()) {
            ProfRec n;
            if (hipEventCreate(&n.a) != hipSuccess || hipEventCreate(&n.b) != hipSuccess) return nullptr;
            ctx.recs.push_back(n);
        }
        ProfRec* r = &ctx.recs[ctx.recs_used++];
        r->flops = flops; r->bytes = bytes;
        r->kind = kind; r->B = a.B; r->H = a.H; r->W = a.W; r->cin = c.cin; r->cout = c.cout; r->nt = c.nt; r->ntiles = a.ntiles;
        r->mtiles = a.mtiles; r->n_fast = a.gm * 1000 + a.gn;
        (void)hipEventRecord(r->a, s);
        return r;
    }

    int check(hipError_t e, const char* what) {
        if (e != hipSuccess && rc == MZ_OK) rc = hip_rc(e, what);
        return rc;
    }

    // what every launch says alike: the layer's main packing and chunk counts, its first input over B x H x W pixels, its output of
    // cp_out channels per pixel, its walk
    void base_args(ConvArgs& a, const ConvW& c, const void* in0, void* out, int B, int H, int W, int cp_out, const Walk& w) {
        memset(&a, 0, sizeof(a));
        a.wpk = c.packed[PK_MAIN].p;
        a.zero = ctx.zero_page.p;
        a.dbg = debug_buffer();
        a.nchunks = c.nchunks;
        a.nchunks_real = c.nchunks_real;
        a.in0 = in0; a.out = out;
        a.B = B; a.H = H; a.W = W; a.Ho = H; a.Wo = W;
        a.p0 = c.cp0 * dtype_size(dtype) / 16;
        a.cp_out = cp_out;
        a.p_out = a.cp_out * dtype_size(dtype) / 16;
        put_walk(a, w);
    }

    // conv3r_kernel / conv3t_kernel: the launch's tiles in walk order as a table in HBM (ConvArgs::tile_tab), so that the kernels'
    // helper role -- the critical path of their short tiles -- reads a tile's coordinates with one scalar load instead of running
    // the divisions of the group walk (tile_of / tile_rc, mz_device.h) three times per phase.  The order IS that walk's (tile_list(),
    // mz_select.h).  Sets a.tile_tab and a.grid (= tiles listed), padded for up to wgs workgroups.  One table per geometry, kept
    // with the context.
    void tile_table(ConvArgs& a, const Walk& w, int th, int tw, int wgs) {
        const int pad = 4 * ((wgs > 256 ? wgs : 256) / 8) + 8;
        const std::vector<int> key = {th, tw, a.B, w.tiles_x, w.tiles_y, w.ntiles, w.gm, w.gn, w.grid, w.blk4, pad};
        auto it = ctx.tile_tabs.find(key);
        if (it == ctx.tile_tabs.end()) {
            std::vector<uint32_t> t;
            t.reserve(2 * ((size_t)w.mtiles * w.ntiles + pad));
            tile_list(w, th, tw, t);
            const int n = (int)(t.size() / 2);
            t.resize(t.size() + 2 * (size_t)pad, 0u);
            DevBuf d;
            if (check(d.alloc(t.size() * 4), "tile table")) return;
            if (check(hipMemcpy(d.p, t.data(), t.size() * 4, hipMemcpyHostToDevice), "tile table upload")) return;
            it = ctx.tile_tabs.emplace(key, std::make_pair(std::move(d), n)).first;
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
        if (r) (void)hipEventRecord(r->b, s);
    }

    // conv3x3, pad 1 (model.py:742-748, 900-909, 1010)
    void conv3(const Conv3Call& k) {
        if (rc) return;
        const KernelChoice ch = choose_conv3(knobs, dtype, k, cus);
        if (!ch.ok) { rc = fail(MZ_ERR_INVALID_ARGUMENT, "%s", ch.why); return; }
        const ConvW& c = weights(k.c);
        const int B = k.B, H = k.H, W = k.W;
        const double sz = dtype_size(dtype);
        const double px = (double)B * H * W;
        const int tiles_x = (W + ch.tw - 1) / ch.tw, tiles_y = (H + ch.th - 1) / ch.th;
        const Walk w = pick_order(tiles_x, tiles_y, B * tiles_x * tiles_y, c.ntiles, (double)pack_bytes(c, PK_MAIN), px * c.cp0 * sz, knobs);
        ConvArgs a;
        base_args(a, c, k.in, k.out, B, H, W, k.epi == EPI_D2S ? c.cq_p : pad16(c.cout), w);
        a.src = SRC_PLAIN;
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
            a.wmix = weights(k.mixf).packed[PK_MAIN].p;
            a.mix_pieces = k.mixf->nchunks * k.mixf->nt;
            // room for the 8 compute waves' x fragments next to the gate weights in ring slots 1-2?
            const int slot = ch.mode == MODE_C3W16 ? stage_bytes<MODE_C3W16>(c.nt) : stage_bytes<MODE_C3W8>(c.nt);
            const int ncx = a.p1 / 2;
            a.x_via_lds = (a.mix_pieces * 1024 + 8 * ncx * 1024 <= 2 * slot) ? 1 : 0;
            a.mix_scale = 1.0f / (1.0f + std::exp(-k.alpha));
            a.inv_mix_scale = inv_sigmoid(k.alpha);
        }
        a.geo = ch.geo;
        a.ragged_planes = ch.ragged_planes;
        if (ch.layout != PK_MAIN) {
            a.wpk16 = c.packed[ch.layout].p;
            a.nchunks16 = pack_shape(c, ch.layout).nchunks;
            if (fused) a.wmix16 = weights(k.mixf).packed[ch.gate].p;
        }
        if (ch.tile_list) tile_table(a, w, ch.th, ch.tw, ch.persist);
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
        const int sz = dtype_size(dtype);
        const long long npix = (long long)B * H * W;
        // a packing of its own: 192-channel N tiles, x / z straight into MFMA operands (mix16_kernel / mix16b_kernel)
        const bool mix16 = ch.layout != PK_MAIN;
        const PackShape sh = pack_shape(c, ch.layout);
        ConvArgs a;
        base_args(a, c, x, out, B, H, W, pad16(c.cout),
                  pick_order(0, 0, (int)((npix + 255) / 256), sh.ntiles, (double)pack_bytes(c, PK_MAIN),
                             (double)npix * (c.cp0 + pad16(c.c1)) * sz, knobs, mix16 ? 32 : 64));
        a.in1 = z; a.p1 = pad16(c.c1) * sz / 16;
        a.nchunks0 = c.cp0 / chunk_channels(dtype);
        a.src = SRC_CONCAT;
        a.epi = EPI_MIX;
        a.mix_scale = 1.0f / (1.0f + std::exp(-alpha));
        a.inv_mix_scale = inv_sigmoid(alpha);
        if (mix16) {
            a.wpk16 = c.packed[ch.layout].p;
            a.nchunks16 = sh.nchunks;
        }
        launch(ch, a, c.nt, prof_begin(1, a, c, 2.0 * (double)npix * c.cin * c.cout, (double)npix * 3.0 * c.cout * sz));
    }

    // PixelCrush (model.py:857-863, 881-882): conv 2x2 stride 2, floors odd sizes
    void crush(const ConvW& c, const void* in, void* out, int B, int H, int W) {
        if (rc) return;
        const double sz = dtype_size(dtype);
        const long long npix = (long long)B * (H / 2) * (W / 2);
        ConvArgs a;
        base_args(a, c, in, out, B, H, W, pad16(c.cout),
                  pick_order(0, 0, (int)((npix + 255) / 256), c.ntiles, (double)pack_bytes(c, PK_MAIN), (double)B * H * W * c.cp0 * sz, knobs, 64));
        a.Ho = H / 2; a.Wo = W / 2;
        a.nchunks0 = c.cp0 / chunk_channels(dtype);
        a.src = SRC_CRUSH;
        a.epi = EPI_STORE;
        ProfRec* r = prof_begin(2, a, c, 2.0 * (double)npix * 4.0 * c.cin * c.cout, ((double)B * H * W * c.cin + (double)npix * c.cout) * sz);
        KernelChoice ch;  // conv_kernel's 1x1 mode is the only kernel that gathers the 2x2 patches
        ch.ok = true; ch.kernel = K_CONV256; ch.mode = MODE_GEMM1;
        launch(ch, a, c.nt, r, "crush launch");
    }
};

}  // namespace mz
