// What the host decides about a model before anything touches the GPU: the environment knobs, the plan of each layer (shapes, tiles,
// chunks, which packings), and the workspace plan.  Calls nothing in HIP and reports nothing through the error state: plain g++
// compiles it, tests/select_main.cpp runs it under the sanitizers.  The buffers of a planned layer are ConvW's (mz_runner.h).
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "mz_geo.h"

namespace mz {

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
inline Knobs read_knobs() {
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

// ---- the plan of one layer ----------------------------------------------------------------------
struct LayerPlan {
    // logical (reference) shape
    int cout = 0, cin = 0, kh = 0, kw = 0;
    // kernel selection
    int mode = MODE_CONV3, taps = 9, nt = 1, ntiles = 1, nchunks = 1, nchunks_real = 1;
    int out_map = OUT_PLAIN, cq = 0, cq_p = 0;
    int in_map = SRC_PLAIN, c0 = 0, cp0 = 0, c1 = 0;
    int n_logical_padded = 0;
    int nchunks32 = 0;     // 32-channel chunks of in0: the K steps of the 16x16x32 kernels over cp0
    unsigned layouts = 0;  // the planned packings, one bit per PackLayout
    bool has(int layout) const { return layouts >> layout & 1u; }
};

// One packing of a layer: fragments per tap and N tile, N tiles, K chunks (PackArgs; ConvArgs::nchunks16 of the 16-bit layouts)
struct PackShape { int frags, ntiles, nchunks; };
inline PackShape pack_shape(const LayerPlan& c, int layout) {
    switch (layout) {
        case PK_MAIN: return {c.nt, c.ntiles, c.nchunks};
        case PK_CONV16: return {2 * c.nt, c.ntiles, c.nchunks32};
        case PK_MIX16: case PK_MIX16B: return {12, c.cout / 192, 2 * c.cout / 32};  // 192-channel N tiles over [x ; z]
        case PK_GATE16: case PK_GATE16R: return {2 * c.nt, 1, c.nchunks32 + c.nt};   // x K steps, then one per pair of z fragments
        case PK_CONV16T: return {3, 1, c.nchunks32};
        default: return {3, 1, 3};  // PK_GATE16T: three K steps x three fragments
    }
}
inline size_t pack_bytes(const LayerPlan& c, int layout) {
    const PackShape sh = pack_shape(c, layout);
    return packed_bytes(c.taps, sh.frags, sh.ntiles, sh.nchunks);
}
inline PackArgs pack_args(const LayerPlan& c, int layout, int dtype, const float* w_dev, void* dst) {
    const PackShape sh = pack_shape(c, layout);
    PackArgs p;
    p.w = w_dev; p.dst = dst; p.dtype = dtype; p.layout = layout;
    p.cout = c.cout; p.cin = c.cin; p.kh = c.kh; p.kw = c.kw;
    p.taps = c.taps; p.frags = sh.frags; p.ntiles = sh.ntiles; p.nchunks = sh.nchunks;
    p.out_map = c.out_map; p.cq = c.cq; p.cq_p = c.cq_p;
    p.in_map = c.in_map; p.c0 = c.c0; p.cp0 = c.cp0; p.c1 = c.c1;
    return p;
}

inline void plan_conv(LayerPlan& c, int dtype, int mode, int cout, int cin, int kh, int kw, int out_map, int in_map, int c0, int c1) {
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

// The gate weights of a block's mix once more, packed for the fused conv2 + mix epilogue (SRC_MIXF) in conv2's N tile
inline void plan_mixf(LayerPlan& f, int dtype, const LayerPlan& conv2) {
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

// EncoderBlock / DecoderBlock: Layer = LayerPlan where a block is only planned, ConvW (mz_runner.h) where its weights are loaded too
template <class Layer> struct Block {
    Layer conv1, conv2, mix;
    Layer mixf;          // the gate weights once more, packed for the fused conv2 + mix epilogue (SRC_MIXF)
    bool fused = false;  // conv2 keeps all its output channels in one workgroup (<= 96): the mix runs in its epilogue
    float alpha = 0.f;
};
using BlockPlan = Block<LayerPlan>;

// a block of c channels with `hidden` channels between its two convolutions
template <class Layer> void plan_block(Block<Layer>& b, int dtype, int c, int hidden) {
    plan_conv(b.conv1, dtype, MODE_CONV3, hidden, c, 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0);      // model.py:742-744
    plan_conv(b.conv2, dtype, MODE_CONV3, c, hidden, 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0);      // model.py:746-748
    plan_conv(b.mix, dtype, MODE_GEMM1, c, 2 * c, 1, 1, OUT_PLAIN, SRC_CONCAT, c, c);        // model.py:805
    b.fused = b.conv2.ntiles == 1 && b.conv2.nt <= 3;
    if (b.fused) plan_mixf(b.mixf, dtype, b.conv2);
}

// ---- the model ----------------------------------------------------------------------------------
// what of a model sizes its layers and its workspace
struct ModelDims { int dtype, ch[4], hidden_ratio, nhead, num_deg_features; };

// Every layer of a MewZoom: Layer as for Block.  Level l = 0..3 has ch[l] channels at 1 / 2^l of the image; decoder stage d runs
// level 3 - d (the reference's decoder stage1 is the coarsest level, model.py:290-300).
template <class Layer> struct Model {
    int enc[4], dec[4];  // blocks per level
    std::vector<Block<Layer>> enc_blocks[4], dec_blocks[4], head_blocks;  // dec_blocks[d]; one head block per head level
    Layer crush[3], up[3], skipmix[3];  // crush[l]: level l -> l + 1; up[d - 1], skipmix[d - 1]: into decoder stage d
    float skip_alpha[3] = {0, 0, 0};
    std::vector<Layer> head_up;
    Layer qa_conv;
};

// Plans every layer of the model; layers[l] blocks on level l, the encoder's half rounded up (model.py:277-300).  The vectors get
// their final size here: a block or a layer stays where it is (mz_create's registry points at them).
template <class Layer> void plan_model(Model<Layer>& m, const ModelDims& d, const int layers[4]) {
    const int* ch = d.ch;
    auto plan_blocks = [&](std::vector<Block<Layer>>& blocks, int n, int c) {
        blocks = std::vector<Block<Layer>>(n);
        for (auto& b : blocks) plan_block(b, d.dtype, c, d.hidden_ratio * c);
    };
    for (int l = 0; l < 4; ++l) {
        m.enc[l] = (layers[l] + 1) / 2;  // ceil, model.py:277-288
        m.dec[l] = layers[l] / 2;        // floor, model.py:290-300
        plan_blocks(m.enc_blocks[l], m.enc[l], ch[l]);
        plan_blocks(m.dec_blocks[3 - l], m.dec[l], ch[l]);
    }
    for (int l = 0; l < 3; ++l)  // model.py:388-390, 857-863
        plan_conv(m.crush[l], d.dtype, MODE_GEMM1, ch[l + 1], ch[l], 2, 2, OUT_PLAIN, SRC_CRUSH, 0, 0);
    plan_conv(m.qa_conv, d.dtype, MODE_CONV3, d.num_deg_features, ch[3], 3, 3, OUT_PLAIN, SRC_PLAIN, 0, 0);  // model.py:1010
    for (int i = 0; i < 3; ++i) {
        const int cin = ch[3 - i], cout = ch[2 - i];
        plan_conv(m.up[i], d.dtype, MODE_CONV3, 4 * cout, cin, 3, 3, OUT_D2S, SRC_PLAIN, 0, 0);              // model.py:569-571, 900-911
        plan_conv(m.skipmix[i], d.dtype, MODE_GEMM1, cout, 2 * cout, 1, 1, OUT_PLAIN, SRC_CONCAT, cout, cout);  // model.py:573-575
    }
    plan_blocks(m.head_blocks, d.nhead, ch[0]);  // model.py:945-954, 981-983
    m.head_up = std::vector<Layer>(d.nhead);
    for (int i = 0; i < d.nhead; ++i) {
        const bool last = i == d.nhead - 1;
        plan_conv(m.head_up[i], d.dtype, MODE_CONV3, 4 * (last ? 3 : ch[0]), ch[0], 3, 3, last ? OUT_FINAL : OUT_D2S, SRC_PLAIN, 0, 0);
    }
}

// ---- workspace plan -----------------------------------------------------------------------------
struct Plan {
    int nb;                // images per micro-batch
    int hs[4], ws[4];      // level sizes
    size_t R[4][3], HID[4], Z[4], U[3];
    size_t HR[3][2], HHID[3], HZ[3];  // head levels 1..nhead-1 (index j-1... stored at j)
    size_t QA;
    size_t total;
};

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

inline void make_plan(const ModelDims& m, int nb, int H, int W, Plan& p) {
    const size_t sz = dtype_size(m.dtype);
    const int hr = m.hidden_ratio;
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
        const size_t c = px * pad16(m.ch[l]) * sz;
        for (int k = 0; k < 3; ++k) p.R[l][k] = take(c);
        p.HID[l] = take(px * pad16(hr * m.ch[l]) * sz);
        p.Z[l] = take(c);
        if (l < 3) p.U[l] = take(c);
    }
    for (int j = 1; j < m.nhead; ++j) {
        const size_t px = (size_t)nb * ((size_t)H << j) * ((size_t)W << j);
        const size_t c = px * pad16(m.ch[0]) * sz;
        p.HR[j][0] = take(c);
        p.HR[j][1] = take(c);
        p.HHID[j] = take(px * pad16(hr * m.ch[0]) * sz);
        p.HZ[j] = take(c);
    }
    p.QA = take((size_t)nb * p.hs[3] * p.ws[3] * pad16(m.num_deg_features) * sz);
    p.total = off;
}

inline int default_micro_batch(const ModelDims& m, int B, int H, int W, int requested) {
    if (requested > 0) return std::min(B, requested);
    // keep a micro-batch's workspace around <= 48 GiB by default (288 GB of HBM per GPU)
    Plan p;
    make_plan(m, 1, H, W, p);
    const size_t budget = (size_t)48 << 30;
    int nb = (int)std::max<size_t>(1, budget / std::max<size_t>(1, p.total));
    return std::max(1, std::min(B, nb));
}

}  // namespace mz
