// Kernel selection: which kernel runs a 3x3 convolution or a mix, in which geometry, and the tile walk of a launch.  Functions of the
// plan (LayerPlan::has(), never whether a buffer happens to be allocated), the knobs, the shape and the CU count only.  Like mz_plan.h
// this calls nothing in HIP and touches no error state -- a refusal travels in KernelChoice::why --, so mz_debug_select() runs it
// without a GPU (tests/test_select_cpu.py pins its table) and tests/select_main.cpp under the sanitizers.
#pragma once
#include <math.h>

#include <vector>

#include "mz_plan.h"
#include "mz_view_check.h"

namespace mz {

// ---- the tile walk ------------------------------------------------------------------------------
// How a launch walks its mtiles pixel tiles x ntiles N tiles: ids 0 .. grid - 1 in groups of gm x gn (mz_device.h: tile_of / tile_rc)
struct Walk {
    int tiles_x = 0, tiles_y = 0;  // 3x3: tiles per image; 0: pixel tiles are runs of 256 pixels
    int mtiles = 0, ntiles = 0;
    int gm = 1, gn = 1, groups_m = 0, grid = 0;  // grid: whole groups, padding ids included
    int blk4 = 0;  // the tiles of an image in block rows of four tile rows: conv3s_kernel, and the tile lists of conv3r / conv3t
    float inv_gsz = 1.f, inv_groups_m = 1.f, inv_gn = 1.f, inv_tpi = 1.f, inv_tiles_x = 1.f, inv_bsz = 1.f;
};

// the walk in groups of gm pixel tiles x gn N tiles
inline Walk group_walk(int tiles_x, int tiles_y, int mtiles, int ntiles, int gm, int gn, int blk4) {
    Walk w;
    w.tiles_x = tiles_x; w.tiles_y = tiles_y; w.mtiles = mtiles; w.ntiles = ntiles;
    w.gm = gm; w.gn = gn; w.blk4 = blk4;
    w.groups_m = (mtiles + gm - 1) / gm;
    w.grid = (int)((long long)w.groups_m * ((ntiles + gn - 1) / gn) * gm * gn);
    w.inv_gsz = 1.0f / (float)(gm * gn);
    w.inv_groups_m = 1.0f / (float)w.groups_m;
    w.inv_gn = 1.0f / (float)gn;
    if (tiles_x > 0) {
        w.inv_tpi = 1.0f / (float)(tiles_x * tiles_y);
        w.inv_tiles_x = 1.0f / (float)tiles_x;
        w.inv_bsz = 1.0f / (float)(4 * tiles_x);
    }
    return w;
}

// Tile groups of gm pixel tiles x gn N tiles (gm * gn ~ the workgroups resident on one XCD): inside a group both operands are shared
// through the XCD's L2; per group the activations are re-read ntiles/gn times and the weights mtiles/gm times in total.  Picks the shape
// with the least total re-read traffic.
inline Walk pick_order(int tiles_x, int tiles_y, int mtiles, int ntiles, double weight_bytes, double act_bytes, const Knobs& k,
                       int resident_per_xcd = 32) {
    int best_gm = mtiles, best_gn = 1;
    double best = 1e300;
    for (int gn = 1; gn <= ntiles; ++gn) {
        if (gn > resident_per_xcd) break;
        if (ntiles % gn != 0 && gn != ntiles) continue;
        int gm = resident_per_xcd / gn;
        if (gm < 1) gm = 1;
        if (gm > mtiles) gm = mtiles;
        const double groups_n = ceil((double)ntiles / gn), groups_m = ceil((double)mtiles / gm);
        const double traffic = act_bytes * groups_n + weight_bytes * groups_m;
        if (traffic < best) { best = traffic; best_gm = gm; best_gn = gn; }
    }
    return group_walk(tiles_x, tiles_y, mtiles, ntiles, best_gm, best_gn, k.blk4 && tiles_x > 0 && 4 * tiles_x < 65536 ? 1 : 0);
}

inline void put_walk(ConvArgs& a, const Walk& w) {
    a.tiles_x = w.tiles_x; a.tiles_y = w.tiles_y; a.mtiles = w.mtiles; a.ntiles = w.ntiles;
    a.gm = w.gm; a.gn = w.gn; a.groups_m = w.groups_m; a.grid = w.grid; a.blk4 = w.blk4;
    a.inv_gsz = w.inv_gsz; a.inv_groups_m = w.inv_groups_m; a.inv_gn = w.inv_gn;
    a.inv_tpi = w.inv_tpi; a.inv_tiles_x = w.inv_tiles_x; a.inv_bsz = w.inv_bsz;
}

// The tiles of a launch in walk order, two words each: {y0 | x0 << 16, image | N tile << 16}.  The order is the group walk of
// mz_device.h (tile_of / tile_rc): ids 0 .. grid - 1 in groups of gm pixel tiles x gn N tiles, the tiles of an image in block rows of
// four tile rows where blk4 is set, padding ids of partial groups dropped.
inline void tile_list(const Walk& a, int th, int tw, std::vector<uint32_t>& t) {
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

// ---- the choice ---------------------------------------------------------------------------------
struct KernelChoice {
    bool ok = false;             // false = the launch is refused ...
    const char* why = nullptr;   // ... and why: the caller's MZ_ERR_INVALID_ARGUMENT message
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
inline const char* kernel_name(const KernelChoice& ch) {
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
inline int persistent_workgroups(const Knobs& k, int cus) { return k.persist >= 0 ? k.persist : cus; }

// 32-bit buffer offsets: `planes` 16-byte channel planes of `pixels` pixels stay below 4 GiB
inline bool offsets_fit(double planes, double pixels) { return planes * pixels * 16.0 < 4294967296.0; }

// One 3x3 layer call (conv3x3, pad 1): choose_conv3 reads the fields down to Wout, Runner::conv3 all of them.  The role functions below
// are the ONE place that says what a conv1, a block's conv2, a sub-pixel conv, .. is -- for mz_forward, the mz_op_* entries and
// mz_debug_select (which names no buffers) alike.
struct Conv3Call {
    const LayerPlan* c = nullptr;     // a ConvW (mz_runner.h) in every call that is run
    const LayerPlan* mixf = nullptr;  // EPI_FUSEDMIX: the block's gate weights
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
inline Conv3Call plain_call(const LayerPlan& c, const void* in, void* out, int B, int H, int W) {
    Conv3Call k;
    k.c = &c; k.in = in; k.out = out; k.B = B; k.H = H; k.W = W;
    return k;
}
// conv1 of a block + SiLU (model.py:742-744)
inline Conv3Call conv1_call(const LayerPlan& c, const void* in, void* out, int B, int H, int W) {
    Conv3Call k = plain_call(c, in, out, B, H, W);
    k.silu = 1;
    return k;
}
// SubpixelConv2d: 3x3 + PixelShuffle(2) into Hout x Wout (model.py:900-911)
inline Conv3Call d2s_call(const LayerPlan& c, const void* in, void* out, int B, int H, int W, int Hout, int Wout) {
    Conv3Call k = plain_call(c, in, out, B, H, W);
    k.epi = EPI_D2S; k.Hout = Hout; k.Wout = Wout;
    return k;
}
// the image head: 3x3 to 12 channels + PixelShuffle(2) + bicubic skip + add (+ clamp) into 2H x 2W (model.py:926-930, 156, 162, 177);
// the caller names img, R and clamp
inline Conv3Call head_call(const LayerPlan& c, const void* in, void* out, int B, int H, int W) {
    Conv3Call k = plain_call(c, in, out, B, H, W);
    k.epi = EPI_FINAL; k.Hout = 2 * H; k.Wout = 2 * W;
    return k;
}
// 3x3 + FiLM + optional SiLU (mz_op_conv_film); the caller names gamma and beta
inline Conv3Call film_call(const LayerPlan& c, const void* in, void* out, int B, int H, int W, int silu) {
    Conv3Call k = plain_call(c, in, out, B, H, W);
    k.film = true; k.silu = silu;
    return k;
}
// conv2 of a block + AdaptiveResidualMix with the block input xin in one launch (model.py:746-748, 826-839)
template <class Layer> Conv3Call fused_call(const Block<Layer>& b, const void* in, const void* xin, void* out, int B, int H, int W) {
    Conv3Call k = plain_call(b.conv2, in, out, B, H, W);
    k.epi = EPI_FUSEDMIX; k.mixf = &b.mixf; k.xin = xin; k.alpha = b.alpha;
    return k;
}
// conv2 of a block as mz_forward runs it: fused with the mix (mixf set) -- all output channels in one workgroup (Block::fused), on the
// 512-pixel kernels --, or plain and the caller runs the mix.  Where the output goes depends on which: the caller names out
template <class Layer> Conv3Call conv2_call(const Knobs& k, const Block<Layer>& b, const void* in, const void* xin, int B, int H, int W) {
    return b.fused && k.wide && k.fuse ? fused_call(b, in, xin, nullptr, B, H, W) : plain_call(b.conv2, in, nullptr, B, H, W);
}

inline KernelChoice choose_conv3(const Knobs& k, int dtype, const Conv3Call& call, int cus) {
    KernelChoice ch;
    const LayerPlan& c = *call.c;
    const LayerPlan* mixf = call.mixf;
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
        if (!ch.ok) ch.why = "tile table: image, batch or N-tile index beyond 16 bits";
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
        const int tiles_x = (W + tw - 1) / tw, tiles_y = (H + th - 1) / th;
        const Walk g = pick_order(tiles_x, tiles_y, B * tiles_x * tiles_y, c.ntiles, (double)pack_bytes(c, PK_MAIN),
                                  (double)B * H * W * c.cp0 * (double)dtype_size(dtype), k);  // the per-tile grid
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
        ch.why = "the FiLM epilogue exists on the 16x16x32 kernel only: bf16 / fp16, at most 96 output channels per "
                 "N tile, input channels within 12.5 % of a multiple of 32";
        return ch;
    }
    // conv3p has no fused variant: a fused layer off the 16x16x32 kernels stays on the per-tile kernel (kernel_name() has the history)
    ch.kernel = mode == MODE_CONV3 ? K_CONV256 : ch.persist == 0 || (fused && ch.layout == PK_MAIN) ? K_CONV3W : ch.layout != PK_MAIN ? K_CONV3S : K_CONV3P;
    ch.ok = true;
    return ch;
}

// AdaptiveResidualMix of C channels (c: the [C, 2C] gate weights, SRC_CONCAT) over B x H x W pixels
inline KernelChoice choose_mix(const Knobs& k, int dtype, const LayerPlan& c, int B, int H, int W, int cus) {
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

// The layer that op (mz_debug_select's, include/mewzoom_hip.h; 8: the fused gate of a block's conv2) names, planned as the model and
// the mz_op_* entries plan it, inside b.  nullptr (*why says why) for a bad op, a mix whose cin is not 2 cout, or the gate of a block that
// does not fuse.
inline const LayerPlan* plan_debug_layer(BlockPlan& b, int dtype, int op, int cin, int cout, Refusal* why) {
    switch (op) {
        // conv1 + SiLU, plain 3x3, SubpixelConv2d (2: 3x3 + PixelShuffle(2) into 2H x 2W), image head (3), QA head, FiLM conv
        case 0: case 1: case 2: case 3: case 4: case 5:
            plan_conv(b.conv1, dtype, MODE_CONV3, cout, cin, 3, 3, op == 2 ? OUT_D2S : op == 3 ? OUT_FINAL : OUT_PLAIN, SRC_PLAIN, 0, 0);
            return &b.conv1;
        case 6: case 8:  // a block's conv2 (cin = the hidden channels), its fused gate
            plan_block(b, dtype, cout, cin);
            if (op == 6) return &b.conv2;
            if (b.fused) return &b.mixf;
            *why = refuse(MZ_ERR_INVALID_ARGUMENT, "the block does not fuse conv2 and the mix");
            return nullptr;
        case 7:  // unfused AdaptiveResidualMix of cout channels (cin = 2 cout)
            if (cin == 2 * cout) {
                plan_conv(b.mix, dtype, MODE_GEMM1, cout, cin, 1, 1, OUT_PLAIN, SRC_CONCAT, cout, cout);
                return &b.mix;
            }
            *why = refuse(MZ_ERR_INVALID_ARGUMENT, "a mix has cin = 2 cout");
            return nullptr;
    }
    *why = refuse(MZ_ERR_INVALID_ARGUMENT, "bad op %d", op);
    return nullptr;
}

}  // namespace mz
