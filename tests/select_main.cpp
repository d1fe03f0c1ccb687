// Host-only driver of ultrazoom_amd/csrc/mz_plan.h and mz_select.h: layer plans, kernel choices, tile walks, tile lists and workspace
// plans over the layers of tests/test_select_cpu.py's table, channel counts around every tile and chunk boundary, shapes from 1 x 1 to
// 4320 x 7680 and 1 to 64 images.  tests/test_select_cpu.py compiles it with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=undefined and runs it: exit status 0 and no sanitizer report (a signed overflow in a tile count, an offset guard
// or a workspace size would abort it).  Nothing of the library is linked: the two headers call nothing in HIP.
#include <stdio.h>

#include <set>

#include "../ultrazoom_amd/csrc/mz_select.h"

using namespace mz;

static int g_failed = 0;
#define EXPECT(cond)                                                \
    do {                                                            \
        if (!(cond)) {                                              \
            if (++g_failed < 20) printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
        }                                                           \
    } while (0)

// every distinct (dtype, op, cin, cout) of tests/test_select_cpu.py's TABLE (ops: mz_debug_select's, include/mewzoom_hip.h)
static const int kTableLayers[][4] = {
    {0, 0, 48, 96}, {0, 0, 96, 192}, {0, 0, 192, 384}, {0, 0, 384, 768}, {0, 0, 768, 1536}, {0, 2, 96, 192}, {0, 2, 96, 384},
    {0, 2, 192, 384}, {0, 2, 384, 768}, {0, 2, 768, 1536}, {0, 3, 48, 12}, {0, 3, 96, 12}, {0, 4, 384, 3}, {0, 4, 768, 3},
    {0, 5, 96, 96}, {0, 6, 96, 48}, {0, 6, 192, 96}, {0, 6, 384, 192}, {0, 6, 768, 384}, {0, 6, 1536, 768}, {0, 7, 96, 48},
    {0, 7, 192, 96}, {0, 7, 384, 192}, {0, 7, 768, 384}, {0, 7, 1536, 768}, {1, 0, 16, 32}, {1, 0, 16, 64}, {1, 0, 24, 48},
    {1, 0, 32, 64}, {1, 0, 40, 80}, {1, 0, 48, 96}, {1, 0, 64, 128}, {1, 0, 72, 144}, {1, 0, 96, 48}, {1, 0, 96, 192},
    {1, 0, 128, 256}, {1, 0, 136, 272}, {1, 0, 192, 384}, {1, 0, 256, 512}, {1, 0, 384, 768}, {1, 0, 768, 1536}, {1, 1, 16, 16},
    {1, 1, 96, 96}, {1, 2, 16, 64}, {1, 2, 24, 96}, {1, 2, 32, 64}, {1, 2, 32, 128}, {1, 2, 40, 96}, {1, 2, 64, 128},
    {1, 2, 72, 160}, {1, 2, 96, 192}, {1, 2, 96, 384}, {1, 2, 128, 256}, {1, 2, 136, 288}, {1, 2, 192, 384}, {1, 2, 256, 512},
    {1, 2, 384, 768}, {1, 2, 768, 1536}, {1, 3, 16, 12}, {1, 3, 24, 12}, {1, 3, 32, 12}, {1, 3, 48, 12}, {1, 3, 96, 12},
    {1, 4, 128, 3}, {1, 4, 136, 3}, {1, 4, 256, 3}, {1, 4, 384, 3}, {1, 4, 768, 3}, {1, 5, 48, 96}, {1, 5, 96, 96}, {1, 6, 16, 16},
    {1, 6, 32, 16}, {1, 6, 48, 24}, {1, 6, 64, 16}, {1, 6, 64, 32}, {1, 6, 80, 40}, {1, 6, 96, 48}, {1, 6, 128, 64}, {1, 6, 144, 72},
    {1, 6, 192, 96}, {1, 6, 256, 128}, {1, 6, 272, 136}, {1, 6, 384, 192}, {1, 6, 512, 256}, {1, 6, 768, 384}, {1, 6, 1536, 768},
    {1, 7, 32, 16}, {1, 7, 48, 24}, {1, 7, 64, 32}, {1, 7, 80, 40}, {1, 7, 96, 48}, {1, 7, 128, 64}, {1, 7, 144, 72},
    {1, 7, 192, 96}, {1, 7, 256, 128}, {1, 7, 272, 136}, {1, 7, 384, 192}, {1, 7, 512, 256}, {1, 7, 768, 384}, {1, 7, 1536, 768},
    {2, 0, 16, 32}, {2, 0, 24, 48}, {2, 0, 32, 64}, {2, 0, 40, 80}, {2, 0, 64, 128}, {2, 0, 72, 144}, {2, 0, 96, 192},
    {2, 0, 128, 256}, {2, 0, 136, 272}, {2, 0, 192, 384}, {2, 0, 256, 512}, {2, 0, 384, 768}, {2, 0, 768, 1536}, {2, 2, 32, 64},
    {2, 2, 40, 96}, {2, 2, 64, 128}, {2, 2, 72, 160}, {2, 2, 96, 384}, {2, 2, 128, 256}, {2, 2, 136, 288}, {2, 2, 192, 384},
    {2, 2, 256, 512}, {2, 2, 384, 768}, {2, 2, 768, 1536}, {2, 3, 16, 12}, {2, 3, 24, 12}, {2, 3, 32, 12}, {2, 3, 96, 12},
    {2, 4, 128, 3}, {2, 4, 136, 3}, {2, 4, 256, 3}, {2, 4, 768, 3}, {2, 5, 32, 64}, {2, 6, 32, 16}, {2, 6, 48, 24}, {2, 6, 64, 32},
    {2, 6, 80, 40}, {2, 6, 128, 64}, {2, 6, 144, 72}, {2, 6, 192, 96}, {2, 6, 256, 128}, {2, 6, 272, 136}, {2, 6, 384, 192},
    {2, 6, 512, 256}, {2, 6, 768, 384}, {2, 6, 1536, 768}, {2, 7, 32, 16}, {2, 7, 48, 24}, {2, 7, 64, 32}, {2, 7, 80, 40},
    {2, 7, 128, 64}, {2, 7, 144, 72}, {2, 7, 192, 96}, {2, 7, 256, 128}, {2, 7, 272, 136}, {2, 7, 384, 192}, {2, 7, 512, 256},
    {2, 7, 768, 384}, {2, 7, 1536, 768},
};
static const int kChannels[] = {1, 15, 16, 17, 31, 32, 33, 48, 96, 191, 192, 193, 384, 768, 1536, 2047, 2048};
static const int kShapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 3}, {8, 8}, {9, 11}, {37, 45}, {67, 120}, {135, 240}, {540, 960}, {1080, 1920}, {2160, 3840}, {4320, 7680}};
static const int kBatches[] = {1, 3, 16, 64};
static const int kCus[] = {0, 8, 256};
// tile lists are built (once per geometry, as Runner::tile_table keeps them) where they have at most this many entries
static const long long kMaxListed = 1 << 21;

static std::set<std::vector<int>> g_listed;
static long long g_choices = 0, g_lists = 0;

// what tests/test_cabi_cpu.py asserts of mz_debug_tile_list: every (image, tile row, tile column, N tile) exactly once, origins on the grid
static void check_tile_list(const Walk& w, int B, int th, int tw) {
    const std::vector<int> key = {th, tw, B, w.tiles_x, w.tiles_y, w.ntiles, w.gm, w.gn, w.grid, w.blk4};
    if ((long long)w.mtiles * w.ntiles > kMaxListed || !g_listed.insert(key).second) return;
    std::vector<uint32_t> t;
    tile_list(w, th, tw, t);
    EXPECT((long long)t.size() == 2LL * w.mtiles * w.ntiles);
    std::vector<char> seen((size_t)w.mtiles * w.ntiles, 0);
    for (size_t i = 0; i + 1 < t.size(); i += 2) {
        const int y0 = t[i] & 0xFFFF, x0 = t[i] >> 16, b = t[i + 1] & 0xFFFF, nt = t[i + 1] >> 16;
        const bool in_range = y0 % th == 0 && x0 % tw == 0 && y0 / th < w.tiles_y && x0 / tw < w.tiles_x && b < B && nt < w.ntiles;
        EXPECT(in_range);
        if (!in_range) return;
        char& s = seen[(((size_t)b * w.tiles_y + y0 / th) * w.tiles_x + x0 / tw) * w.ntiles + nt];
        EXPECT(!s);
        s = 1;
    }
    ++g_lists;
}

// a walk covers its tiles with whole groups
static void check_walk(const Walk& w) {
    EXPECT(w.gm >= 1 && w.gn >= 1 && w.gm <= w.mtiles && w.gn <= w.ntiles);
    EXPECT((long long)w.groups_m * w.gm >= w.mtiles);
    EXPECT(w.grid >= 0 && (long long)w.grid >= (long long)w.mtiles * w.ntiles && w.grid % (w.gm * w.gn) == 0);
}

// one layer in its role on B x H x W pixels, as mz_debug_select and Runner::conv3 / mix / crush go about it
static void run_layer(const Knobs& k, int dtype, int op, int cin, int cout, int B, int H, int W, int cus) {
    if (op == 7 && cin != 2 * cout) return;                       // a mix has cin = 2 cout
    if (op == 5 && dtype == DT_F32) return;                       // mz_op_conv_film refuses f32 itself
    if (op == 2 && cout % 4 != 0) return;                         // PixelShuffle(2) of cout / 4 channels
    if (op == 3) cout = 12;                                       // the image head
    BlockPlan b;
    Refusal why;
    const LayerPlan* c = plan_debug_layer(b, dtype, op, cin, cout, &why);
    EXPECT(c && !why);
    if (!c) return;
    for (int l = 0; l < PK_COUNT; ++l)
        if (c->has(l)) EXPECT(pack_bytes(*c, l) > 0 && pack_args(*c, l, dtype, nullptr, nullptr).nchunks > 0);
    ++g_choices;
    const double sz = dtype_size(dtype);
    if (op == 7) {
        const KernelChoice ch = choose_mix(k, dtype, *c, B, H, W, cus);
        EXPECT(ch.ok && kernel_name(ch));
        const long long npix = (long long)B * H * W;
        check_walk(pick_order(0, 0, (int)((npix + 255) / 256), pack_shape(*c, ch.layout).ntiles, (double)pack_bytes(*c, PK_MAIN),
                              (double)npix * (c->cp0 + pad16(c->c1)) * sz, k, ch.layout != PK_MAIN ? 32 : 64));
        return;
    }
    Conv3Call call;
    switch (op) {
        case 0: call = conv1_call(*c, nullptr, nullptr, B, H, W); break;
        case 2: call = d2s_call(*c, nullptr, nullptr, B, H, W, 2 * H, 2 * W); break;
        case 3: call = head_call(*c, nullptr, nullptr, B, H, W); break;
        case 5: call = film_call(*c, nullptr, nullptr, B, H, W, 0); break;
        case 6: call = conv2_call(k, b, nullptr, nullptr, B, H, W); break;
        default: call = plain_call(*c, nullptr, nullptr, B, H, W); break;
    }
    const KernelChoice ch = choose_conv3(k, dtype, call, cus);
    EXPECT(ch.ok ? kernel_name(ch) != nullptr && !ch.why : ch.why != nullptr && (call.film || ch.tile_list));
    if (!ch.ok) return;
    const int tiles_x = (W + ch.tw - 1) / ch.tw, tiles_y = (H + ch.th - 1) / ch.th;
    const Walk w = pick_order(tiles_x, tiles_y, B * tiles_x * tiles_y, c->ntiles, (double)pack_bytes(*c, PK_MAIN), (double)B * H * W * c->cp0 * sz, k);
    check_walk(w);
    if (ch.tile_list) check_tile_list(w, B, ch.th, ch.tw);
}

// offsets of a workspace plan: 256-aligned, ascending, each buffer ending before the next begins
static void check_plan(const ModelDims& m, int B, int H, int W) {
    Plan p;
    const int nb = default_micro_batch(m, B, H, W, 0);
    EXPECT(nb >= 1 && nb <= B);
    make_plan(m, nb, H, W, p);
    const size_t sz = dtype_size(m.dtype);
    std::vector<std::pair<size_t, size_t>> bufs;  // offset, bytes, in the order make_plan takes them
    for (int l = 0; l < 4; ++l) {
        const size_t px = (size_t)nb * p.hs[l] * p.ws[l], c = px * pad16(m.ch[l]) * sz;
        for (int i = 0; i < 3; ++i) bufs.push_back({p.R[l][i], c});
        bufs.push_back({p.HID[l], px * pad16(m.hidden_ratio * m.ch[l]) * sz});
        bufs.push_back({p.Z[l], c});
        if (l < 3) bufs.push_back({p.U[l], c});
    }
    for (int j = 1; j < m.nhead; ++j) {
        const size_t px = (size_t)nb * ((size_t)H << j) * ((size_t)W << j), c = px * pad16(m.ch[0]) * sz;
        bufs.push_back({p.HR[j][0], c});
        bufs.push_back({p.HR[j][1], c});
        bufs.push_back({p.HHID[j], px * pad16(m.hidden_ratio * m.ch[0]) * sz});
        bufs.push_back({p.HZ[j], c});
    }
    bufs.push_back({p.QA, (size_t)nb * p.hs[3] * p.ws[3] * pad16(m.num_deg_features) * sz});
    for (size_t i = 0; i < bufs.size(); ++i) {
        EXPECT(bufs[i].first % 256 == 0 && bufs[i].second > 0);
        EXPECT(bufs[i].first + bufs[i].second <= (i + 1 < bufs.size() ? bufs[i + 1].first : p.total));
    }
    EXPECT(bufs[0].first == 0 && p.total % 256 == 0);
}

int main() {
    Knobs other;  // row-major tile walk, eight persistent workgroups
    other.blk4 = 0; other.persist = 8;
    const Knobs knobs[] = {Knobs(), other};
    for (const Knobs& k : knobs)
        for (int cus : kCus) {
            // the table's layers at every shape and batch
            for (const auto& l : kTableLayers)
                for (const auto& s : kShapes)
                    for (int B : kBatches) run_layer(k, l[0], l[1], l[2], l[3], B, s[0], s[1], cus);
            // every role at channel counts around the 16 / 32 / 48 / 96 / 192 boundaries, at the ends and the middle of the shapes
            for (int dtype = 0; dtype < 3; ++dtype)
                for (int op = 0; op < 8; ++op)
                    for (int cin : kChannels)
                        for (int cout : kChannels)
                            for (int si : {0, 3, 4, 6, 8, 12})
                                for (int B : {1, 64}) run_layer(k, dtype, op, op == 7 ? 2 * cout : cin, cout, B, kShapes[si][0], kShapes[si][1], cus);
        }
    // refusals name themselves
    BlockPlan b;
    Refusal why;
    EXPECT(!plan_debug_layer(b, DT_BF16, 9, 96, 96, &why) && why.code == MZ_ERR_INVALID_ARGUMENT && why.msg[0]);
    EXPECT(!plan_debug_layer(b, DT_BF16, 7, 96, 96, &why) && why.msg[0]);
    EXPECT(!plan_debug_layer(b, DT_BF16, 8, 768, 384, &why) && why.msg[0]);
    // the workspace of bench.py's three workloads, every dtype
    for (int dtype = 0; dtype < 3; ++dtype) {
        check_plan({dtype, {96, 192, 384, 768}, 2, 2, 3}, 16, 1080, 1920);  // cfg3_1080p
        check_plan({dtype, {96, 192, 384, 768}, 2, 2, 3}, 16, 540, 960);    // cfg3_540p
        check_plan({dtype, {48, 96, 192, 384}, 2, 1, 3}, 32, 540, 960);     // cfg2
        check_plan({dtype, {16, 32, 64, 128}, 4, 3, 3}, 64, 8, 8);          // the smallest image, 8X
    }
    printf("%lld layer calls, %lld tile lists\n", g_choices, g_lists);
    if (g_failed) return 1;
    printf("selection OK\n");
    return 0;
}
