// Host-only driver of ultrazoom_amd/csrc/mz_plan.h, mz_select.h and mz_schedule.h: planned models and their schedules (liveness and
// extents of every operand) for the fixture configurations and bench.py's models, then layer plans, kernel choices, tile walks and tile
// lists over the layers of those schedules, channel counts around every tile and chunk boundary, shapes from 1 x 1 to 4320 x 7680 and
// 1 to 64 images.  tests/test_select_cpu.py compiles it with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=undefined and runs it: exit status 0 and no sanitizer report (a signed overflow in a tile count, an offset guard
// or a workspace size would abort it).  Nothing of the library is linked: the three headers call nothing in HIP.
#include <stdio.h>

#include <array>
#include <set>

#include "../ultrazoom_amd/csrc/mz_schedule.h"

using namespace mz;

static int g_failed = 0;
#define EXPECT(cond)                                                \
    do {                                                            \
        if (!(cond)) {                                              \
            if (++g_failed < 20) printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
        }                                                           \
    } while (0)

// the models whose schedules are built: the fixtures' configurations (2X / 4X / 8X; C = 16, 24, 32; hidden ratio 1, 2, 4) and bench.py's two
struct Config { int ratio, ch[4], layers[4], hidden_ratio, features; };
static const Config kFixtures[] = {
    {2, {16, 32, 64, 128}, {2, 2, 2, 2}, 2, 3}, {4, {16, 32, 64, 128}, {2, 2, 2, 2}, 2, 3}, {8, {16, 32, 64, 128}, {2, 2, 2, 2}, 2, 3},
    {2, {16, 32, 64, 128}, {2, 2, 2, 2}, 1, 3}, {2, {16, 32, 64, 128}, {2, 2, 2, 2}, 4, 3}, {2, {16, 32, 64, 128}, {3, 2, 5, 4}, 2, 3},
    {2, {24, 40, 72, 136}, {2, 2, 2, 2}, 2, 5}, {4, {24, 40, 72, 136}, {2, 2, 2, 2}, 2, 3}, {4, {32, 64, 128, 256}, {2, 2, 2, 4}, 2, 3},
};
static const Config kBench[] = {
    {4, {96, 192, 384, 768}, {8, 8, 8, 16}, 2, 3},  // cfg3
    {2, {48, 96, 192, 384}, {4, 4, 4, 8}, 2, 3},    // cfg2
};
// (dtype, op, cin, cout) of tests/test_select_cpu.py's knob, tile-shape and FiLM rows that no schedule above has (ops: mz_debug_select's)
static const int kExtraLayers[][4] = {
    {0, 5, 96, 96}, {1, 0, 96, 48}, {1, 1, 16, 16}, {1, 1, 96, 96}, {1, 5, 48, 96}, {1, 5, 96, 96}, {2, 5, 32, 64},
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

// the buffers of a workspace plan as {offset, bytes}, in the order make_plan takes them: 256-aligned, ascending, each ending before the next
static std::vector<std::pair<size_t, size_t>> check_plan(const ModelDims& m, const Plan& p) {
    const size_t sz = dtype_size(m.dtype), nb = p.nb;
    std::vector<std::pair<size_t, size_t>> bufs;
    for (int l = 0; l < 4; ++l) {
        const size_t px = nb * p.hs[l] * p.ws[l], c = px * pad16(m.ch[l]) * sz;
        for (int i = 0; i < 3; ++i) bufs.push_back({p.R[l][i], c});
        bufs.push_back({p.HID[l], px * pad16(m.hidden_ratio * m.ch[l]) * sz});
        bufs.push_back({p.Z[l], c});
        if (l < 3) bufs.push_back({p.U[l], c});
    }
    for (int j = 1; j < m.nhead; ++j) {
        const size_t px = nb * ((size_t)p.hs[0] << j) * ((size_t)p.ws[0] << j), c = px * pad16(m.ch[0]) * sz;
        bufs.push_back({p.HR[j][0], c});
        bufs.push_back({p.HR[j][1], c});
        bufs.push_back({p.HHID[j], px * pad16(m.hidden_ratio * m.ch[0]) * sz});
        bufs.push_back({p.HZ[j], c});
    }
    bufs.push_back({p.QA, nb * p.hs[3] * p.ws[3] * pad16(m.num_deg_features) * sz});
    for (size_t i = 0; i < bufs.size(); ++i) {
        EXPECT(bufs[i].first % 256 == 0 && bufs[i].second > 0);
        EXPECT(bufs[i].first + bufs[i].second <= (i + 1 < bufs.size() ? bufs[i + 1].first : p.total));
    }
    EXPECT(bufs[0].first == 0 && p.total % 256 == 0);
    return bufs;
}

static std::set<std::array<int, 4>> g_layers;  // (dtype, op, cin, cout) of every 3x3 / mix step scheduled
static long long g_steps = 0;

// One micro-batch of the model: every operand has the extent of its shape and sits in a buffer of the plan that holds it; what a step
// reads, an earlier step wrote and none since has touched; no step but the zero border writes over its own input; the image comes in
// at the first step and leaves at the last.  (tests/test_schedule_cpu.py asserts the same of mz_debug_schedule.)
static void check_schedule(const Config& cfg, int dtype, const Knobs& k, int B, int H, int W, bool want_qa) {
    const int nhead = cfg.ratio == 2 ? 1 : cfg.ratio == 4 ? 2 : 3;
    const ModelDims dims = {dtype, {cfg.ch[0], cfg.ch[1], cfg.ch[2], cfg.ch[3]}, cfg.hidden_ratio, nhead, cfg.features};
    Model<LayerPlan> m;
    plan_model(m, dims, cfg.layers);
    Plan p;
    const int nb = default_micro_batch(dims, B, H, W, 0);
    EXPECT(nb >= 1 && nb <= B);
    make_plan(dims, nb, H, W, p);
    const auto bufs = check_plan(dims, p);
    const auto steps = make_schedule(m, dims, p, k, want_qa, cfg.ratio, 1);
    const size_t sz = dtype_size(dtype);
    auto bytes = [&](long long hh, long long ww, int c) { return (size_t)nb * hh * ww * pad16(c) * sz; };
    std::vector<std::pair<size_t, size_t>> live;  // {begin, end} of the tensors in the workspace
    auto overlaps = [](const BufRef& a, const BufRef& b) {
        return a.where == BUF_WS && b.where == BUF_WS && a.off < b.off + b.bytes && b.off < a.off + a.bytes;
    };
    for (size_t i = 0; i < steps.size(); ++i) {
        const Step<LayerPlan>& s = steps[i];
        const bool conv3 = s.kind == ST_CONV3, d2s = s.role == ROLE_D2S || s.kind == ST_ZERO_BORDER, head = s.role == ROLE_HEAD;
        ++g_steps;
        // extents
        const size_t image = (size_t)nb * 3 * H * W * sz;
        EXPECT(s.B == nb && s.cin > 0 && s.cout > 0);
        if (s.kind == ST_STEM) EXPECT(i == 0 && s.in.where == BUF_IMAGE_IN && s.in.bytes == image && s.cin == 3);
        else if (s.kind == ST_ZERO_BORDER) EXPECT(s.in.where == BUF_WS && s.in.off == s.out.off && s.in.bytes == s.out.bytes);
        else EXPECT(s.in.where == BUF_WS && s.in.bytes == bytes(s.H, s.W, s.kind == ST_MIX || s.kind == ST_QA_REDUCE ? s.cout : s.cin));
        if (s.kind == ST_MIX || s.fused) EXPECT(s.in1.where == BUF_WS && s.in1.bytes == bytes(s.H, s.W, s.cout));
        else if (head) EXPECT(s.in1.where == BUF_IMAGE_IN && s.in1.bytes == image && s.Hout == cfg.ratio * H && s.Wout == cfg.ratio * W);
        else EXPECT(s.in1.where == BUF_NONE);
        if (head) EXPECT(i + 1 == steps.size() && s.out.where == BUF_IMAGE_OUT && s.out.bytes == (size_t)nb * 3 * s.Hout * s.Wout * sz);
        else if (s.kind == ST_QA_REDUCE) EXPECT(s.out.where == BUF_QA_OUT && s.out.bytes == (size_t)nb * s.cout * 4);
        else if (d2s) EXPECT(s.out.where == BUF_WS && s.out.bytes == (size_t)nb * s.Hout * s.Wout * s.layer->cq_p * sz && s.Hout >= 2 * s.H && s.Wout >= 2 * s.W);
        else if (s.kind == ST_CRUSH) EXPECT(s.out.where == BUF_WS && s.out.bytes == bytes(s.Hout, s.Wout, s.cout) && s.Hout == s.H / 2 && s.Wout == s.W / 2);
        else EXPECT(s.out.where == BUF_WS && s.out.bytes == bytes(s.H, s.W, s.cout));
        // each workspace operand inside one buffer of the plan
        for (const BufRef* b : {&s.in, &s.in1, &s.out}) {
            if (b->where != BUF_WS) continue;
            bool found = false;
            for (const auto& buf : bufs) found = found || (buf.first == b->off && b->bytes <= buf.second);
            EXPECT(found && b->off + b->bytes <= p.total);
        }
        // liveness
        for (const BufRef* b : {&s.in, &s.in1}) {
            if (b->where != BUF_WS) continue;
            bool found = false;
            for (const auto& t : live) found = found || (t.first == b->off && t.second == b->off + b->bytes);
            EXPECT(found);
        }
        if (s.kind != ST_ZERO_BORDER) EXPECT(!overlaps(s.out, s.in) && !overlaps(s.out, s.in1));
        if (s.out.where == BUF_WS) {
            const size_t b0 = s.out.off, b1 = s.out.off + s.out.bytes;
            for (size_t t = live.size(); t-- > 0;)
                if (live[t].first < b1 && b0 < live[t].second) live.erase(live.begin() + t);
            live.push_back({b0, b1});
        }
        // the layer, for the sweep below
        static const int role_op[] = {-1, 0, 6, 4, 2, 3};
        if (conv3) g_layers.insert({dtype, role_op[s.role], s.cin, s.cout});
        if (s.kind == ST_MIX) g_layers.insert({dtype, 7, s.cin, s.cout});
        // with MZ_NO_FUSE=1 no block fuses; otherwise those of at most 96 channels do
        if (s.role == ROLE_CONV2) EXPECT(s.fused == (k.fuse && s.cout <= 96));
    }
    EXPECT(!steps.empty() && steps.back().role == ROLE_HEAD);
}

int main() {
    Knobs other;  // row-major tile walk, eight persistent workgroups
    other.blk4 = 0; other.persist = 8;
    Knobs nofuse;  // MZ_NO_FUSE=1
    nofuse.fuse = false;
    const Knobs knobs[] = {Knobs(), other};
    // the schedules: the fixture configurations at the sizes of tests/test_schedule_cpu.py, bench.py's models up to 4320 x 7680
    for (int dtype = 0; dtype < 3; ++dtype)
        for (const Knobs& k : {Knobs(), nofuse})
            for (bool want_qa : {false, true}) {
                for (const Config& cfg : kFixtures)
                    for (const auto& s : {std::array<int, 2>{8, 8}, {37, 45}, {64, 120}}) check_schedule(cfg, dtype, k, 2, s[0], s[1], want_qa);
                for (const Config& cfg : kBench)
                    for (const auto& s : kShapes)
                        for (int B : kBatches)
                            if (s[0] >= 8 && s[1] >= 8) check_schedule(cfg, dtype, k, B, s[0], s[1], want_qa);
            }
    for (const auto& l : kExtraLayers) EXPECT(g_layers.insert({l[0], l[1], l[2], l[3]}).second);  // (a layer the schedules have is no extra)
    for (const Knobs& k : knobs)
        for (int cus : kCus) {
            // the schedules' layers at every shape and batch
            for (const auto& l : g_layers)
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
    printf("%lld scheduled steps, %d layers, %lld layer calls, %lld tile lists\n", g_steps, (int)g_layers.size(), g_choices, g_lists);
    if (g_failed) return 1;
    printf("selection OK\n");
    return 0;
}
