// Introspection entries of libmewzoom_hip.so -- the error and last-kernel state every host unit writes (mz_err.h), the per-device CU
// count, and the host-only (no GPU) views of planning, selection and packing that the CPU tests read.
#include <cstdarg>
#include <cstdio>

#include "mz_host.h"
#include "mz_pack.h"

using namespace mz;

static thread_local char g_err[512] = "";
thread_local const char* mz::g_last_kernel = "";
int mz::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* mz_last_error(void) { return g_err; }
extern "C" const char* mz_debug_last_kernel(void) { return g_last_kernel; }

int mz::device_cus() {
    static int known[kMaxDevices];  // 0 unknown, else the CU count + 1
    int n = 0, dev = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(MZ_ERR_NO_DEVICE, "no HIP device visible");
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return fail(MZ_ERR_NO_DEVICE, "bad current device");
    if (!known[dev]) {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c = 0;
        known[dev] = c / 8 * 8 + 1;
    }
    return known[dev] - 1;
}

extern "C" int mz_debug_read(unsigned long long* host_dst) {
    unsigned long long* b = debug_buffer();
    if (!b) return -1;
    return hipMemcpy(host_dst, b, 16 * 64 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -6;
}

// Host-only (no GPU): the tile list Runner::tile_table() uploads for a launch of B images of tiles_y x tiles_x tiles of th x tw pixels,
// ntiles N tiles, walked in groups of gm x gn (blk4: block rows of four tile rows).  Writes at most cap entries of two words to out
// and returns the number of tiles listed (tests/test_cabi_cpu.py checks that every tile appears exactly once).
extern "C" int mz_debug_tile_list(int B, int tiles_y, int tiles_x, int ntiles, int gm, int gn, int blk4, int th, int tw, unsigned int* out, int cap) {
    if (B < 1 || tiles_x < 1 || tiles_y < 1 || ntiles < 1 || gm < 1 || gn < 1 || th < 1 || tw < 1 || !out || cap < 0) return MZ_ERR_INVALID_ARGUMENT;
    const int mtiles = B * tiles_x * tiles_y;
    std::vector<uint32_t> t;
    tile_list(group_walk(tiles_x, tiles_y, mtiles, ntiles, std::min(gm, mtiles), std::min(gn, ntiles), blk4 ? 1 : 0), th, tw, t);
    const int n = (int)(t.size() / 2);
    for (int i = 0; i < n && i < cap; ++i) { out[2 * i] = t[2 * i]; out[2 * i + 1] = t[2 * i + 1]; }
    return n;
}

// what an entry that returns no code refuses: the message for mz_last_error(), and the entry's own "nothing"
template <class T> static T refused(T nothing, const Refusal& r) { fail(r); return nothing; }

// Host-only (no GPU): the kernel family Runner::conv3 / Runner::mix would launch for one layer -- the same role functions make the call,
// the same choose_* choose -- with the knobs read from the environment as the mz_op_* entries read them.
extern "C" const char* mz_debug_select(int dtype, int op, int cin, int cout, int B, int H, int W, int cus) {
    const char* const none = nullptr;
    if ((dtype != MZ_F32 && dtype != MZ_BF16 && dtype != MZ_F16) || cin < 1 || cout < 1 || B < 1 || H < 1 || W < 1 || cus < 0)
        return refused(none, refuse(MZ_ERR_INVALID_ARGUMENT, "bad arguments"));
    if (op == 5 && dtype != DT_BF16 && dtype != DT_F16)
        return refused(none, refuse(MZ_ERR_INVALID_ARGUMENT, "the FiLM epilogue is implemented for bf16 / fp16"));
    if (op == 8) return refused(none, refuse(MZ_ERR_INVALID_ARGUMENT, "bad op %d", op));  // the gate is no launch of its own
    const Knobs k = read_knobs();
    BlockPlan b;
    Refusal why;
    const LayerPlan* c = plan_debug_layer(b, dtype, op, cin, cout, &why);
    if (!c) return refused(none, why);
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
    const KernelChoice ch = choose_conv3(k, dtype, call, cus);
    return ch.ok ? kernel_name(ch) : refused(none, refuse(MZ_ERR_INVALID_ARGUMENT, "%s", ch.why));
}

// Host-only (no GPU): packing `layout` of one layer (mz_debug_select's ops; 8 = the fused gate of a block's conv2), as pack_kernel writes
// it: the OIHW source index of each packed element, -1 for padding.  Writes at most cap of them to out.
extern "C" long long mz_debug_pack(int dtype, int op, int cin, int cout, int layout, long long* out, long long cap) {
    if ((dtype != MZ_F32 && dtype != MZ_BF16 && dtype != MZ_F16) || cin < 1 || cout < 1 || layout < 0 || layout >= PK_COUNT || cap < 0 ||
        (cap > 0 && !out))
        return refused(-1LL, refuse(MZ_ERR_INVALID_ARGUMENT, "bad arguments"));
    BlockPlan b;
    Refusal why;
    const LayerPlan* c = plan_debug_layer(b, dtype, op, cin, cout, &why);
    if (!c) return refused(-1LL, why);
    if (!c->has(layout)) return refused(-1LL, refuse(MZ_ERR_INVALID_ARGUMENT, "the layer has no packing %d", layout));
    const PackArgs p = pack_args(*c, layout, dtype, nullptr, nullptr);
    const long long n = (long long)(packed_bytes(p.taps, p.frags, p.ntiles, p.nchunks) / dtype_size(dtype));
    for (long long i = 0; i < n && i < cap; ++i) out[i] = dtype == DT_F32 ? pack_source<4>(p, i) : pack_source<2>(p, i);
    return n;
}
extern "C" const char* mz_version(void) { return "mewzoom_hip 0.1 (gfx950)"; }

extern "C" double mz_flops_per_image(const mz_handle* h, int H, int W) {
    if (!h) return 0.0;
    Plan p;
    make_plan(h->dims, 1, H, W, p);
    long long macs = 0;
    for (const auto& st : make_schedule(h->model, h->dims, p, h->ctx.knobs, /*want_qa*/ true, h->cfg.upscale_ratio, 0)) macs += step_macs(st);
    return 2.0 * (double)macs;
}

// Host-only (no GPU, no weights): the steps of one micro-batch of B images of H x W pixels under the handle's own knobs, and the kernel a
// device of `cus` compute units runs each 3x3 convolution and mix on.  Writes at most cap steps to out, returns their number.
extern "C" int mz_debug_schedule(const mz_handle* h, int B, int H, int W, int want_qa, int cus, mz_debug_step* out, int cap) {
    if (!h || cap < 0 || (cap > 0 && !out) || cus < 0) return fail(MZ_ERR_INVALID_ARGUMENT, "bad arguments");
    if (B <= 0 || H < 8 || W < 8) return fail(MZ_ERR_INVALID_ARGUMENT, "need B >= 1 and H, W >= 8 (got %d, %d, %d)", B, H, W);
    const Knobs& k = h->ctx.knobs;
    const int dtype = h->dims.dtype;
    Plan p;
    make_plan(h->dims, B, H, W, p);
    const auto steps = make_schedule(h->model, h->dims, p, k, want_qa != 0, h->cfg.upscale_ratio, 0);
    static const int role_op[] = {-1, 0, 6, 4, 2, 3};  // StepRole -> mz_debug_select's op
    for (size_t i = 0; i < steps.size() && i < (size_t)cap; ++i) {
        const Step<ConvW>& st = steps[i];
        mz_debug_step& d = out[i];
        d.kind = st.kind;
        d.op = st.kind == ST_MIX ? 7 : role_op[st.role];
        d.cin = st.cin; d.cout = st.cout;
        d.B = st.B; d.H = st.H; d.W = st.W; d.Hout = st.Hout; d.Wout = st.Wout;
        d.fused = st.fused;
        const BufRef* bufs[3] = {&st.in, &st.in1, &st.out};
        for (int j = 0; j < 3; ++j) {
            d.off[j] = bufs[j]->where == BUF_WS ? (long long)bufs[j]->off : bufs[j]->where;  // the external codes are negative
            d.bytes[j] = bufs[j]->bytes;
        }
        d.kernel = nullptr;
        if (st.kind == ST_MIX) d.kernel = kernel_name(choose_mix(k, dtype, *st.layer, st.B, st.H, st.W, cus));
        if (st.kind == ST_CONV3) d.kernel = kernel_name(choose_conv3(k, dtype, step_call(k, st, nullptr, nullptr, nullptr), cus));
    }
    return (int)steps.size();
}
