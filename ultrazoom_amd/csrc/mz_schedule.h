// The forward pass of a planned model as data: the steps of one micro-batch in launch order, each with its layer, its shapes and its
// operands as buffer references.  forward_micro (mz_host.cpp) runs it, mz_flops_per_image and mz_debug_schedule (mz_debug.cpp) read it.
// Like mz_plan.h and mz_select.h this calls nothing in HIP and touches no error state: tests/select_main.cpp builds schedules under the
// sanitizers, tests/test_schedule_cpu.py checks through mz_debug_schedule that no step reads what an earlier one has not left there.
//
// The schedule follows the reference's MewZoom.forward (src/ultrazoom/model.py:149-164) and its sub-modules; each part cites the lines
// it replaces.
#pragma once
#include "mz_select.h"

namespace mz {

enum StepKind { ST_STEM, ST_CONV3, ST_MIX, ST_CRUSH, ST_ZERO_BORDER, ST_QA_REDUCE };
// which role function (mz_select.h) makes the Conv3Call of an ST_CONV3 step
enum StepRole { ROLE_NONE, ROLE_CONV1, ROLE_CONV2, ROLE_PLAIN, ROLE_D2S, ROLE_HEAD };

// An operand: `bytes` bytes at offset `off` of the workspace, or one of the three tensors the caller names (off = 0; bytes: of a dense
// tensor in the model's dtype -- mz_forward_u8 and mz_forward_view lay the images out otherwise).  Never a pointer: a schedule is built
// without a workspace.
enum BufWhere { BUF_WS = 0, BUF_NONE = -1, BUF_IMAGE_IN = -2, BUF_IMAGE_OUT = -3, BUF_QA_OUT = -4 };  // negative: mz_debug_step::off reports them
struct BufRef {
    int where = BUF_NONE;
    size_t off = 0, bytes = 0;
};

template <class Layer> struct Step {
    int kind = ST_CONV3, role = ROLE_NONE;
    const Layer* layer = nullptr;         // the layer that runs (ST_ZERO_BORDER: the sub-pixel conv before it; ST_STEM: none)
    const Block<Layer>* block = nullptr;  // ROLE_CONV2: its block
    bool fused = false;                   // ROLE_CONV2: the mix runs in its epilogue
    float alpha = 0.f;                    // ST_MIX
    int cin = 0, cout = 0;
    int B = 0, H = 0, W = 0;              // input pixels
    int Hout = 0, Wout = 0;               // ROLE_D2S, ROLE_HEAD, ST_ZERO_BORDER, ST_CRUSH: output pixels; else 0
    int R = 0, clamp = 0;                 // ROLE_HEAD: the total upscale ratio, clamp to [0, 1]
    BufRef in, in1, out;                  // in1: the block input of a fused conv2, z of a mix, the low-resolution image of the head
};

// multiply-accumulates of a step (convolutions only)
template <class Layer> long long step_macs(const Step<Layer>& s) {
    const long long px = (long long)s.B * s.H * s.W, cc = (long long)s.cin * s.cout;
    switch (s.kind) {
        case ST_STEM: case ST_MIX: return px * cc;
        case ST_CONV3: return px * cc * 9 + (s.fused ? px * 2 * s.cout * s.cout : 0);
        case ST_CRUSH: return (long long)s.B * s.Hout * s.Wout * cc * 4;
        default: return 0;
    }
}

// The Conv3Call of an ST_CONV3 step on its resolved operands; an image head's views are the caller's to add
template <class Layer> Conv3Call step_call(const Knobs& k, const Step<Layer>& s, const void* in, const void* in1, void* out) {
    Conv3Call c;
    switch (s.role) {
        case ROLE_CONV1: return conv1_call(*s.layer, in, out, s.B, s.H, s.W);
        case ROLE_CONV2: c = conv2_call(k, *s.block, in, in1, s.B, s.H, s.W); c.out = out; return c;
        case ROLE_D2S: return d2s_call(*s.layer, in, out, s.B, s.H, s.W, s.Hout, s.Wout);
        case ROLE_HEAD: c = head_call(*s.layer, in, out, s.B, s.H, s.W); c.img = in1; c.R = s.R; c.clamp = s.clamp; return c;
        default: return plain_call(*s.layer, in, out, s.B, s.H, s.W);
    }
}

// The steps of one micro-batch of p.nb images of p.hs[0] x p.ws[0] pixels, in launch order.  R: the model's upscale ratio.
template <class Layer>
std::vector<Step<Layer>> make_schedule(const Model<Layer>& m, const ModelDims& dims, const Plan& p, const Knobs& knobs, bool want_qa, int R, int clamp) {
    std::vector<Step<Layer>> steps;
    const size_t sz = dtype_size(dims.dtype);
    const int nb = p.nb, H = p.hs[0], W = p.ws[0];
    // c channels per pixel of nb x hh x ww pixels, at a workspace offset
    auto act = [&](size_t off, long long hh, long long ww, int c) { return BufRef{BUF_WS, off, (size_t)nb * hh * ww * pad16(c) * sz}; };
    auto step = [&](int kind, int role, const Layer* c, int hh, int ww, const BufRef& in, const BufRef& in1, const BufRef& out) -> Step<Layer>& {
        Step<Layer> s;
        s.kind = kind; s.role = role; s.layer = c;
        if (c) { s.cin = c->cin; s.cout = c->cout; }
        s.B = nb; s.H = hh; s.W = ww;
        s.in = in; s.in1 = in1; s.out = out;
        steps.push_back(s);
        return steps.back();
    };
    // EncoderBlock / DecoderBlock (model.py:507-511): conv1 -> SiLU -> conv2 -> adaptive mix with the input
    auto block = [&](const Block<Layer>& b, const BufRef& xin, size_t hid_off, size_t z_off, size_t y_off, int hh, int ww) {
        const BufRef hid = act(hid_off, hh, ww, b.conv1.cout), y = act(y_off, hh, ww, b.conv2.cout);
        step(ST_CONV3, ROLE_CONV1, &b.conv1, hh, ww, xin, {}, hid);
        // conv2 + AdaptiveResidualMix in one launch (all output channels live in one workgroup), or in two
        const bool fused = conv2_call(knobs, b, nullptr, nullptr, nb, hh, ww).mixf != nullptr;
        const BufRef z = act(z_off, hh, ww, b.conv2.cout);
        Step<Layer>& c2 = step(ST_CONV3, ROLE_CONV2, &b.conv2, hh, ww, hid, fused ? xin : BufRef{}, fused ? y : z);
        c2.block = &b; c2.fused = fused;
        if (!fused) step(ST_MIX, ROLE_NONE, &b.mix, hh, ww, xin, z, y).alpha = b.alpha;
        return y;
    };

    // stem (model.py:158): NCHW image -> NHWC features
    const BufRef image = {BUF_IMAGE_IN, 0, (size_t)nb * 3 * H * W * sz};
    BufRef cur = act(p.R[0][0], H, W, dims.ch[0]);
    Step<Layer>& stem = step(ST_STEM, ROLE_NONE, nullptr, H, W, image, {}, cur);
    stem.cin = 3; stem.cout = dims.ch[0];

    // encoder (model.py:461-484)
    BufRef feat[4];
    int feat_slot[4];
    for (int l = 0; l < 4; ++l) {
        int slot = 0;
        if (l > 0) {  // PixelCrush (model.py:857-863, 881-882)
            cur = act(p.R[l][0], p.hs[l], p.ws[l], dims.ch[l]);
            Step<Layer>& s = step(ST_CRUSH, ROLE_NONE, &m.crush[l - 1], p.hs[l - 1], p.ws[l - 1], feat[l - 1], {}, cur);
            s.Hout = p.hs[l]; s.Wout = p.ws[l];
        }
        for (auto& b : m.enc_blocks[l]) {
            cur = block(b, cur, p.HID[l], p.Z[l], p.R[l][slot ^ 1], p.hs[l], p.ws[l]);
            slot ^= 1;
        }
        feat[l] = cur;
        feat_slot[l] = slot;
    }

    // quality head (model.py:482, 1026-1032); upscale() discards it (model.py:175)
    if (want_qa) {
        const int F = dims.num_deg_features;
        const BufRef qa = act(p.QA, p.hs[3], p.ws[3], F);
        step(ST_CONV3, ROLE_PLAIN, &m.qa_conv, p.hs[3], p.ws[3], feat[3], {}, qa);
        step(ST_QA_REDUCE, ROLE_NONE, &m.qa_conv, p.hs[3], p.ws[3], qa, {}, {BUF_QA_OUT, 0, (size_t)nb * F * sizeof(float)});
    }

    // decoder (model.py:691-724)
    cur = feat[3];
    int slot = feat_slot[3];
    for (int d = 0; d < 4; ++d) {
        const int l = 3 - d;
        if (d > 0) {
            // SubpixelConv2d (model.py:926-930) + crop_feature_maps zero pad (model.py:650-689) + skip mix (:701)
            const Layer& up = m.up[d - 1];
            const BufRef u = act(p.U[l], p.hs[l], p.ws[l], up.cq);
            Step<Layer>& d2s = step(ST_CONV3, ROLE_D2S, &up, p.hs[l + 1], p.ws[l + 1], cur, {}, u);
            d2s.Hout = p.hs[l]; d2s.Wout = p.ws[l];
            // the border that 2 hs[l + 1] x 2 ws[l + 1] pixels leave of u, zeroed in place
            Step<Layer>& border = step(ST_ZERO_BORDER, ROLE_NONE, &up, p.hs[l + 1], p.ws[l + 1], u, {}, u);
            border.Hout = p.hs[l]; border.Wout = p.ws[l];
            // pick a level-l buffer that is not the saved encoder feature
            slot = (feat_slot[l] + 1) % 3;
            const BufRef dst = act(p.R[l][slot], p.hs[l], p.ws[l], dims.ch[l]);
            step(ST_MIX, ROLE_NONE, &m.skipmix[d - 1], p.hs[l], p.ws[l], feat[l], u, dst).alpha = m.skip_alpha[d - 1];
            cur = dst;
        }
        for (auto& b : m.dec_blocks[d]) {
            int nslot = (slot + 1) % 3;
            if (d > 0 && nslot == feat_slot[l]) nslot = (nslot + 1) % 3;  // (the encoder feature is dead after the skip mix, but keep it simple)
            cur = block(b, cur, p.HID[l], p.Z[l], p.R[l][nslot], p.hs[l], p.ws[l]);
            slot = nslot;
        }
    }

    // head (model.py:968-972, 997-1001) + bicubic skip + residual add + clamp (model.py:156,162,177)
    int hh = H, ww = W;
    for (int i = 0; i < dims.nhead; ++i) {
        const BufRef y = i == 0 ? block(m.head_blocks[i], cur, p.HID[0], p.Z[0], p.R[0][(slot + 1) % 3], hh, ww)
                                : block(m.head_blocks[i], cur, p.HHID[i], p.HZ[i], p.HR[i][1], hh, ww);
        if (i == dims.nhead - 1) {
            Step<Layer>& s = step(ST_CONV3, ROLE_HEAD, &m.head_up[i], hh, ww, y, image, {BUF_IMAGE_OUT, 0, (size_t)nb * 3 * (2 * hh) * (2 * ww) * sz});
            s.Hout = 2 * hh; s.Wout = 2 * ww; s.R = R; s.clamp = clamp;
        } else {
            cur = act(p.HR[i + 1][0], 2LL * hh, 2LL * ww, dims.ch[0]);
            Step<Layer>& s = step(ST_CONV3, ROLE_D2S, &m.head_up[i], hh, ww, y, {}, cur);
            s.Hout = 2 * hh; s.Wout = 2 * ww;
            hh *= 2; ww *= 2;
        }
    }
    return steps;
}

}  // namespace mz
