// forward_lite.cpp -- the forward of MoeNet_lite2.Net (python/MoeNet_lite2.py:22-54: three LBs with FRM gates, two pointwise upsampler branches).
#include "net.h"

using namespace moe;

int moe::forward_lite(const moe_net& n, Fwd& f)
{
    const int B = f.B, h = f.h, w = f.w;
    const long long P = (long long)B * h * w;
    hipStream_t s = f.s;
    const FwdIO& io = f.io;
    Act A = f.act(P), Bb = f.act(P), Cc = f.act(P), Dd = f.act(P);
    const int nslab = (int)std::min<long long>(64, std::max<long long>(1, ((long long)h * w) / 256));
    // the pooled sums of conv_2's output come out of conv64_x3's epilogue, one slab per workgroup (fp16x3, the default of lite); in the
    // other modes a separate pass (pool_partial) forms nslab slabs per plane
    const int pslabs = f.groups;
    const bool poolfuse = n.opt.pool_fuse;
    float* partial = (float*)f.ar.take((size_t)B * std::max(nslab, pslabs) * 64 * 4);
    float* gate = (float*)f.ar.take((size_t)B * 64 * 4);
    // conv_input2's output is x times a fixed vector (see "stem.p2"): the stem writes it beside its own output, the 48 -> 48 1x1 conv is not launched (round 6)
    const bool stem2 = n.opt.stem2 && !n.debug && !f.direct && (int)n.scalars.at("stem_taps") == 1;
    if (stem2) f.stem(A, &Bb);
    else {
        f.stem(A);
        f.tap("stem", A, h, w, 64, 48);
        f.conv("input2", A, Bb, nullptr, h, w);
        f.tap("input2", Bb, h, w, 64, 48);
    }
    float* gate2 = (float*)f.ar.take((size_t)2 * B * 64 * 4);
    for (int k = 1; k <= 3; ++k) {
        const std::string key = "lb" + std::to_string(k);
        // round 6: conv_2 has no bias and no activation, so the mean the gate pools is linear in conv_2's INPUT: conv_1's epilogue forms the totals of its own output m,
        // frm_pre visits m's border, applies conv_2's weights to the nine shifted-window sums and the gate's two layers; conv_2 then stores gate * conv + x itself
        // (FrmPreArgs in common.h).  frm_apply's pass over six tensors (2.7 ms of a 1080p frame, at 6 TB/s) is gone.
        if (n.opt.frm_pre && poolfuse && f.x3 && !f.use_q8() && !n.debug && !f.direct) {      // (f.x3: every activation has its low part)
            if (!f.dry()) (void)hipMemsetAsync(partial, 0, (size_t)B * pslabs * 64 * 4, s);      // (workgroups without a patch in a plane leave their slab untouched)
            ConvExtra c1;
            c1.pool = true; c1.pool_out = partial; c1.pool_slabs = pslabs; c1.pool_act = true;
            if (f.conv(key + ".c1", Bb, Cc, nullptr, h, w, c1).pooled) {
                if (!f.dry()) {
                    FrmPreArgs a{};
                    a.m = Cc.hi; a.m_lo = Cc.lo; a.partial = partial; a.nslab = pslabs; a.c2t = f.small<float>(key + ".c2t");
                    a.w0 = f.small<float>(key + ".w0"); a.b0 = f.small<float>(key + ".b0"); a.w2 = f.small<float>(key + ".w2"); a.b2 = f.small<float>(key + ".b2");
                    a.gate = gate2; a.B = B; a.H = h; a.W = w;
                    launch_frm_pre(a, s);
                }
                ConvExtra c2;
                c2.gate = true; c2.gate_in = gate2;
                if (!f.conv(key + ".c2", Cc, Dd, &Bb, h, w, c2).gated) return fail(MOE_EINVAL, "internal error: layer %s: the gated form of conv64_x3 refused a shape its pooled form took", key.c_str());
                std::swap(Bb, Dd);
                f.tap(key, Bb, h, w, 64, 48);
                continue;
            }
            // (conv_1 ran without the pooled epilogue: the shape is outside pooled_groups_ok -- the form below, from conv_2 on)
        } else
            f.conv(key + ".c1", Bb, Cc, nullptr, h, w);
        ConvExtra c2;
        if (poolfuse && f.x3) {
            if (!f.dry()) (void)hipMemsetAsync(partial, 0, (size_t)B * pslabs * 64 * 4, s);      // (workgroups without a patch in a plane leave their slab untouched)
            c2.pool = true; c2.pool_out = partial; c2.pool_slabs = pslabs;
        }
        const bool pooled = f.conv(key + ".c2", Cc, Dd, nullptr, h, w, c2).pooled;
        if (!f.dry()) {
            if (!pooled) launch_pool_partial(Dd.hi, Dd.lo, partial, B, (long long)h * w, 64, nslab, s);
            FrmArgs a{};
            a.partial = partial; a.nslab = pooled ? pslabs : nslab; a.HW = (long long)h * w;
            a.w0 = f.small<float>(key + ".w0"); a.b0 = f.small<float>(key + ".b0");
            a.w2 = f.small<float>(key + ".w2"); a.b2 = f.small<float>(key + ".b2");
            a.t = Dd.hi; a.x = Bb.hi; a.out = Bb.hi; a.t_lo = Dd.lo; a.x_lo = Bb.lo; a.out_lo = Bb.lo;
            a.gate = gate; a.B = B;
            launch_frm(a, s);
        }
        f.tap(key, Bb, h, w, 64, 48);
    }
    Act fin[2];
    int H = h, W = w;
    // The last upsampler stage and the 48->1 tail conv run as one kernel (the 64-channel HR tensor, 128 B per HR pixel written
    // and read back per branch, never exists): the conv's epilogue dots its fp32 activations with the tail weights.
    const bool fuse1 = n.opt.fuse_tail && !f.direct && !n.debug && n.stages >= 1;
    float* part[2] = {nullptr, nullptr};
    const auto up_key = [](int br, int st) { return std::string(br == 0 ? "ures" : "uim") + ".up" + std::to_string(st); };
    // the last TWO stages and the tail in one launch (conv1x1_f2.hip): every layer of the upsampler is pointwise -- the tensor between the stages never exists
    const auto two_stages = [&](int br, int st, int H, int W) {
        if (!(fuse1 && f.x3 && n.opt.up_fuse2 && n.opt.conv1x1 && n.opt.k48 && n.opt.conv_impl == 2 && n.stages >= 2 && st == n.stages - 2)) return false;
        const ConvLayer& LA = n.convs[n.conv_index.at(up_key(br, st))];
        const ConvLayer& LB = n.convs[n.conv_index.at(up_key(br, st + 1))];
        return LA.taps == 1 && LB.taps == 1 && LA.cin <= 48 && LB.cin <= 48 && LA.r == 2 && LB.r == 2 && LA.nchunks == 4 && LB.nchunks == 4 && LA.w_lo && LB.w_lo &&
               LA.scale == 1.f && LB.scale == 1.f && conv1x1_f2_applicable(B, H, W, LA.slope, LB.slope, f.groups);
    };
    ConvExtra last;      // what the last stage is asked for under fuse1 (the pointers follow per branch)
    last.fuse_tail1 = true;
    // partial planes per branch the fused 1x1 tail of branch br writes: 1 (complete dot products: conv1x1_f2.hip, conv1x1.hip) or 2 (conv_mfma_kernel's channel halves)
    const auto tail_parts = [&](int br) {
        Act in; in.has_lo = f.x3;      // (the form of every activation here: f.act's)
        int H = h, W = w;
        for (int st = 0; st + 1 < n.stages; ++st, H *= 2, W *= 2) if (two_stages(br, st, H, W)) return 1;
        return f.route(up_key(br, n.stages - 1), in, Act{}, nullptr, H, W, last).done.tail1_parts;
    };
    const int nparts = fuse1 ? tail_parts(0) : 0;
    // fp16 input and the table of this checkpoint's U branch at hand (moe_net::lut): the U branch is not run, the final sum looks its value up (the table holds
    // complete dot products: a launch set whose R tail comes out in the two-part form computes the U branch as well).  The planning pass has no input: it plans the branch.
    const bool use_lut = !f.ctx.lut_capture && fuse1 && io.x_dtype == MOE_F16 && n.lut_state == 1 && n.lut && n.opt.lite_lut && nparts == 1;
    if (fuse1 && !use_lut && tail_parts(1) != nparts) return fail(MOE_EINVAL, "internal error: lite's two branches routed their fused tails to different forms");
    f.skips_planned_work = use_lut;
    for (int br = 0; br < (use_lut ? 1 : 2); ++br) {
        Act cur = br == 0 ? Bb : A;
        H = h; W = w;
        for (int st = 0; st < n.stages; ++st) {
            const std::string ckey = up_key(br, st);
            if (two_stages(br, st, H, W)) {
                const ConvLayer& LA = n.convs[n.conv_index.at(ckey)];
                const ConvLayer& LB = n.convs[n.conv_index.at(up_key(br, st + 1))];
                part[br] = (float*)f.ar.take((size_t)2 * B * H * 4 * W * 4 * 4);
                if (!f.dry()) {
                    Conv1x1F2Args q{};
                    q.in_hi = cur.hi; q.in_lo = cur.lo;
                    q.wa_hi = f.blob<half_t>(LA.w_hi); q.wa_lo = f.blob<half_t>(LA.w_lo); q.wb_hi = f.blob<half_t>(LB.w_hi); q.wb_lo = f.blob<half_t>(LB.w_lo);
                    q.bias_a = LA.has_bias ? f.blob<float>(LA.bias) : f.small<float>("zero_bias"); q.bias_b = LB.has_bias ? f.blob<float>(LB.bias) : f.small<float>("zero_bias");
                    q.tail_w = f.small<float>(br == 0 ? "tail_r.f32" : "tail_u.f32"); q.tail_out = part[br];
                    q.slope_a = LA.slope; q.slope_b = LB.slope; q.B = B; q.H = H; q.W = W;
                    const int rec = f.prof_begin(ckey, 3.0 * 2.0 * (double)B * H * W * (LA.cout * LA.cin + 4.0 * LB.cout * LB.cin));
                    const bool ok = launch_conv1x1_f2(q, f.groups, s);
                    f.prof_end(rec);
                    if (!ok) return fail(MOE_EINVAL, "internal error: fused upsampler stages (conv1x1_f2) rejected layer %s", ckey.c_str());
                }
                H *= 4; W *= 4;
                break;
            }
            if (fuse1 && st == n.stages - 1) {
                part[br] = (float*)f.ar.take((size_t)2 * B * H * 2 * W * 2 * 4);
                if (!f.dry()) { last.tail1_w = f.small<float>(br == 0 ? "tail_r.f32" : "tail_u.f32"); last.tail1_out = part[br]; }
                f.conv(ckey, cur, Act{}, nullptr, H, W, last);
                H *= 2; W *= 2;
                continue;
            }
            Act nxt = f.act((long long)B * H * 2 * W * 2);
            f.conv(ckey, cur, nxt, nullptr, H, W);
            H *= 2; W *= 2;
            f.tap(std::string(br == 0 ? "r" : "u") + ".up" + std::to_string(st), nxt, H, W, 64, 48);
            cur = nxt;
        }
        fin[br] = cur;
    }
    if (fuse1) {
        if (!f.dry()) {
            if (f.ctx.lut_capture) {      // (B = 1, the 256 x 256 image of all patterns: part[1] IS the table)
                if (nparts != 1 || !part[1]) return MOE_EINVAL;
                HIP_TRY(hipMemcpyAsync(f.ctx.lut_capture, part[1], (size_t)H * W * 4, hipMemcpyDeviceToDevice, s));
                return MOE_OK;
            }
            Tail1SumArgs t{};
            t.p0 = part[0]; t.p1 = use_lut ? nullptr : part[1]; t.nparts = nparts; t.y = io.y; t.y_dtype = io.y_dtype; t.y_off = io.y_off; t.B = B; t.H = H; t.W = W;
            if (use_lut) { t.lut = n.lut; t.r = n.scale; t.x = io.x; t.x_off = io.x_off; t.sB = io.sB; t.sH = io.sH; t.sW = io.sW; t.vec_ok = f.y_vec; }
            launch_tail1sum(t, s);
        }
        return MOE_OK;
    }
    if (f.ctx.lut_capture) return MOE_EINVAL;      // (no fused tail: no table -- build_lite_lut marks it unavailable)
    f.tail(&fin[0], &fin[1], H, W, false);
    return MOE_OK;
}
