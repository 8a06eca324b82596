// forward_sedn.cpp -- the forward of SEDN (models.py:190-223: sixteen _Conv_Blocks with their squeeze-excite gates).
#include "net.h"

using namespace moe;

int moe::forward_sedn(const moe_net& n, Fwd& f)
{
    const int B = f.B, h = f.h, w = f.w;
    const long long P = (long long)B * h * w;
    hipStream_t s = f.s;
    Act A = f.act(P), Cc = f.act(P), Dd = f.act(P), T = f.act(P, 256);
    const int nslab = (int)std::min<long long>(64, std::max<long long>(1, ((long long)h * w) / 256));
    float* partial = (float*)f.ar.take((size_t)B * nslab * 256 * 4);
    const ConvLayer& Lt = n.convs[n.conv_index.at("b0.trans")];
    const size_t wel = (size_t)Lt.nchunks * Lt.nfrag() * 512;
    half_t* wplane = (half_t*)f.ar.take(f.direct ? (size_t)B * 64 * 256 * 4 : (size_t)B * wel * 2);
    half_t* wplane_lo = f.x3 ? (half_t*)f.ar.take((size_t)B * wel * 2) : nullptr;
    f.drop_taps();      // (the two forms leave different taps: none of another forward's stays behind to be read as this one's)
    f.stem(A);
    f.tap("stem", A, h, w, 64, 64);
    // fused block tail (see sedn_fuse in misc_kernels.hip): single-pass precision, fast kernel, planes fit the per-XCD split -- one 3x3 64->64 conv with per-plane
    // weights, LeakyReLU and the residual: on conv64_s.hip, or on conv3x3_sp<6>
    ConvForm tf;
    tf.B = B; tf.H = h; tf.W = w; tf.nchunks = B; tf.py = (h + kTileH - 1) / kTileH; tf.slope = 0.2f; tf.res = true; tf.plane_w = true;
    tf.G = (int)std::max<long long>(B, std::min<long long>(f.groups, (long long)B * ((w + kTileW - 1) / kTileW) * tf.py));   // total workgroups (plane b gets every B-th)
    const bool s64 = n.opt.s64 && conv64_s_applicable(tf);
    const bool sfuse = n.opt.sedn_fuse && !f.x3 && !f.direct && !n.debug && n.opt.conv_impl == 2 && B <= f.groups && (s64 || conv3x3_sp_applicable(tf));
    float* xpart = (float*)f.ar.take((size_t)B * nslab * 5 * 64 * 4);
    // the channel totals of rblock.2's output come out of that conv's epilogue (conv3x3_rw EPI 4), sedn_xsum then only visits the border
    const int pslabs = 2 * f.groups;
    float* xpool = (float*)f.ar.take((size_t)B * pslabs * 64 * 4);
    const bool spool = n.opt.pool_fuse;
    float* fgate = (float*)f.ar.take((size_t)B * 256 * 4);
    half_t* weff = (half_t*)f.ar.take((size_t)B * 72 * 512 * 2);
    for (int b = 0; b < 16; ++b) {
        const std::string k = "b" + std::to_string(b);
        f.conv(k + ".rb0", A, Cc, nullptr, h, w);
        f.tap(k + ".rb0", Cc, h, w, 64, 64);
        ConvExtra rb2;
        if (sfuse && spool) { rb2.pool = true; rb2.pool_out = xpool; rb2.pool_slabs = pslabs; }      // (the conv writes the first 2 min(G, py) slabs of every plane, all of them: no memset)
        const bool pooled = f.conv(k + ".rb2", Cc, Dd, nullptr, h, w, rb2).pooled;
        f.tap(k + ".rb2", Dd, h, w, 64, 64);
        if (sfuse) {
            if (!f.dry()) {
                SednFuseArgs fa{};
                fa.x = Dd.hi; fa.partial = xpart; fa.nslab = nslab; fa.B = B; fa.H = h; fa.W = w;
                if (pooled) {
                    const int py = (h + kTileH - 1) / kTileH;
                    fa.pooled = xpool; fa.pooled_slabs = pslabs;
                    fa.pooled_count = 2 * std::min(pooled_groups((long long)py, (long long)B * py, f.groups), py);      // conv3x3_rw EPI 4: slab 2 (g % py) + wave half
                }
                fa.w256t = f.small<float>(k + ".w256t"); fa.w256 = f.small<float>(k + ".w256"); fa.wt = f.small<float>(k + ".wt");
                fa.w_down = f.small<float>(k + ".down"); fa.w_up = f.small<float>(k + ".up");
                fa.gate = fgate; fa.weff = weff;
                launch_sedn_fuse(fa, s);
                f.tap_f32(k + ".mean", fgate, 256);              // (the fused branch runs with n.debug off: these are moe_net_set_debug's value 2)
                f.tap_raw16(k + ".weff", weff, 72 * 512);        // the A fragments as they lie in memory: the reader undoes pack_conv's order
                ConvArgs a{};
                a.in = Dd.hi; a.out = A.hi; a.res = A.hi; a.wpk = weff; a.plane_w = 1;
                a.bias = f.small<float>("zero_bias"); a.bias_img = f.small<float>("zero_bias_img");
                a.zero = f.small<half_t>("zero"); a.trash = f.small<half_t>("trash");
                a.B = B; a.H = h; a.W = w; a.in_cs = tf.in_cs; a.out_cs = tf.out_cs; a.r = tf.r; a.nchunks = tf.nchunks;
                a.px = (w + kTileW - 1) / kTileW; a.py = tf.py; a.G = tf.G;
                a.slope = tf.slope; a.scale = tf.scale;
                if (!(s64 ? launch_conv64_s(a, f.groups, s) : launch_conv3x3_sp(a, s))) return fail(MOE_EINVAL, "internal error: SEDN fused block tail: %s rejected the layer", s64 ? "conv64_s" : "conv3x3_sp");
                f.tap("block" + std::to_string(b), A, h, w, 64, 64);
            }
            continue;
        }
        f.conv(k + ".rb4", Dd, T, nullptr, h, w);
        f.tap(k + ".rb4", T, h, w, 256, 256);
        if (!f.dry()) {
            launch_pool_partial(T.hi, T.lo, partial, B, (long long)h * w, 256, nslab, s);
            const ConvLayer& L = n.convs[n.conv_index.at(k + ".trans")];
            SednSeArgs a{};
            a.partial = partial; a.nslab = nslab; a.HW = (long long)h * w;
            a.w_down = f.small<float>(k + ".down"); a.w_up = f.small<float>(k + ".up");
            a.B = B;
            if (f.direct) {
                // plain fp32 OIHW weights [64][256]: element i -> cin = i % 256; reuse the SE kernel with a
                // "fragment" view of 1 element per cin is not possible, so the debug path scales on the host-side layout:
                a.trans_pk32 = f.blob<float>(L.w_plain); a.nfrag = -(64 * 256);   // negative: plain layout marker
                a.trans_out = wplane;
            } else {
                a.trans_pk32 = f.blob<float>(L.w_pk32); a.nfrag = L.nfrag() * L.nchunks;
                a.trans_out = wplane; a.trans_out_lo = wplane_lo;
            }
            launch_sedn_se(a, s);
            if (!f.direct) f.tap_raw16(k + ".wtrans", wplane, (long long)wel);      // the per-plane trans weights in fragment order (fp16 parts)
        }
        ConvExtra trans;
        trans.plane_w = wplane; trans.plane_w_lo = wplane_lo;
        f.conv(k + ".trans", T, A, &A, h, w, trans);
        f.tap("block" + std::to_string(b), A, h, w, 64, 64);
    }
    f.tail(&A, nullptr, h, w, true);
    return MOE_OK;
}
