// weights.cpp -- the parameter schema of the four families, the packing of a state dict into the device blob, and the life of a net
// (create, set_param, finalize, destroy).
#include "net.h"

using namespace moe;

static void declare_params(moe_net& n)
{
    const int C = n.C;
    auto arsb = [&](const std::string& p) {
        n.add(p + "conv_1.weight", {C, C, 3, 3});
        n.add(p + "relu.weight", {1});
        n.add(p + "conv_2.weight", {C, C, 3, 3});
        n.add(p + "scale.scale", {1});
    };
    if (n.arch == MOE_ARCH_NET2X || n.arch == MOE_ARCH_NET3X || n.arch == MOE_ARCH_NET4X) {
        n.add("conv_input.weight", {64, 1, 3, 3});
        n.add("conv_input2.weight", {64, 64, 3, 3});
        n.add("relu.weight", {1});
        for (const char* br : {"u", "convt_R1"}) {
            for (int s = 0; s < n.stages; ++s) {
                const std::string p = std::string(br) + "." + std::to_string(s) + ".";
                n.add(p + "0.weight", {64 * n.r * n.r, 64, 3, 3});
                n.add(p + "0.bias", {64 * n.r * n.r});
                n.add(p + "2.weight", {1});
            }
            n.add(std::string(br) + "." + std::to_string(n.stages) + ".weight", {1, 64, 3, 3});
        }
        for (int i = 1; i <= 6; ++i) arsb("convt_F" + std::to_string(i) + ".0.");
    } else if (n.arch == MOE_ARCH_NETDN) {
        n.add("conv_input.weight", {48, 1, 3, 3});
        n.add("conv_input2.weight", {48, 48, 3, 3});
        n.add("relu.weight", {1});
        n.add("u.weight", {1, 48, 3, 3});
        n.add("convt_R1.weight", {1, 48, 3, 3});
        for (int i = 1; i <= 6; ++i) arsb("convt_F" + std::to_string(i) + ".0.");
    } else if (n.arch == MOE_ARCH_SEDN) {
        n.add("conv_input.weight", {64, 1, 3, 3});
        n.add("convt_R1.weight", {1, 64, 3, 3});
        for (int b = 0; b < 16; ++b) {
            const std::string p = "convt_F1." + std::to_string(b) + ".";
            n.add(p + "rblock.0.weight", {64, 64, 3, 3});
            n.add(p + "rblock.2.weight", {64, 64, 3, 3});
            n.add(p + "rblock.4.weight", {256, 64, 3, 3});
            n.add(p + "trans.0.weight", {64, 256, 1, 1});
            n.add(p + "conv_down.weight", {16, 256, 1, 1});
            n.add(p + "conv_up.weight", {256, 16, 1, 1});
        }
    } else {   // MOE_ARCH_LITE
        n.add("conv_input.weight", {48, 1, 1, 1});
        n.add("conv_input2.weight", {48, 48, 1, 1});
        n.add("relu.weight", {1});
        for (const char* br : {"ures", "uim"})
            for (int s = 0; s < n.stages; ++s) {
                const std::string p = std::string(br) + "." + std::to_string(s) + ".";
                n.add(p + "0.weight", {192, 48, 1, 1});
                n.add(p + "0.bias", {192});
                n.add(p + "2.weight", {1});
            }
        n.add("convt_R1.weight", {1, 48, 1, 1});
        n.add("convt_I1.weight", {1, 48, 1, 1});
        for (int k = 1; k <= 3; ++k) {
            const std::string p = "convt_F1" + std::to_string(k) + ".";
            n.add(p + "conv_1.weight", {48, 48, 3, 3});
            n.add(p + "conv_2.weight", {48, 48, 3, 3});
            n.add(p + "relu.weight", {1});
            n.add(p + "se.conv_du.0.weight", {3, 48, 1, 1});
            n.add(p + "se.conv_du.0.bias", {3});
            n.add(p + "se.conv_du.2.weight", {48, 3, 1, 1});
            n.add(p + "se.conv_du.2.bias", {48});
        }
    }
}

// =====================================================================================================
// weight packing
// =====================================================================================================
namespace {

struct BlobBuilder {
    std::vector<char> data;
    size_t take(size_t bytes)
    {
        const size_t a = (data.size() + 255) & ~(size_t)255;
        data.resize(a + bytes, 0);
        return a;
    }
    template <typename T> T* at(size_t off) { return (T*)(data.data() + off); }
};

// packed output channel n' = chunk*64 + cl  ->  original output channel, or -1 (padding).
// r > 1: chunk = sub-pixel (i*r + j), cl = channel c of the shuffled output: original = c*r*r + i*r + j
inline int orig_cout(int np, int cout, int r)
{
    const int chunk = np / 64, cl = np % 64;
    if (r > 1) {
        const int cs = cout / (r * r);
        return cl < cs ? cl * r * r + chunk : -1;
    }
    return np < cout ? np : -1;
}

// A-operand fragments of v_mfma_f32_32x32x16_f16 for D[cout][pixel]: fragment f = ((seg*taps + tap)*4 + ks)*2 + nblk,
// lane l holds W[cout = chunk*64 + nblk*32 + (l&31)][cin = seg*64 + ks*16 + 8*(l>>5) + e][tap], e = 0..7
void pack_conv(const Param& W, const Param* bias, int r, ConvLayer& L, BlobBuilder& bb, bool want_lo, bool want_plain, bool want_pk32,
               float fold = 1.f)   // ScaleLayer folded into the MFMA weights: conv(x, w) * s == conv(x, w * s), product formed in fp32
{
    const int cout = (int)W.shape[0], cin = (int)W.shape[1], k = (int)W.shape[2];
    L.cout = cout; L.cin = cin; L.k = k; L.r = r;
    L.taps = k * k;
    L.nseg = (cin + 63) / 64;
    L.nchunks = r > 1 ? r * r : (cout + 63) / 64;
    const int nfrag = L.nfrag();
    const size_t nel = (size_t)L.nchunks * nfrag * 512;
    L.w_hi = bb.take(nel * 2);
    if (want_lo) L.w_lo = bb.take(nel * 2);
    if (want_pk32) L.w_pk32 = bb.take(nel * 4);
    for (int chunk = 0; chunk < L.nchunks; ++chunk)
        for (int f = 0; f < nfrag; ++f) {
            const int nblk = f & 1, ks = (f >> 1) & 3, st = f >> 3;
            const int tap = st % L.taps, seg = st / L.taps;
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int np = chunk * 64 + nblk * 32 + (l & 31);
                    const int ci = seg * 64 + ks * 16 + 8 * (l >> 5) + e;
                    const int oc = orig_cout(np, cout, r);
                    float v = 0.f;
                    if (oc >= 0 && ci < cin) v = W.data[((size_t)oc * cin + ci) * L.taps + tap] * fold;
                    const size_t idx = ((size_t)(chunk * nfrag + f) * 64 + l) * 8 + e;
                    const half_t hv = (half_t)v;
                    bb.at<half_t>(L.w_hi)[idx] = hv;
                    if (want_lo) bb.at<half_t>(L.w_lo)[idx] = (half_t)((v - (float)hv) * 2048.f);
                    if (want_pk32) bb.at<float>(L.w_pk32)[idx] = v;
                }
        }
    if (want_lo && L.taps == 1 && L.nseg == 1) {
        // single-launch split precision (conv_mfma_kernel<1,3>): per chunk the 8 fragments of w_lo, then those of w_hi twice
        L.has_x3 = true;
        L.w_x3 = bb.take(nel * 2 * 3);
        const size_t per = (size_t)nfrag * 512;               // elements of one chunk
        for (int chunk = 0; chunk < L.nchunks; ++chunk)
            for (int seg3 = 0; seg3 < 3; ++seg3)
                memcpy(bb.at<half_t>(L.w_x3) + ((size_t)chunk * 3 + seg3) * per,
                       bb.at<half_t>(seg3 == 0 ? L.w_lo : L.w_hi) + (size_t)chunk * per, per * 2);
    }
    L.has_bias = bias != nullptr;
    L.bias_img = bb.take((size_t)L.nchunks * 256 * 4);        // zero-filled; the biases are written below
    if (bias) {
        L.bias = bb.take((size_t)L.nchunks * 64 * 4);
        for (int np = 0; np < L.nchunks * 64; ++np) {
            const int oc = orig_cout(np, cout, r);
            bb.at<float>(L.bias)[np] = oc >= 0 ? bias->data[oc] * fold : 0.f;
            bb.at<float>(L.bias_img)[(np / 64) * 256 + (np % 64)] = bb.at<float>(L.bias)[np];
        }
    }
    if (want_plain) {
        L.w_plain = bb.take(W.data.size() * 4);
        memcpy(bb.at<float>(L.w_plain), W.data.data(), W.data.size() * 4);
        if (bias) {
            L.bias_plain = bb.take(bias->data.size() * 4);
            memcpy(bb.at<float>(L.bias_plain), bias->data.data(), bias->data.size() * 4);
        }
    }
}

}  // namespace

// conv64_x3.hip's weight order (introduced by round 2's arsb_fused.hip, retired): [wave w][fragment f = tap * 2 + kh][lane l][e], lane l = (m = l & 15, kq = l >> 4) holds
// W[cout = 16w + m][cin = 8 * SL(kh, kq) + e][tap] with SL(kh, kq) = (2kh + (kq >> 1)) ^ 4(kq & 1) -- the k order in which that kernel's
// bank-conflict-free LDS image delivers the activations
static void pack_arsb(const Param& W, ConvLayer& L, BlobBuilder& bb, float fold, bool want_lo)
{
    const int cout = (int)W.shape[0], cin = (int)W.shape[1];
    L.w_arsb = bb.take((size_t)4 * 18 * 512 * 2);
    if (want_lo) L.w_arsb_lo = bb.take((size_t)4 * 18 * 512 * 2);
    for (int w = 0; w < 4; ++w)
        for (int f = 0; f < 18; ++f) {
            const int tap = f >> 1, kh = f & 1;
            for (int l = 0; l < 64; ++l) {
                const int m = l & 15, kq = l >> 4;
                const int slot = (2 * kh + (kq >> 1)) ^ (4 * (kq & 1));
                for (int e = 0; e < 8; ++e) {
                    const int oc = 16 * w + m, ci = 8 * slot + e;
                    const float v = (oc < cout && ci < cin) ? W.data[((size_t)oc * cin + ci) * 9 + tap] * fold : 0.f;
                    const half_t hv = (half_t)v;
                    bb.at<half_t>(L.w_arsb)[((size_t)(w * 18 + f) * 64 + l) * 8 + e] = hv;
                    if (want_lo) bb.at<half_t>(L.w_arsb_lo)[((size_t)(w * 18 + f) * 64 + l) * 8 + e] = (half_t)((v - (float)hv) * 2048.f);
                }
            }
        }
}

// OCP fp8 e4m3 (4 exponent bits, bias 7, no infinities, one NaN code; largest finite value 448), round to nearest even, saturating
static unsigned char to_e4m3(float v)
{
    const unsigned char sign = std::signbit(v) ? 0x80 : 0;
    float x = std::fabs(v);
    if (!(x == x)) return sign | 0x7F;
    if (x >= 448.f) return sign | 0x7E;
    if (x < 0.0009765625f) return sign;                       // below half of the smallest subnormal (2^-9): zero (ties to even: 2^-10 -> 0)
    int e;
    (void)std::frexp(x, &e);                                  // x = m 2^e, m in [0.5, 1)
    int ex = e - 1;                                           // x = 1.f 2^ex
    if (ex < -6) ex = -6;                                     // subnormal: spacing 2^-9
    const float q = std::ldexp(1.f, ex - 3);                  // spacing of the grid at this exponent
    float n = std::nearbyint(x / q);                          // (default rounding mode: to nearest even)
    float y = n * q;
    if (y >= 448.f) return sign | 0x7E;
    if (y < 0.015625f) return sign | (unsigned char)(int)std::nearbyint(y * 512.f);      // subnormal: mantissa = y / 2^-9
    int e2;
    const float m2 = std::frexp(y, &e2);                      // y = m2 2^e2
    const int ebits = e2 - 1 + 7;
    const int mbits = (int)std::nearbyint((m2 * 2.f - 1.f) * 8.f);
    return sign | (unsigned char)((ebits << 3) | mbits);
}

// fp8 weight parts of a 3x3 64->64 conv for conv64_q8.hip: lane l of fragment (tap, half c) holds output channel 32c + (l & 31), input channels
// 32 (l >> 5) .. + 31 of that tap; both parts carry a factor 2^8 (the kernel's E8M0 scale takes it out again)
static void pack_q8(const Param& W, ConvLayer& L, BlobBuilder& bb, float fold)
{
    const int cout = (int)W.shape[0], cin = (int)W.shape[1];
    // a weight of 1.75 or more would saturate (448 / 2^8) and its correction product would be wrong by the excess: such a layer keeps conv64_x3
    for (size_t i = 0; i < (size_t)cout * cin * 9; ++i)
        if (!(std::fabs(W.data[i] * fold) < 1.75f)) return;
    L.wq_hi8 = bb.take((size_t)9 * 2 * 64 * 32);
    L.wq_lo8 = bb.take((size_t)9 * 2 * 64 * 32);
    for (int tap = 0; tap < 9; ++tap)
        for (int c = 0; c < 2; ++c)
            for (int l = 0; l < 64; ++l)
                for (int b = 0; b < 32; ++b) {
                    const int oc = 32 * c + (l & 31), ci = 32 * (l >> 5) + b;
                    const float v = (oc < cout && ci < cin) ? W.data[((size_t)oc * cin + ci) * 9 + tap] * fold : 0.f;
                    const half_t hv = (half_t)v;
                    const size_t idx = ((size_t)(tap * 2 + c) * 64 + l) * 32 + b;
                    bb.at<unsigned char>(L.wq_hi8)[idx] = to_e4m3((float)hv * 256.f);
                    bb.at<unsigned char>(L.wq_lo8)[idx] = to_e4m3((float)(half_t)((v - (float)hv) * 2048.f) * 256.f);
                }
}

static float scalar_of(const moe_net& n, const std::string& name) { return n.get(name)->data[0]; }

void moe::drop_lut(moe_net& n)
{
    if (n.lut) { (void)hipDeviceSynchronize(); (void)hipFree(n.lut); }      // (a forward reading the table may be in flight; rare: weights or options changed)
    n.lut = nullptr; n.lut_state = 0;
}

namespace {

// the blob of one net under construction: what the families below register their layers and tables with
struct Packer {
    moe_net& n;
    const int precision;
    const bool mixed = precision == MOE_PREC_MIXED, plain = precision == MOE_PREC_DEBUG_DIRECT;
    BlobBuilder bb;
    void conv(const std::string& key, const std::string& wname, const char* bname, int r, float slope, float scale, bool per_plane = false);
    void f32table(const std::string& key, const std::vector<float>& v);
    void stem(const std::string& wname);
    void tail(const std::string& key, const std::string& wname);
    void arsb_nets();      // Net2x / Net3x / Net4x, NetDN
    void sedn();
    void lite();
};

void Packer::conv(const std::string& key, const std::string& wname, const char* bname, int r, float slope, float scale, bool per_plane)
{
    ConvLayer L;
    const Param* b = bname ? n.get(bname) : nullptr;
    // low-order weight parts: every conv under FP16X3; under MIXED the trunk convs that may run with split operands
    const bool lo = precision == MOE_PREC_FP16X3 || (mixed && (key == "input2" || key.compare(0, 3, "c1_") == 0 || key.compare(0, 3, "c2_") == 0));
    // the debug path keeps the plain weights and applies the scale in its epilogue; the MFMA kernels get it pre-multiplied
    pack_conv(*n.get(wname), b, r, L, bb, lo, plain, per_plane, plain ? 1.f : scale);
    L.slope = slope; L.scale = plain ? scale : 1.f; L.per_plane = per_plane;
    // every bias-free 3x3 conv with <= 64 channels in and out (the trunks of Net*x / NetDN, lite's LB convs, SEDN's rblock.0/2) also gets
    // the register-resident weight order of conv64_x3.hip (+ its low part where split operands may be asked for)
    if (!plain && r == 1 && L.taps == 9 && L.nseg == 1 && L.nchunks == 1 && !b && !per_plane)
    {
        pack_arsb(*n.get(wname), L, bb, scale, lo);
        if (lo) pack_q8(*n.get(wname), L, bb, scale);
    }
    n.conv_index[key] = (int)n.convs.size();
    n.convs.push_back(L);
}

void Packer::f32table(const std::string& key, const std::vector<float>& v)
{
    const size_t o = bb.take(v.size() * 4);
    memcpy(bb.at<float>(o), v.data(), v.size() * 4);
    n.small[key] = o;
}

void Packer::stem(const std::string& wname)      // [tap][64] fp32
{
    const Param& W = *n.get(wname);
    const int C = (int)W.shape[0], taps = (int)(W.shape[2] * W.shape[3]);
    std::vector<float> t((size_t)taps * 64, 0.f);
    for (int c = 0; c < C; ++c) for (int k = 0; k < taps; ++k) t[(size_t)k * 64 + c] = W.data[(size_t)c * taps + k];
    f32table("stem", t);
    n.scalars["stem_taps"] = (float)taps;
}

void Packer::tail(const std::string& key, const std::string& wname)      // [tap][64] fp16 (+lo)
{
    const Param& W = *n.get(wname);
    const int C = (int)W.shape[1], taps = (int)(W.shape[2] * W.shape[3]);
    const size_t o = bb.take((size_t)taps * 64 * 2), ol = bb.take((size_t)taps * 64 * 2);
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < taps; ++k) {
            const float v = W.data[(size_t)c * taps + k];
            const half_t hv = (half_t)v;
            bb.at<half_t>(o)[(size_t)k * 64 + c] = hv;
            bb.at<half_t>(ol)[(size_t)k * 64 + c] = (half_t)((v - (float)hv) * 2048.f);
        }
    n.small[key] = o; n.small[key + ".lo"] = ol;
    n.scalars["tail_taps"] = (float)taps;
    if (taps == 9) {   // A fragments for the fused tail (conv3x3_sp EPI 3): slice i = 16 channels, lane row = tap, k = (hh, e)
        // Rows 0..8 carry the fp16 weights of the nine taps, rows 16..24 their rounding remainders (w - fp16(w)) * 2^11: the same
        // MFMA that forms the tap sums also forms the low-order sums (23 of the 32 rows were idle), and the epilogue adds
        // row 16+t * 2^-11 to row t -- the tail conv sees its weights to ~22 bits at no extra matrix work.
        // Fragments 4..7 (EPI 7, the activation operand split as well): the fp16 weights again, but in rows 16..24 -- multiplied by the
        // activations' low parts (units of 2^-11) they accumulate into the same low-order rows.
        const size_t of = bb.take(8 * 512 * 2);
        for (int i = 0; i < 8; ++i)
            for (int l = 0; l < 64; ++l)
                for (int e8 = 0; e8 < 8; ++e8) {
                    const int row = l & 31, hh = l >> 5;
                    const int tap = row < 9 ? row : (row >= 16 && row < 25 ? row - 16 : -1);
                    const int ch = (i & 3) * 16 + (e8 < 4 ? 4 * hh + e8 : 8 + 4 * hh + (e8 - 4));
                    float v = 0.f;
                    if (tap >= 0 && ch < C) {
                        const float wv = W.data[(size_t)ch * taps + tap];
                        const half_t hv = (half_t)wv;
                        if (i < 4) v = row < 9 ? (float)hv : (wv - (float)hv) * 2048.f;
                        else v = row < 9 ? 0.f : (float)hv;
                    }
                    bb.at<half_t>(of)[(i * 64 + l) * 8 + e8] = (half_t)v;
                }
        n.small[key + ".frag"] = of;
    }
}

void Packer::arsb_nets()
{
    stem("conv_input.weight");
    n.scalars["stem_slope"] = scalar_of(n, "relu.weight");
    conv("input2", "conv_input2.weight", nullptr, 1, 1.f, 1.f);
    for (int i = 1; i <= 6; ++i) {
        const std::string p = "convt_F" + std::to_string(i) + ".0.";
        conv("c1_" + std::to_string(i), p + "conv_1.weight", nullptr, 1, scalar_of(n, p + "relu.weight"), 1.f);
        conv("c2_" + std::to_string(i), p + "conv_2.weight", nullptr, 1, 1.f, scalar_of(n, p + "scale.scale"));
    }
    if (n.arch == MOE_ARCH_NETDN) {
        tail("tail_r", "convt_R1.weight");
        tail("tail_u", "u.weight");
    } else {
        for (const char* br : {"u", "convt_R1"}) {
            for (int s = 0; s < n.stages; ++s) {
                const std::string p = std::string(br) + "." + std::to_string(s) + ".";
                conv(std::string(br) + ".up" + std::to_string(s), p + "0.weight", (p + "0.bias").c_str(), n.r,
                     scalar_of(n, p + "2.weight"), 1.f);
            }
        }
        tail("tail_r", "convt_R1." + std::to_string(n.stages) + ".weight");
        tail("tail_u", "u." + std::to_string(n.stages) + ".weight");
    }
}

void Packer::sedn()
{
    stem("conv_input.weight");
    n.scalars["stem_slope"] = 0.2f;
    for (int b = 0; b < 16; ++b) {
        const std::string p = "convt_F1." + std::to_string(b) + ".", k = "b" + std::to_string(b);
        conv(k + ".rb0", p + "rblock.0.weight", nullptr, 1, 0.2f, 1.f);
        conv(k + ".rb2", p + "rblock.2.weight", nullptr, 1, 0.2f, 1.f);
        conv(k + ".rb4", p + "rblock.4.weight", nullptr, 1, 1.f, 1.f);
        conv(k + ".trans", p + "trans.0.weight", nullptr, 1, 0.2f, 1.f, true);
        f32table(k + ".down", n.get(p + "conv_down.weight")->data);
        f32table(k + ".up", n.get(p + "conv_up.weight")->data);
        {   // fused block tail (sedn_fuse): rblock.4 as [256][tap*64 + ci] and transposed, trans as [64][256], all fp32
            const Param& W4 = *n.get(p + "rblock.4.weight");
            std::vector<float> w256((size_t)256 * 576), w256t((size_t)576 * 256);
            for (int m = 0; m < 256; ++m)
                for (int ci = 0; ci < 64; ++ci)
                    for (int tap = 0; tap < 9; ++tap) {
                        const float v = W4.data[((size_t)m * 64 + ci) * 9 + tap];
                        w256[(size_t)m * 576 + tap * 64 + ci] = v;
                        w256t[(size_t)(tap * 64 + ci) * 256 + m] = v;
                    }
            f32table(k + ".w256", w256);
            f32table(k + ".w256t", w256t);
            f32table(k + ".wt", n.get(p + "trans.0.weight")->data);
        }
    }
    tail("tail_r", "convt_R1.weight");
}

void Packer::lite()
{
    stem("conv_input.weight");
    n.scalars["stem_slope"] = scalar_of(n, "relu.weight");
    conv("input2", "conv_input2.weight", nullptr, 1, 1.f, 1.f);
    {   // conv_input2(PReLU(conv_input(x))) in closed form (MoeNet_lite2.py:40-41: one input channel, 1x1 kernels, no bias): PReLU(w_s[c] x) = x p[c] for x >= 0 and
        // x q[c] for x < 0 (p, q = w_s[c] or slope w_s[c] by the sign of w_s[c]), so conv_input2's output is x P / x Q with P = W2 p, Q = W2 q, summed in double here
        const Param& Ws = *n.get("conv_input.weight");
        const Param& W2 = *n.get("conv_input2.weight");
        const double sl = (double)scalar_of(n, "relu.weight");
        std::vector<float> pq(2 * 64, 0.f);
        for (int co = 0; co < 48; ++co) {
            double P = 0.0, Q = 0.0;
            for (int c = 0; c < 48; ++c) {
                const double w = (double)Ws.data[c], w2 = (double)W2.data[(size_t)co * 48 + c];
                P += w2 * (w >= 0.0 ? w : sl * w);
                Q += w2 * (w <= 0.0 ? w : sl * w);
            }
            pq[co] = (float)P; pq[64 + co] = (float)Q;
        }
        f32table("stem.p2", pq);
    }
    for (int k = 1; k <= 3; ++k) {
        const std::string p = "convt_F1" + std::to_string(k) + ".", key = "lb" + std::to_string(k);
        conv(key + ".c1", p + "conv_1.weight", nullptr, 1, scalar_of(n, p + "relu.weight"), 1.f);
        conv(key + ".c2", p + "conv_2.weight", nullptr, 1, 1.f, 1.f);
        // FRM tables padded to 64 channels: w0 [3][64], b0 [3], w2 [64][3], b2 [64]
        std::vector<float> w0(3 * 64, 0.f), w2(64 * 3, 0.f), b2(64, 0.f);
        const Param& W0 = *n.get(p + "se.conv_du.0.weight");
        const Param& W2 = *n.get(p + "se.conv_du.2.weight");
        for (int j = 0; j < 3; ++j) for (int c = 0; c < 48; ++c) w0[j * 64 + c] = W0.data[j * 48 + c];
        for (int c = 0; c < 48; ++c) { for (int j = 0; j < 3; ++j) w2[c * 3 + j] = W2.data[c * 3 + j]; b2[c] = n.get(p + "se.conv_du.2.bias")->data[c]; }
        f32table(key + ".w0", w0);
        f32table(key + ".b0", n.get(p + "se.conv_du.0.bias")->data);
        f32table(key + ".w2", w2);
        f32table(key + ".b2", b2);
        // conv_2's weights once more, fp32 and transposed: [tap*64 + ci][co 64] -- the gate's pooled mean is this matrix applied to the window sums of conv_2's input (frm_pre)
        std::vector<float> c2t((size_t)576 * 64, 0.f);
        const Param& C2 = *n.get(p + "conv_2.weight");
        for (int co = 0; co < 48; ++co)
            for (int ci = 0; ci < 48; ++ci)
                for (int tap = 0; tap < 9; ++tap) c2t[(size_t)(tap * 64 + ci) * 64 + co] = C2.data[((size_t)co * 48 + ci) * 9 + tap];
        f32table(key + ".c2t", c2t);
    }
    for (const char* br : {"ures", "uim"})
        for (int s = 0; s < n.stages; ++s) {
            const std::string p = std::string(br) + "." + std::to_string(s) + ".";
            conv(std::string(br) + ".up" + std::to_string(s), p + "0.weight", (p + "0.bias").c_str(), 2, scalar_of(n, p + "2.weight"), 1.f);
        }
    tail("tail_r", "convt_R1.weight");
    tail("tail_u", "convt_I1.weight");
    for (const char* kv : {"tail_r", "tail_u"}) {     // fp32 copies for the fused 1x1 tail (conv_mfma_kernel, tail1_w)
        const Param& W = *n.get(std::string(kv) == "tail_r" ? "convt_R1.weight" : "convt_I1.weight");
        std::vector<float> t(64, 0.f);
        for (int c = 0; c < (int)W.shape[1]; ++c) t[c] = W.data[c];
        f32table(std::string(kv) + ".f32", t);
    }
}

}  // namespace

int moe::build_device_weights(moe_net& n, int precision)
{
    drop_lut(n);      // (the table holds the U branch of the weights packed before)

    n.convs.clear(); n.conv_index.clear(); n.small.clear(); n.scalars.clear();
    Packer pk{n, precision};
    BlobBuilder& bb = pk.bb;
    n.small["zero"] = bb.take(1024);
    n.small["trash"] = bb.take(4096);
    n.small["zero_bias"] = bb.take(1024 * 4);      // up to 16 chunks of 64 fp32 zeros
    n.small["zero_bias_img"] = bb.take(16 * 256 * 4);   // the same as 1-KiB-per-chunk images (conv3x3_sp)

    if (n.arch == MOE_ARCH_NET2X || n.arch == MOE_ARCH_NET3X || n.arch == MOE_ARCH_NET4X || n.arch == MOE_ARCH_NETDN) pk.arsb_nets();
    else if (n.arch == MOE_ARCH_SEDN) pk.sedn();
    else pk.lite();

    if (n.blob) { (void)hipFree(n.blob); n.blob = nullptr; }
    HIP_TRY(hipMalloc((void**)&n.blob, bb.data.size()));
    n.blob_bytes = bb.data.size();
    HIP_TRY(hipMemcpy(n.blob, bb.data.data(), bb.data.size(), hipMemcpyHostToDevice));
    return MOE_OK;
}

extern "C" {

int moe_net_create(int arch, int scale, moe_net** out)
{
    if (!out) return fail(MOE_EINVAL, "moe_net_create: out is NULL");
    auto n = std::make_unique<moe_net>();
    n->arch = arch;
    n->opt.from_env();
    switch (arch) {
        case MOE_ARCH_NET2X: n->scale = 2; n->stages = 1; n->r = 2; break;
        case MOE_ARCH_NET3X: n->scale = 3; n->stages = 1; n->r = 3; break;
        case MOE_ARCH_NET4X: n->scale = 4; n->stages = 2; n->r = 2; break;
        case MOE_ARCH_NETDN: n->scale = 1; n->stages = 0; n->C = 48; break;
        case MOE_ARCH_SEDN: n->scale = 1; n->stages = 0; break;
        case MOE_ARCH_LITE:
            if (scale != 2 && scale != 4 && scale != 8) return fail(MOE_EINVAL, "MoeNet_lite2.Net: upscale must be 2, 4 or 8 (got %d)", scale);
            n->scale = scale; n->r = 2; n->C = 48;
            n->stages = scale == 2 ? 1 : (scale == 4 ? 2 : 3);
            break;
        default: return fail(MOE_EINVAL, "moe_net_create: unknown architecture %d", arch);
    }
    if (arch != MOE_ARCH_LITE && scale != 0 && scale != n->scale)
        return fail(MOE_EINVAL, "moe_net_create: architecture %d has scale %d, not %d", arch, n->scale, scale);
    declare_params(*n);
    *out = n.release();
    return MOE_OK;
}

void moe_net_destroy(moe_net* n)
{
    if (!n) return;
    drop_lut(*n);
    if (n->blob) (void)hipFree(n->blob);
    pipe_destroy(*n);
    free_set(n->set);
    free_records(n->rt);
    free_ens_scratch(*n);
    delete n;
}

int moe_net_scale(const moe_net* n) { return n ? n->scale : 0; }
int moe_net_num_params(const moe_net* n) { return n ? (int)n->params.size() : 0; }

int moe_net_param_info(const moe_net* n, int i, const char** name, int64_t shape[4], int* ndim)
{
    if (!n || i < 0 || i >= (int)n->params.size()) return fail(MOE_EINVAL, "moe_net_param_info: index out of range");
    const Param& p = n->params[i];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = (int)p.shape.size();
    if (shape) for (size_t d = 0; d < p.shape.size() && d < 4; ++d) shape[d] = p.shape[d];
    return MOE_OK;
}

int moe_net_set_param(moe_net* n, const char* name, const float* data, const int64_t* shape, int ndim)
{
    if (!n || !name || !data) return fail(MOE_EINVAL, "moe_net_set_param: NULL argument");
    auto it = n->index.find(name);
    if (it == n->index.end()) return fail(MOE_EINVAL, "Unexpected key(s) in state_dict: \"%s\"", name);
    Param& p = n->params[it->second];
    bool same = (int)p.shape.size() == ndim;
    for (int d = 0; same && d < ndim; ++d) same = p.shape[d] == shape[d];
    if (!same) {
        std::string got, want;
        for (int d = 0; d < ndim; ++d) got += (d ? ", " : "") + std::to_string((long long)shape[d]);
        for (size_t d = 0; d < p.shape.size(); ++d) want += (d ? ", " : "") + std::to_string((long long)p.shape[d]);
        return fail(MOE_EINVAL, "size mismatch for %s: copying a param with shape (%s), the shape in current model is (%s)", name, got.c_str(), want.c_str());
    }
    p.data.assign(data, data + p.numel());
    p.set = true;
    n->finalized = false;
    n->calib_valid = false;          // (a measurement of other weights)
    n->auto_resolved = -1;
    return MOE_OK;
}

// MOE_PREC_AUTO: the arithmetic that holds the product's tolerance (1e-3 max-abs against the reference's fp32 CPU path, on natural images and on white
// noise) for the family -- the per-family policy lives HERE, behind the C ABI, so that the one-line stub of INTEGRATION.md works for every plugin-table key
static int resolve_precision(int arch, int precision)
{
    if (precision != MOE_PREC_AUTO) return precision;
    switch (arch) {
        case MOE_ARCH_SEDN: return MOE_PREC_FP16;       // l15 / l25 / l50: 4-6e-4 in plain fp16 on the synthetic l25; moe_net_finalize measures the checkpoint
        case MOE_ARCH_LITE: return MOE_PREC_FP16X3;     // lite2 / 4 / 8: every conv but one would have to be split anyway
        default: return MOE_PREC_MIXED;                 // Net2x / 3x / 4x, NetDN
    }
}

int moe_net_resolved_precision(const moe_net* n, int precision)
{
    if (!n) return fail(MOE_EINVAL, "moe_net_resolved_precision: NULL net");
    if (precision < MOE_PREC_FP16 || precision > MOE_PREC_AUTO) return fail(MOE_EINVAL, "moe_net_resolved_precision: unknown precision %d", precision);
    if (precision == MOE_PREC_AUTO && n->auto_resolved >= 0) return n->auto_resolved;      // (what the last finalize with AUTO settled on for these weights)
    return resolve_precision(n->arch, precision);
}

int moe_net_finalize(moe_net* n, int device, int precision)
{
    if (!n) return fail(MOE_EINVAL, "moe_net_finalize: NULL net");
    const bool autop = precision == MOE_PREC_AUTO;
    if (precision == MOE_PREC_AUTO) precision = resolve_precision(n->arch, precision);
    if (precision != MOE_PREC_FP16 && precision != MOE_PREC_FP16X3 && precision != MOE_PREC_DEBUG_DIRECT && precision != MOE_PREC_MIXED)
        return fail(MOE_EINVAL, "moe_net_finalize: unknown precision %d", precision);
    if (precision == MOE_PREC_MIXED && (n->arch == MOE_ARCH_SEDN || n->arch == MOE_ARCH_LITE))
        return fail(MOE_EINVAL, "moe_net_finalize: MOE_PREC_MIXED is defined for Net2x/3x/4x and NetDN (use FP16 for SEDN, FP16X3 for lite)");
    std::string missing;
    for (const auto& p : n->params) if (!p.set) missing += (missing.empty() ? "\"" : ", \"") + p.name + "\"";
    if (!missing.empty()) return fail(MOE_ESTATE, "Missing key(s) in state_dict: %s", missing.c_str());
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt < 1) { (void)hipGetLastError(); return fail(MOE_EHIP, "no HIP device available (this engine has no CPU path)"); }
    if (device < 0 || device >= cnt) return fail(MOE_EINVAL, "device %d out of range (%d visible)", device, cnt);
    if (n->device >= 0 && n->device != device) {
        // the net moves to another device: its streams, events and workspace belong to the old one (the side stream of small launch sets was created once and
        // would have been used on the new device's forwards); the weight blob is rebuilt below
        (void)hipSetDevice(n->device);
        (void)hipDeviceSynchronize();
        pipe_destroy(*n);
        free_set(n->set);
        free_records(n->rt);
        free_ens_scratch(*n);
        if (n->blob) { (void)hipFree(n->blob); n->blob = nullptr; n->blob_bytes = 0; }
        n->calib_valid = false;      // (measured on the other device: the arithmetic is the same, but the rule is one measurement per checkpoint AND device)
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(conv_mfma_init());
    n->max_groups = conv_mfma_max_groups();
    if (n->opt.max_groups > 0) n->max_groups = n->opt.max_groups;
    n->device = device;
    n->precision = precision;
    int rc = build_device_weights(*n, precision);
    if (rc) return rc;
    n->finalized = true;
    if (autop) {
        // MOE_PREC_AUTO promises the 1e-3 contract for THIS checkpoint, not for the zoo's: the ARSB nets measure their count of split-operand blocks on the device
        // now (calibrate_blocks above; once per checkpoint -- the result is kept until a parameter changes), and fall back to FP16X3 when no count reaches the target.
        // An explicit moe_net_set_exact_blocks / MOE_EXACT_BLOCKS or option auto_calibrate = 0 leaves the per-architecture default in force.
        if (precision == MOE_PREC_MIXED && calibratable(*n) && n->opt.auto_calibrate && n->exact_blocks < 0 && n->opt.exact_blocks_env < 0) {
            if (!n->calib_valid) {
                // the measurement's device work (three weight rebuilds, up to seven forwards) runs on a stream of its own: the legacy NULL stream would serialise against
                // every blocking stream of the process and is illegal while another stream captures; callers with a stream of theirs use moe_net_calibrate
                hipStream_t cs = nullptr;
                HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
                rc = calibrate_blocks(*n, 0.0, cs);
                (void)hipStreamSynchronize(cs);
                (void)hipStreamDestroy(cs);
                if (rc) { n->finalized = false; return rc; }
            }
            if (n->calib_blocks < 0) {
                rc = build_device_weights(*n, MOE_PREC_FP16X3);
                if (rc) { n->finalized = false; return rc; }
                n->precision = precision = MOE_PREC_FP16X3;
            }
        }
        // SEDN: the family's default is plain fp16; whether THIS checkpoint holds the contract in it is measured the same way (calibrate_sedn: fp16 as it ships against
        // the exact mode), and a checkpoint that does not runs in FP16X3 -- whose weights the measurement then leaves on the device.  auto_calibrate = 0: fp16, unmeasured.
        if (n->arch == MOE_ARCH_SEDN && precision == MOE_PREC_FP16 && n->opt.auto_calibrate) {
            if (!n->calib_valid) {
                hipStream_t cs = nullptr;
                HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
                rc = calibrate_sedn(*n, 0.0, cs, true);
                (void)hipStreamSynchronize(cs);
                (void)hipStreamDestroy(cs);
                if (rc) { n->finalized = false; return rc; }
                precision = n->precision;
            } else if (n->calib_blocks < 0) {
                rc = build_device_weights(*n, MOE_PREC_FP16X3);
                if (rc) { n->finalized = false; return rc; }
                n->precision = precision = MOE_PREC_FP16X3;
            }
        }
        n->auto_resolved = precision;
    }
    return MOE_OK;
}

}  // extern "C"
