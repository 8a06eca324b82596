// chroma_args_check.cpp -- every refusal of moe_chroma_resample (include/moephoto_amd.h), called from a stand-alone program so that the argument validation in
// polyphase.cpp -- the walk over the caller's coefficient and offset tables included -- can run under the host sanitizers.  No device is touched: every call must
// return before its first HIP call.  The tables are heap blocks of exactly scale x taps / scale elements, so a read past either end is an AddressSanitizer report.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       polyphase.cpp errors.cpp ../../tools/chroma_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/chroma_args_check
//   /tmp/chroma_args_check          (exit status 0 and "chroma_args_check: N refusals, all as declared")
//
// polyphase.cpp and errors.cpp are compiled into the program with the sanitizers (the program's definitions win over the library's); the library only
// supplies the kernels' launchers those files refer to.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/moephoto_amd.h"

static int n_checked = 0, n_bad = 0;

static void expect(int rc, int want, const char* text, const char* what)
{
    ++n_checked;
    const char* msg = moe_last_error();
    if (rc != want || !msg || !strstr(msg, text)) {
        ++n_bad;
        fprintf(stderr, "%s: rc %d (want %d), message \"%s\" (want \"%s\" in it)\n", what, rc, want, msg ? msg : "(null)", text);
    }
}

// The tables of one call: the bilinear filter at `scale` with centre siting (phase p: f = frac((2p + 1 - scale) / (2 scale)), the weights (1 - f, f) in 14 bits), or
// for other tap counts a unit tap in front of zeros -- valid tables, which the cases below then spoil.
struct Tables {
    std::vector<int16_t> cx, cy;
    std::vector<int8_t> ox, oy;
    Tables(int scale, int taps) : cx(scale * taps, 0), cy(scale * taps, 0), ox(scale, 0), oy(scale, 0)
    {
        for (int p = 0; p < scale; ++p) {
            const int num = 2 * p + 1 - scale, den = 2 * scale, fl = num < 0 ? -1 : 0, f = (num - fl * den) * 16384 / den;
            if (taps == 2) {
                cx[p * 2] = cy[p * 2] = (int16_t)(16384 - f);
                cx[p * 2 + 1] = cy[p * 2 + 1] = (int16_t)f;
                ox[p] = oy[p] = (int8_t)fl;
            } else cx[p * taps] = cy[p * taps] = 16384;
        }
    }
};

int main()
{
    alignas(16) static unsigned char buf[4096];
    void* src = buf;
    void* dst = buf + 2048;
    void* odd_src = buf + 1;
    void* odd_dst = buf + 2049;
#define CR(s, ds, h, w, d, dd, scale, taps, t) moe_chroma_resample(s, ds, h, w, d, dd, scale, taps, (t).cx.data(), (t).ox.data(), (t).cy.data(), (t).oy.data(), 0, nullptr)
    const Tables t2(2, 2);
    expect(CR(nullptr, 10, 3, 5, dst, 10, 2, 2, t2), MOE_EINVAL, "moe_chroma_resample: NULL", "src");
    expect(CR(src, 10, 3, 5, nullptr, 10, 2, 2, t2), MOE_EINVAL, "NULL", "dst");
    expect(moe_chroma_resample(src, 10, 3, 5, dst, 10, 2, 2, nullptr, t2.ox.data(), t2.cy.data(), t2.oy.data(), 0, nullptr), MOE_EINVAL, "NULL", "cx");
    expect(moe_chroma_resample(src, 10, 3, 5, dst, 10, 2, 2, t2.cx.data(), nullptr, t2.cy.data(), t2.oy.data(), 0, nullptr), MOE_EINVAL, "NULL", "ox");
    expect(moe_chroma_resample(src, 10, 3, 5, dst, 10, 2, 2, t2.cx.data(), t2.ox.data(), nullptr, t2.oy.data(), 0, nullptr), MOE_EINVAL, "NULL", "cy");
    expect(moe_chroma_resample(src, 10, 3, 5, dst, 10, 2, 2, t2.cx.data(), t2.ox.data(), t2.cy.data(), nullptr, 0, nullptr), MOE_EINVAL, "NULL", "oy");
    const int depths[] = {-8, 0, 7, 9, 11, 14, 17, 32};
    for (int d : depths) {
        expect(CR(src, d, 3, 5, dst, 10, 2, 2, t2), MOE_EINVAL, "depth", "src depth");
        expect(CR(src, 10, 3, 5, dst, d, 2, 2, t2), MOE_EINVAL, "depth", "dst depth");
    }
    const int sizes[][2] = {{0, 5}, {3, 0}, {-1, 5}, {3, -7}, {0, 0}};
    for (auto& s : sizes) expect(CR(src, 10, s[0], s[1], dst, 10, 2, 2, t2), MOE_EINVAL, "must be positive", "size");
    const int scales[] = {0, -1, 17, 64};
    for (int s : scales) expect(CR(src, 10, 3, 5, dst, 10, s, 2, t2), MOE_EINVAL, "scale", "scale");      // (refused before a table is read: t2 holds two phases only)
    expect(CR(src, 10, 1 << 30, 5, dst, 10, 2, 2, t2), MOE_EINVAL, "does not fit", "h * scale");
    expect(CR(src, 10, 3, 1 << 30, dst, 10, 2, 2, t2), MOE_EINVAL, "does not fit", "w * scale");
    const int taps[] = {0, 3, 5, 8, -1};
    for (int t : taps) expect(CR(src, 10, 3, 5, dst, 10, 2, t, t2), MOE_EINVAL, "taps", "taps");
    expect(CR(odd_src, 10, 3, 5, dst, 10, 2, 2, t2), MOE_EINVAL, "src is not 2-byte aligned", "odd src at 10 bits");
    expect(CR(odd_src, 16, 3, 5, dst, 8, 2, 2, t2), MOE_EINVAL, "src is not 2-byte aligned", "odd src at 16 bits");
    expect(CR(src, 10, 3, 5, odd_dst, 12, 2, 2, t2), MOE_EINVAL, "dst is not 2-byte aligned", "odd dst at 12 bits");
    expect(CR(odd_src, 8, 3, 5, odd_dst, 16, 2, 2, t2), MOE_EINVAL, "dst is not 2-byte aligned", "odd src is fine at 8 bits, odd dst is not at 16");
    // tables: every scale's last phase spoilt on either axis, for each tap count (the walk reaches the last element of exact-size blocks)
    const int all_taps[] = {1, 2, 4}, some_scales[] = {1, 2, 3, 16};
    for (int tp : all_taps)
        for (int sc : some_scales) {
            for (int axis = 0; axis < 2; ++axis) {
                Tables t(sc, tp);
                auto& c = axis ? t.cy : t.cx;
                c[sc * tp - 1] += 1;                                     // the row sums to 2^14 + 1
                expect(CR(src, 10, 3, 5, dst, 10, sc, tp, t), MOE_EINVAL, axis ? "vertical coefficients" : "horizontal coefficients", "row sum");
                Tables o(sc, tp);
                (axis ? o.oy : o.ox)[sc - 1] = 2;
                expect(CR(src, 10, 3, 5, dst, 10, sc, tp, o), MOE_EINVAL, axis ? "vertical offset 2" : "horizontal offset 2", "offset above 1");
                (axis ? o.oy : o.ox)[sc - 1] = -3;
                expect(CR(src, 10, 3, 5, dst, 10, sc, tp, o), MOE_EINVAL, axis ? "vertical offset -3" : "horizontal offset -3", "offset below -2");
            }
        }
    {   // a row that sums to 2^14 with magnitudes beyond the int32 bound: 2^14 + 8192 + 8192 + ... = 16384 + 2 * 8193 > 32767
        Tables t(2, 4);
        int16_t row[4] = {-8193, 16385, 16385, -8193};
        memcpy(&t.cx[4], row, sizeof(row));
        expect(CR(src, 16, 3, 5, dst, 16, 2, 4, t), MOE_EINVAL, "magnitudes 49156", "magnitudes, horizontal");
        Tables u(2, 4);
        memcpy(&u.cy[0], row, sizeof(row));
        expect(CR(src, 16, 3, 5, dst, 16, 2, 4, u), MOE_EINVAL, "vertical coefficients of phase 0", "magnitudes, vertical");
    }
    if (n_bad) {
        fprintf(stderr, "chroma_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("chroma_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
