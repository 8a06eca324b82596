// planes_rgb_args_check.cpp -- every refusal of moe_planes_to_rgb (include/moephoto_amd.h), called from a stand-alone program so that the argument validation in
// polyphase.cpp -- the walk over the caller's coefficient, offset and constant tables included -- can run under the host sanitizers.  No device is touched: every call
// must return before its first HIP call.  The tables are heap blocks of exactly 2 x taps / 2 / 5 elements, so a read past either end is an AddressSanitizer report.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       polyphase.cpp errors.cpp ../../tools/planes_rgb_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/planes_rgb_args_check
//   /tmp/planes_rgb_args_check          (exit status 0 and "planes_rgb_args_check: N refusals, all as declared")
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

// The tables of one call: per phase one coefficient 2^14 in front of zeros, offset 0, and bt709's constants for 10-bit sources and 16-bit samples -- valid tables,
// which the cases below then spoil.
struct Tables {
    std::vector<int16_t> cx, cy;
    std::vector<int8_t> ox, oy;
    std::vector<int32_t> coef;
    explicit Tables(int taps) : cx(2 * taps, 0), cy(2 * taps, 0), ox(2, 0), oy(2, 0), coef{78446891, 120780616, -14366993, -35903186, 142316809}
    {
        for (int p = 0; p < 2; ++p) cx[p * taps] = cy[p * taps] = 16384;
    }
};

int main()
{
    // a 6 x 4 frame at up to 16 bits: src 72 bytes at buf, dst 144 bytes at buf + 1024
    alignas(16) static unsigned char buf[4096];
    void* src = buf + 512;
    void* dst = buf + 1024;
#define PR(s, depth, H, W, d, bits, matrix, order, taps, t) \
    moe_planes_to_rgb(s, depth, H, W, d, bits, matrix, order, taps, (t).cx.data(), (t).ox.data(), (t).cy.data(), (t).oy.data(), (t).coef.data(), 0, nullptr)
    const Tables t4(4);
    expect(PR(nullptr, 10, 4, 6, dst, 16, 0, 0, 4, t4), MOE_EINVAL, "moe_planes_to_rgb: NULL", "src");
    expect(PR(src, 10, 4, 6, nullptr, 16, 0, 0, 4, t4), MOE_EINVAL, "NULL", "dst");
    expect(moe_planes_to_rgb(src, 10, 4, 6, dst, 16, 0, 0, 4, nullptr, t4.ox.data(), t4.cy.data(), t4.oy.data(), t4.coef.data(), 0, nullptr), MOE_EINVAL, "NULL", "cx");
    expect(moe_planes_to_rgb(src, 10, 4, 6, dst, 16, 0, 0, 4, t4.cx.data(), nullptr, t4.cy.data(), t4.oy.data(), t4.coef.data(), 0, nullptr), MOE_EINVAL, "NULL", "ox");
    expect(moe_planes_to_rgb(src, 10, 4, 6, dst, 16, 0, 0, 4, t4.cx.data(), t4.ox.data(), nullptr, t4.oy.data(), t4.coef.data(), 0, nullptr), MOE_EINVAL, "NULL", "cy");
    expect(moe_planes_to_rgb(src, 10, 4, 6, dst, 16, 0, 0, 4, t4.cx.data(), t4.ox.data(), t4.cy.data(), nullptr, t4.coef.data(), 0, nullptr), MOE_EINVAL, "NULL", "oy");
    expect(moe_planes_to_rgb(src, 10, 4, 6, dst, 16, 0, 0, 4, t4.cx.data(), t4.ox.data(), t4.cy.data(), t4.oy.data(), nullptr, 0, nullptr), MOE_EINVAL, "NULL", "coef");
    const int depths[] = {-8, 0, 7, 9, 11, 14, 17, 32, 10 | MOE_Q_ROUND};
    for (int d : depths) expect(PR(src, d, 4, 6, dst, 16, 0, 0, 4, t4), MOE_EINVAL, "depth", "depth");
    const int bits[] = {0, 1, 10, 12, 24, 32, MOE_Q_ORDERED, 255 | MOE_Q_ROUND};
    for (int b : bits) expect(PR(src, 10, 4, 6, dst, b, 0, 0, 4, t4), MOE_EINVAL, "bits", "bits");
    expect(PR(src, 10, 4, 6, dst, 16 | MOE_Q_UNIT, 0, 0, 4, t4), MOE_EINVAL, "MOE_Q_UNIT", "unit scale alone");
    expect(PR(src, 10, 4, 6, dst, 8 | MOE_Q_UNIT | MOE_Q_ROUND, 0, 0, 4, t4), MOE_EINVAL, "MOE_Q_UNIT", "unit scale with a mode");
    expect(PR(src, 10, 4, 6, dst, 16 | MOE_Q_ROUND | MOE_Q_ORDERED, 0, 0, 4, t4), MOE_EINVAL, "both set", "two modes");
    expect(PR(src, 10, 4, 6, dst, 16 | 0x800, 0, 0, 4, t4), MOE_EINVAL, "unknown flags", "another high bit");
    expect(PR(src, 10, 4, 6, dst, -16, 0, 0, 4, t4), MOE_EINVAL, "unknown flags", "negative bits");
    const int sizes[][2] = {{5, 6}, {4, 7}, {0, 6}, {4, 0}, {1, 1}, {-2, 6}, {4, -6}, {3, 3}};
    for (auto& s : sizes) expect(PR(src, 10, s[0], s[1], dst, 16, 0, 0, 4, t4), MOE_EINVAL, "an even width and height", "size");
    expect(PR(src, 10, 1 << 15, 1 << 15, dst, 16, 0, 0, 4, t4), MOE_EINVAL, "do not fit an int", "3 H W");
    expect(PR(src, 10, 2, 1 << 30, dst, 16, 0, 0, 4, t4), MOE_EINVAL, "do not fit an int", "3 H W, a long row");
    const int matrices[] = {-1, 3, 9};
    for (int m : matrices) expect(PR(src, 10, 4, 6, dst, 16, m, 0, 4, t4), MOE_EINVAL, "matrix", "matrix");
    const int orders[] = {-1, 2, 7};
    for (int o : orders) expect(PR(src, 10, 4, 6, dst, 16, 0, o, 4, t4), MOE_EINVAL, "order", "order");
    const int tapss[] = {0, 3, 5, 8, 16, -1};
    for (int t : tapss) expect(PR(src, 10, 4, 6, dst, 16, 0, 0, t, t4), MOE_EINVAL, "taps", "taps");          // (refused before a table is read)
    expect(PR(buf + 513, 10, 4, 6, dst, 16, 0, 0, 4, t4), MOE_EINVAL, "src is not 2-byte aligned", "odd src at 10 bits");
    expect(PR(src, 10, 4, 6, buf + 1025, 16, 0, 0, 4, t4), MOE_EINVAL, "dst is not 2-byte aligned", "odd dst at 16 bits");
    expect(PR(buf + 513, 8, 4, 6, buf + 1025, 16, 0, 0, 4, t4), MOE_EINVAL, "dst is not 2-byte aligned", "an odd src is fine at 8 bits, an odd dst is not at 16");
    // tables: the last phase of every tap count spoilt on either axis (the walk reaches the last element of exact-size blocks)
    const int some_taps[] = {1, 2, 4};
    for (int taps : some_taps)
        for (int axis = 0; axis < 2; ++axis) {
            Tables t(taps);
            (axis ? t.cy : t.cx)[2 * taps - 1] += 1;                     // the row sums to 16385
            expect(PR(src, 8, 4, 6, dst, 8, 0, 0, taps, t), MOE_EINVAL, axis ? "vertical coefficients" : "horizontal coefficients", "row sum above");
            Tables u(taps);
            (axis ? u.cy : u.cx)[taps] -= 1;                             // 16383
            expect(PR(src, 8, 4, 6, dst, 8, 0, 0, taps, u), MOE_EINVAL, "sum to 16383", "row sum below");
            if (taps > 1) {
                Tables m(taps);
                (axis ? m.cy : m.cx)[taps] = 32767;                      // sums to 2^14 with magnitudes of 49150
                (axis ? m.cy : m.cx)[2 * taps - 1] = -16383;
                expect(PR(src, 8, 4, 6, dst, 8, 0, 0, taps, m), MOE_EINVAL, "magnitudes", "row magnitudes");
            }
            Tables o(taps);
            (axis ? o.oy : o.ox)[1] = 2;
            expect(PR(src, 8, 4, 6, dst, 8, 0, 0, taps, o), MOE_EINVAL, axis ? "vertical offset 2" : "horizontal offset 2", "offset above 1");
            (axis ? o.oy : o.ox)[1] = -3;
            expect(PR(src, 8, 4, 6, dst, 8, 0, 0, taps, o), MOE_EINVAL, axis ? "vertical offset -3" : "horizontal offset -3", "offset below -2");
        }
    const struct { int i; int32_t v; const char* name; } consts[] = {{0, 0, "cY"}, {0, -5, "cY"}, {0, (1 << 30) + 1, "cY"}, {1, (1 << 30) + 1, "cRV"}, {2, -(1 << 30) - 1, "cGU"},
                                                                      {3, INT32_MIN, "cGV"}, {4, INT32_MAX, "cBU"}};
    for (auto& c : consts) {
        Tables t(4);
        t.coef[c.i] = c.v;
        expect(PR(src, 10, 4, 6, dst, 16, 0, 0, 4, t), MOE_EINVAL, c.name, "matrix constant");
    }
    // dst at the start of, inside, across the end of and across the start of the 72 bytes of src
    const int overlaps[] = {0, 10, 70, -142};
    for (int at : overlaps) expect(PR(src, 10, 4, 6, buf + 512 + at, 16, 0, 0, 4, t4), MOE_EINVAL, "overlaps", "dst over src");
    if (n_bad) {
        fprintf(stderr, "planes_rgb_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("planes_rgb_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
