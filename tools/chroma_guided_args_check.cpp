// chroma_guided_args_check.cpp -- every refusal of moe_chroma_guided (include/moephoto_amd.h), called from a stand-alone program so that the argument validation in
// polyphase.cpp -- the walk over the caller's coefficient, offset and range tables included -- can run under the host sanitizers.  No device is touched: every call
// must return before its first HIP call.  The tables are heap blocks of exactly scale x 4 / scale / 64 elements, so a read past either end is an AddressSanitizer
// report.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       polyphase.cpp errors.cpp ../../tools/chroma_guided_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/chroma_guided_args_check
//   /tmp/chroma_guided_args_check          (exit status 0 and "chroma_guided_args_check: N refusals, all as declared")
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

// The tables of one call: per phase the B-spline's row at f = 0, (43, 170, 43, 0), offset -1, and a range table of ones -- valid tables, which the cases below then spoil.
struct Tables {
    std::vector<uint8_t> cx, cy, range;
    std::vector<int8_t> ox, oy;
    explicit Tables(int scale) : cx(scale * 4), cy(scale * 4), range(64, 1), ox(scale, -1), oy(scale, -1)
    {
        const uint8_t row[4] = {43, 170, 43, 0};
        for (int p = 0; p < scale; ++p) {
            memcpy(&cx[p * 4], row, 4);
            memcpy(&cy[p * 4], row, 4);
        }
    }
};

int main()
{
    // a 3 x 5 chroma plane at scale 2 and up to 16 bits: src_c 60 bytes, src_y 120; dst_y 480 bytes, dst_c 240 right behind it -- a frame
    alignas(16) static unsigned char buf[8192];
    void* sc = buf;
    void* sy = buf + 256;
    void* dy = buf + 2048;
    void* dc = buf + 2048 + 480;
#define CG(sc, sy, ds, h, w, dc, dy, dd, scale, loc, t) \
    moe_chroma_guided(sc, sy, ds, h, w, dc, dy, dd, scale, loc, (t).cx.data(), (t).ox.data(), (t).cy.data(), (t).oy.data(), (t).range.data(), 0, nullptr)
    const Tables t2(2);
    expect(CG(nullptr, sy, 10, 3, 5, dc, dy, 10, 2, 0, t2), MOE_EINVAL, "moe_chroma_guided: NULL", "src_c");
    expect(CG(sc, nullptr, 10, 3, 5, dc, dy, 10, 2, 0, t2), MOE_EINVAL, "NULL", "src_y");
    expect(CG(sc, sy, 10, 3, 5, nullptr, dy, 10, 2, 0, t2), MOE_EINVAL, "NULL", "dst_c");
    expect(CG(sc, sy, 10, 3, 5, dc, nullptr, 10, 2, 0, t2), MOE_EINVAL, "NULL", "dst_y");
    expect(moe_chroma_guided(sc, sy, 10, 3, 5, dc, dy, 10, 2, 0, nullptr, t2.ox.data(), t2.cy.data(), t2.oy.data(), t2.range.data(), 0, nullptr), MOE_EINVAL, "NULL", "cx");
    expect(moe_chroma_guided(sc, sy, 10, 3, 5, dc, dy, 10, 2, 0, t2.cx.data(), nullptr, t2.cy.data(), t2.oy.data(), t2.range.data(), 0, nullptr), MOE_EINVAL, "NULL", "ox");
    expect(moe_chroma_guided(sc, sy, 10, 3, 5, dc, dy, 10, 2, 0, t2.cx.data(), t2.ox.data(), nullptr, t2.oy.data(), t2.range.data(), 0, nullptr), MOE_EINVAL, "NULL", "cy");
    expect(moe_chroma_guided(sc, sy, 10, 3, 5, dc, dy, 10, 2, 0, t2.cx.data(), t2.ox.data(), t2.cy.data(), nullptr, t2.range.data(), 0, nullptr), MOE_EINVAL, "NULL", "oy");
    expect(moe_chroma_guided(sc, sy, 10, 3, 5, dc, dy, 10, 2, 0, t2.cx.data(), t2.ox.data(), t2.cy.data(), t2.oy.data(), nullptr, 0, nullptr), MOE_EINVAL, "NULL", "range64");
    const int depths[] = {-8, 0, 7, 9, 11, 14, 17, 32};
    for (int d : depths) {
        expect(CG(sc, sy, d, 3, 5, dc, dy, 10, 2, 0, t2), MOE_EINVAL, "depth", "src depth");
        expect(CG(sc, sy, 10, 3, 5, dc, dy, d, 2, 0, t2), MOE_EINVAL, "depth", "dst depth");
    }
    const int sizes[][2] = {{0, 5}, {3, 0}, {-1, 5}, {3, -7}, {0, 0}};
    for (auto& s : sizes) expect(CG(sc, sy, 10, s[0], s[1], dc, dy, 10, 2, 0, t2), MOE_EINVAL, "must be positive", "size");
    const int scales[] = {1, 0, -1, 17, 64};
    for (int s : scales) expect(CG(sc, sy, 10, 3, 5, dc, dy, 10, s, 0, t2), MOE_EINVAL, "scale", "scale");      // (refused before a table is read: t2 holds two phases only)
    expect(CG(sc, sy, 10, 1 << 29, 5, dc, dy, 10, 2, 0, t2), MOE_EINVAL, "does not fit", "2 h scale");
    expect(CG(sc, sy, 10, 3, 1 << 29, dc, dy, 10, 2, 0, t2), MOE_EINVAL, "does not fit", "2 w scale");
    const int locs[] = {-1, 2, 7};
    for (int l : locs) expect(CG(sc, sy, 10, 3, 5, dc, dy, 10, 2, l, t2), MOE_EINVAL, "loc", "loc");
    expect(CG(buf + 1, sy, 10, 3, 5, dc, dy, 10, 2, 0, t2), MOE_EINVAL, "src is not 2-byte aligned", "odd src_c at 10 bits");
    expect(CG(sc, buf + 257, 16, 3, 5, dc, dy, 8, 2, 0, t2), MOE_EINVAL, "src_y is not 2-byte aligned", "odd src_y at 16 bits");
    expect(CG(sc, sy, 10, 3, 5, buf + 2048 + 481, dy, 12, 2, 0, t2), MOE_EINVAL, "dst is not 2-byte aligned", "odd dst_c at 12 bits");
    expect(CG(buf + 1, buf + 257, 8, 3, 5, dc, buf + 2049, 16, 2, 1, t2), MOE_EINVAL, "dst_y is not 2-byte aligned", "odd sources are fine at 8 bits, an odd dst_y is not at 16");
    // tables: every scale's last phase spoilt on either axis (the walk reaches the last element of exact-size blocks)
    const int some_scales[] = {2, 3, 16};
    for (int scl : some_scales)
        for (int axis = 0; axis < 2; ++axis) {
            Tables t(scl);
            (axis ? t.cy : t.cx)[scl * 4 - 1] += 1;                      // the row sums to 257
            expect(CG(sc, sy, 8, 3, 5, dc, dy, 8, scl, 0, t), MOE_EINVAL, axis ? "vertical coefficients" : "horizontal coefficients", "row sum above");
            Tables u(scl);
            (axis ? u.cy : u.cx)[scl * 4 - 3] -= 1;                      // 255
            expect(CG(sc, sy, 8, 3, 5, dc, dy, 8, scl, 0, u), MOE_EINVAL, "sum to 255", "row sum below");
            Tables o(scl);
            (axis ? o.oy : o.ox)[scl - 1] = 2;
            expect(CG(sc, sy, 8, 3, 5, dc, dy, 8, scl, 0, o), MOE_EINVAL, axis ? "vertical offset 2" : "horizontal offset 2", "offset above 1");
            (axis ? o.oy : o.ox)[scl - 1] = -3;
            expect(CG(sc, sy, 8, 3, 5, dc, dy, 8, scl, 0, o), MOE_EINVAL, axis ? "vertical offset -3" : "horizontal offset -3", "offset below -2");
        }
    const int zeros[] = {0, 7, 63};
    for (int d : zeros) {
        Tables t(2);
        t.range[d] = 0;
        expect(CG(sc, sy, 10, 3, 5, dc, dy, 10, 2, 0, t), MOE_EINVAL, "is zero", "range weight");
    }
    // dst_c at the start of, inside, across the end of and across the start of the 480 bytes of dst_y
    const int overlaps[] = {0, 100, 478, -238};
    for (int at : overlaps) expect(CG(sc, sy, 10, 3, 5, buf + 2048 + at, dy, 10, 2, 0, t2), MOE_EINVAL, "overlaps", "dst_c over dst_y");
    if (n_bad) {
        fprintf(stderr, "chroma_guided_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("chroma_guided_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
