// fit_px_args_check.cpp -- every refusal of moe_fit_create_px (include/moephoto_amd.h), called from a stand-alone program so that the argument validation in
// polyphase.cpp -- the walk over the caller's tables and the search for the tile, whose windows are counted in elements of interleaved pixels here -- can run under the
// host sanitizers.  No device is touched: every call must return before its first HIP call.  The tables are heap blocks of exactly m x taps / m elements, so a read
// past either end is an AddressSanitizer report.  (moe_fit_create's own refusals: tools/fit_args_check.cpp.)
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       polyphase.cpp errors.cpp ../../tools/fit_px_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/fit_px_args_check
//   /tmp/fit_px_args_check          (exit status 0 and "fit_px_args_check: N refusals, all as declared")
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
    if (rc != want || !msg || !strstr(msg, text) || !strstr(msg, "moe_fit_create_px")) {
        ++n_bad;
        fprintf(stderr, "%s: rc %d (want %d), message \"%s\" (want \"%s\" in it, and the entry point's name)\n", what, rc, want, msg ? msg : "(null)", text);
    }
}

// Valid tables of one call: per axis a unit tap in front of zeros at offset floor(o * n / m) -- nearest by index, which the cases below then spoil.
struct Tables {
    int64_t h, w, oh, ow;
    int tx, ty;
    std::vector<int16_t> cx, cy;
    std::vector<int32_t> ox, oy;
    Tables(int64_t h_, int64_t w_, int64_t oh_, int64_t ow_, int tx_, int ty_)
        : h(h_), w(w_), oh(oh_), ow(ow_), tx(tx_), ty(ty_), cx(ow_ * tx_, 0), cy(oh_ * ty_, 0), ox(ow_, 0), oy(oh_, 0)
    {
        for (int64_t o = 0; o < ow; ++o) { cx[o * tx] = 16384; ox[o] = (int32_t)(o * w / ow); }
        for (int64_t o = 0; o < oh; ++o) { cy[o * ty] = 16384; oy[o] = (int32_t)(o * h / oh); }
    }
};

static int create(const Tables& t, int channels = 3, int ds = 16, int dd = 8, moe_fit** out = nullptr)
{
    static moe_fit* sink;
    return moe_fit_create_px(channels, ds, t.h, t.w, dd, t.oh, t.ow, t.tx, t.cx.data(), t.ox.data(), t.ty, t.cy.data(), t.oy.data(), 0, out ? out : &sink);
}

int main()
{
    moe_fit* f = nullptr;
    const Tables t(6, 10, 4, 7, 2, 3);
    const int channels[] = {0, -1, 5, 64};
    for (int c : channels) expect(create(t, c), MOE_EINVAL, "channels (1 to 4)", "channels");
    // NULLs
    expect(moe_fit_create_px(3, 16, t.h, t.w, 8, t.oh, t.ow, t.tx, nullptr, t.ox.data(), t.ty, t.cy.data(), t.oy.data(), 0, &f), MOE_EINVAL, "NULL", "cx");
    expect(moe_fit_create_px(3, 16, t.h, t.w, 8, t.oh, t.ow, t.tx, t.cx.data(), nullptr, t.ty, t.cy.data(), t.oy.data(), 0, &f), MOE_EINVAL, "NULL", "ox");
    expect(moe_fit_create_px(3, 16, t.h, t.w, 8, t.oh, t.ow, t.tx, t.cx.data(), t.ox.data(), t.ty, nullptr, t.oy.data(), 0, &f), MOE_EINVAL, "NULL", "cy");
    expect(moe_fit_create_px(3, 16, t.h, t.w, 8, t.oh, t.ow, t.tx, t.cx.data(), t.ox.data(), t.ty, t.cy.data(), nullptr, 0, &f), MOE_EINVAL, "NULL", "oy");
    expect(moe_fit_create_px(3, 16, t.h, t.w, 8, t.oh, t.ow, t.tx, t.cx.data(), t.ox.data(), t.ty, t.cy.data(), t.oy.data(), 0, nullptr), MOE_EINVAL, "NULL", "handle");
    const int depths[] = {-8, 0, 7, 9, 11, 14, 17, 32};
    for (int d : depths) {
        expect(create(t, 3, d, 8), MOE_EINVAL, "depth", "src depth");
        expect(create(t, 3, 16, d), MOE_EINVAL, "depth", "dst depth");
    }
    {   // sizes: refused before a table is read (the tables hold the valid geometry's elements only)
        const int64_t bad[] = {0, -3, (int64_t)1 << 31, (int64_t)1 << 40};
        for (int64_t v : bad) {
            const char* text = v < 1 ? "must be positive" : "does not fit an int";
            Tables a = t; a.h = v; expect(create(a), MOE_EINVAL, text, "h");
            Tables b = t; b.w = v; expect(create(b), MOE_EINVAL, text, "w");
            Tables c = t; c.oh = v; expect(create(c), MOE_EINVAL, text, "oh");
            Tables d = t; d.ow = v; expect(create(d), MOE_EINVAL, text, "ow");
        }
        // pixels that fit an int in a row whose elements do not
        for (int c = 2; c <= 4; ++c) {
            Tables a = t; a.w = ((int64_t)1 << 31) / c + 1; expect(create(a, c), MOE_EINVAL, "channels does not fit an int", "w x channels");
            Tables b = t; b.ow = ((int64_t)1 << 31) / c + 1; expect(create(b, c), MOE_EINVAL, "channels does not fit an int", "ow x channels");
        }
    }
    const int taps[] = {0, -1, 17, 64};
    for (int n : taps) {
        Tables a = t; a.tx = n; expect(create(a), MOE_EINVAL, "taps", "taps_x");
        Tables b = t; b.ty = n; expect(create(b), MOE_EINVAL, "taps", "taps_y");
    }
    // tables: the last row of either axis spoilt, for several tap counts and every channel count (the walk reaches the last element of exact-size blocks)
    const int some_taps[] = {1, 2, 5, 16};
    for (int ch = 1; ch <= 4; ++ch)
        for (int tp : some_taps)
            for (int axis = 0; axis < 2; ++axis) {
                const char* const coefs = axis ? "vertical coefficients" : "horizontal coefficients";
                const char* const offset = axis ? "vertical offset" : "horizontal offset";
                Tables a(6, 10, 4, 7, tp, tp);
                (axis ? a.cy : a.cx).back() += 1;                                    // the row sums to 2^14 + 1
                expect(create(a, ch), MOE_EINVAL, coefs, "row sum");
                Tables b(6, 10, 4, 7, tp, tp);
                (axis ? b.oy : b.ox).back() = axis ? 6 : 10;                         // the first tap lies behind the image
                expect(create(b, ch), MOE_EINVAL, offset, "offset beyond n - 1");
                Tables c(6, 10, 4, 7, tp, tp);
                (axis ? c.oy : c.ox)[0] = -tp;                                       // the last tap lies in front of the image
                expect(create(c, ch), MOE_EINVAL, offset, "offset below 1 - taps");
                Tables d(6, 10, 4, 7, tp, tp);
                (axis ? d.oy : d.ox)[2] = 0;                                         // 0 behind 1
                expect(create(d, ch), MOE_EINVAL, "must not decrease", "offsets decrease");
            }
    {   // a row that sums to 2^14 with magnitudes beyond the int32 bound: 2 * 16385 + 2 * 8193 = 49156 > 32767
        const int16_t row[4] = {-8193, 16385, 16385, -8193};
        Tables a(6, 10, 4, 7, 4, 4);
        memcpy(&a.cx[4 * 6], row, sizeof(row));
        expect(create(a, 3, 16, 16), MOE_EINVAL, "magnitudes 49156", "magnitudes, horizontal");
        Tables b(6, 10, 4, 7, 4, 4);
        memcpy(&b.cy[0], row, sizeof(row));
        expect(create(b, 3, 16, 16), MOE_EINVAL, "vertical coefficients of output 0", "magnitudes, vertical");
    }
    // offsets that step too far: the window of a tile of 128 ELEMENTS does not fit the LDS.  Rows of 43 pixels: one tile at C = 1 .. 2, two at 3 (the edge inside
    // pixel 42) and at 4; the search walks every tile of every channel count over exact-size tables
    for (int ch = 1; ch <= 4; ++ch) {
        Tables a(1 << 16, 1 << 16, 43, 43, 1, 1);
        for (int o = 0; o < 43; ++o) a.ox[o] = a.oy[o] = o * 1024;
        expect(create(a, ch), MOE_EINVAL, "bytes of LDS", "window");
    }
    if (n_bad) {
        fprintf(stderr, "fit_px_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("fit_px_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
