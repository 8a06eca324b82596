// lut3d_args_check.cpp -- every refusal of moe_lut3d_create / moe_lut3d_run / moe_lut3d_info (include/moephoto_amd.h), called from a stand-alone program so that the
// argument validation in lut3d_api.cpp -- the walk over the caller's table and vertices included -- can run under the host sanitizers.  No device is touched: every
// call must return before its first HIP call.  The tables are heap blocks of exactly 3 d^3 and 3 d floats, so a read past either end is an AddressSanitizer report.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       lut3d_api.cpp errors.cpp ../../tools/lut3d_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/lut3d_args_check
//   /tmp/lut3d_args_check          (exit status 0 and "lut3d_args_check: N refusals, all as declared")
//
// lut3d_api.cpp and errors.cpp are compiled into the program with the sanitizers (the program's definitions win over the library's); the library only supplies the
// kernel's launcher those files refer to.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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

// A valid table of size d: the identity over uniform vertices, which the cases below then spoil.
struct Lut {
    int d;
    std::vector<float> table, vert;
    explicit Lut(int d_) : d(d_), table(3 * (size_t)d_ * d_ * d_), vert(3 * (size_t)d_)
    {
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < d; ++i) vert[c * d + i] = (float)i / (float)(d - 1);
        const size_t n = (size_t)d * d * d;
        for (size_t i = 0; i < n; ++i) {
            table[i] = vert[i % d]; table[n + i] = vert[d + (i / d) % d]; table[2 * n + i] = vert[2 * d + i / ((size_t)d * d)];
        }
    }
};

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    moe_lut3d* h = (moe_lut3d*)(uintptr_t)0x10;          // (every refusal comes before the handle is written or read)
    // ---- moe_lut3d_create
    {
        const Lut t(2);
        moe_lut3d* out = h;
        expect(moe_lut3d_create(2, nullptr, t.vert.data(), 0, &out), MOE_EINVAL, "moe_lut3d_create: NULL", "table");
        expect(moe_lut3d_create(2, t.table.data(), nullptr, 0, &out), MOE_EINVAL, "NULL", "vertices");
        expect(moe_lut3d_create(2, t.table.data(), t.vert.data(), 0, nullptr), MOE_EINVAL, "NULL", "handle");
        const int sizes[] = {-1, 0, 1, 66, 129, 1 << 20};
        for (int d : sizes) expect(moe_lut3d_create(d, t.table.data(), t.vert.data(), 0, &out), MOE_EINVAL, "d = ", "d");          // (refused before a table is read)
    }
    const int ds[] = {2, 5, 65};
    for (int d : ds) {
        moe_lut3d* out = nullptr;
        const float bad[] = {inf, -inf, nan};
        for (float b : bad) {
            Lut t(d);
            t.table.back() = b;                                        // the last value of an exact-size block
            expect(moe_lut3d_create(d, t.table.data(), t.vert.data(), 0, &out), MOE_EINVAL, "table value", "table not finite, last");
            Lut u(d);
            u.table[0] = b;
            expect(moe_lut3d_create(d, u.table.data(), u.vert.data(), 0, &out), MOE_EINVAL, "of channel 0 is not finite", "table not finite, first");
            Lut v(d);
            v.vert.back() = b;
            expect(moe_lut3d_create(d, v.table.data(), v.vert.data(), 0, &out), MOE_EINVAL, "of channel 2 is not finite", "vertex not finite, last");
            Lut w(d);
            w.vert[0] = b;
            expect(moe_lut3d_create(d, w.table.data(), w.vert.data(), 0, &out), MOE_EINVAL, "vertex 0 of channel 0 is not finite", "vertex not finite, first");
        }
        for (int c = 0; c < 3; ++c) {
            Lut t(d);
            t.vert[c * d + d - 1] = t.vert[c * d + d - 2] - 0.25f;      // the last vertex of a row below the one before it
            expect(moe_lut3d_create(d, t.table.data(), t.vert.data(), 0, &out), MOE_EINVAL, "decreases", "decreasing vertices");
        }
    }
    // ---- moe_lut3d_run: a 6 x 4 frame of 16-bit samples, src 144 bytes at buf + 512, dst 144 bytes at buf + 1024
    alignas(16) static unsigned char buf[4096];
    void* src = buf + 512;
    void* dst = buf + 1024;
#define RUN(hh, s, sb, H, W, d, bits, order, strength) moe_lut3d_run(hh, s, sb, H, W, d, bits, order, strength, nullptr)
    expect(RUN(nullptr, src, 16, 4, 6, dst, 16, 0, 1.f), MOE_EINVAL, "moe_lut3d_run: NULL", "handle");
    expect(RUN(h, nullptr, 16, 4, 6, dst, 16, 0, 1.f), MOE_EINVAL, "NULL", "src");
    expect(RUN(h, src, 16, 4, 6, nullptr, 16, 0, 1.f), MOE_EINVAL, "NULL", "dst");
    const int src_bits[] = {-8, 0, 1, 10, 12, 24, 32, 16 | MOE_Q_ROUND};
    for (int b : src_bits) expect(RUN(h, src, b, 4, 6, dst, 16, 0, 1.f), MOE_EINVAL, "src_bits", "src_bits");
    const int bits[] = {0, 1, 10, 12, 24, 32, MOE_Q_ORDERED, 255 | MOE_Q_ROUND};
    for (int b : bits) expect(RUN(h, src, 16, 4, 6, dst, b, 0, 1.f), MOE_EINVAL, "bits", "bits");
    expect(RUN(h, src, 16, 4, 6, dst, 16 | MOE_Q_UNIT, 0, 1.f), MOE_EINVAL, "MOE_Q_UNIT without", "unit scale alone");
    expect(RUN(h, src, 16, 4, 6, dst, 8 | MOE_Q_ROUND | MOE_Q_ORDERED, 0, 1.f), MOE_EINVAL, "both set", "two modes");
    expect(RUN(h, src, 16, 4, 6, dst, 8 | MOE_Q_ROUND | MOE_Q_ORDERED | MOE_Q_UNIT, 0, 1.f), MOE_EINVAL, "both set", "two modes at unit scale");
    expect(RUN(h, src, 16, 4, 6, dst, 16 | 0x800, 0, 1.f), MOE_EINVAL, "unknown flags", "another high bit");
    expect(RUN(h, src, 16, 4, 6, dst, -16, 0, 1.f), MOE_EINVAL, "unknown flags", "negative bits");
    const int sizes[][2] = {{0, 6}, {4, 0}, {-2, 6}, {4, -6}, {0, 0}};
    for (auto& s : sizes) expect(RUN(h, src, 16, s[0], s[1], dst, 16, 0, 1.f), MOE_EINVAL, "must be positive", "size");
    expect(RUN(h, src, 16, 1 << 15, 1 << 15, dst, 16, 0, 1.f), MOE_EINVAL, "do not fit an int", "3 H W");
    expect(RUN(h, src, 16, 1, 1 << 30, dst, 16, 0, 1.f), MOE_EINVAL, "do not fit an int", "3 H W, a long row");
    const int orders[] = {-1, 2, 7};
    for (int o : orders) expect(RUN(h, src, 16, 4, 6, dst, 16, o, 1.f), MOE_EINVAL, "order", "order");
    const float strengths[] = {inf, -inf, nan};
    for (float s : strengths) expect(RUN(h, src, 16, 4, 6, dst, 16, 0, s), MOE_EINVAL, "strength is not finite", "strength");
    expect(RUN(h, buf + 513, 16, 4, 6, dst, 16, 0, 1.f), MOE_EINVAL, "src is not 2-byte aligned", "odd src at 16 bits");
    expect(RUN(h, src, 16, 4, 6, buf + 1025, 16, 0, 1.f), MOE_EINVAL, "dst is not 2-byte aligned", "odd dst at 16 bits");
    expect(RUN(h, buf + 513, 8, 4, 6, buf + 1025, 16, 0, 1.f), MOE_EINVAL, "dst is not 2-byte aligned", "an odd src is fine at 8 bits, an odd dst is not at 16");
    // dst at the start of, inside, across the end of and across the start of the 144 bytes of src
    const int overlaps[] = {0, 10, 142, -142};
    for (int at : overlaps) expect(RUN(h, src, 16, 4, 6, buf + 512 + at, 16, 0, 1.f), MOE_EINVAL, "overlaps", "dst over src");
    expect(RUN(h, src, 8, 4, 6, buf + 512 + 71, 8, 0, 1.f), MOE_EINVAL, "overlaps", "dst over the last byte of an 8-bit src");
    // ---- moe_lut3d_info
    int64_t info[4];
    expect(moe_lut3d_info(nullptr, info), MOE_EINVAL, "moe_lut3d_info: NULL", "info handle");
    expect(moe_lut3d_info(h, nullptr), MOE_EINVAL, "NULL", "info block");
    moe_lut3d_destroy(nullptr);          // (nothing to free: returns)
    if (n_bad) {
        fprintf(stderr, "lut3d_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("lut3d_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
