// ailut_args_check.cpp -- the refusals of moe_ailut_create / _num_params / _param_info / _set_param / _finalize / _run / _stage / _guards, moe_ailut_thumbnail and
// moe_lut3d_read (include/moephoto_amd.h), called from a stand-alone program so that the argument validation in ailut_api.cpp -- the walk over the caller's
// parameters included -- can run under the host sanitizers.  No device is touched: every call must return before its first HIP call.  The parameter blocks are heap
// blocks of exactly the announced size, so a read past either end is an AddressSanitizer report.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       ailut_api.cpp errors.cpp ../../tools/ailut_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/ailut_args_check
//   /tmp/ailut_args_check          (exit status 0 and "ailut_args_check: N refusals, all as declared")
//
// ailut_api.cpp and errors.cpp are compiled into the program with the sanitizers (the program's definitions win over the library's); the library only supplies the
// kernels' launchers those files refer to.  Not reached here: the device mismatch between generator and table handle, which needs a finalized generator.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
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

// the table handle's host object as csrc/net.h declares it: moe_ailut_run reads its d and device, and those reads must stay inside it
struct LutHost { int d, device; void* dev; size_t table_bytes; };

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- moe_ailut_create
    moe_ailut* g = nullptr;
    expect(moe_ailut_create(33, 3, nullptr), MOE_EINVAL, "moe_ailut_create: NULL", "handle");
    const int ds[] = {-1, 0, 1, 66, 1 << 20};
    for (int d : ds) expect(moe_ailut_create(d, 3, &g), MOE_EINVAL, "d = ", "d");
    const int rs[] = {-1, 0, 9, 1 << 20};
    for (int r : rs) expect(moe_ailut_create(33, r, &g), MOE_EINVAL, "ranks = ", "ranks");
    const int nets[][2] = {{2, 1}, {9, 3}, {33, 5}, {65, 8}};
    for (auto& net : nets) {
        const int d = net[0], ranks = net[1];
        if (moe_ailut_create(d, ranks, &g) != MOE_OK || !g) { fprintf(stderr, "create(%d, %d) failed: %s\n", d, ranks, moe_last_error()); return 1; }
        const int n = moe_ailut_num_params(g);
        if (n != 23) { fprintf(stderr, "num_params = %d\n", n); return 1; }
        const char* name = nullptr;
        int64_t shape[4] = {0, 0, 0, 0};
        int ndim = 0;
        // ---- moe_ailut_param_info
        expect(moe_ailut_param_info(nullptr, 0, &name, shape, &ndim), MOE_EINVAL, "moe_ailut_param_info: NULL", "info handle");
        expect(moe_ailut_param_info(g, 0, nullptr, shape, &ndim), MOE_EINVAL, "NULL", "info name");
        expect(moe_ailut_param_info(g, 0, &name, nullptr, &ndim), MOE_EINVAL, "NULL", "info shape");
        expect(moe_ailut_param_info(g, 0, &name, shape, nullptr), MOE_EINVAL, "NULL", "info ndim");
        expect(moe_ailut_param_info(g, -1, &name, shape, &ndim), MOE_EINVAL, "index -1", "info index below");
        expect(moe_ailut_param_info(g, n, &name, shape, &ndim), MOE_EINVAL, "index 23", "info index above");
        // ---- moe_ailut_finalize before anything is set, then with all but the last parameter
        expect(moe_ailut_finalize(nullptr, 0), MOE_EINVAL, "moe_ailut_finalize: NULL", "finalize handle");
        expect(moe_ailut_finalize(g, -1), MOE_EINVAL, "device -1", "finalize device");
        expect(moe_ailut_finalize(g, 0), MOE_ESTATE, "'backbone.0.0.weight' is not set", "finalize, nothing set");
        // ---- moe_ailut_set_param: every parameter as a heap block of exactly its size
        for (int i = 0; i < n; ++i) {
            if (moe_ailut_param_info(g, i, &name, shape, &ndim) != MOE_OK) { fprintf(stderr, "param_info(%d) failed\n", i); return 1; }
            int64_t numel = 1;
            for (int k = 0; k < ndim; ++k) numel *= shape[k];
            std::vector<float> data((size_t)numel, 0.25f);
            expect(moe_ailut_set_param(nullptr, name, data.data(), shape, ndim), MOE_EINVAL, "moe_ailut_set_param: NULL", "set handle");
            expect(moe_ailut_set_param(g, nullptr, data.data(), shape, ndim), MOE_EINVAL, "NULL", "set name");
            expect(moe_ailut_set_param(g, name, nullptr, shape, ndim), MOE_EINVAL, "NULL", "set data");
            expect(moe_ailut_set_param(g, name, data.data(), nullptr, ndim), MOE_EINVAL, "NULL", "set shape");
            expect(moe_ailut_set_param(g, (std::string(name) + "x").c_str(), data.data(), shape, ndim), MOE_EINVAL, "unknown parameter", "set unknown name");
            expect(moe_ailut_set_param(g, name, data.data(), shape, ndim - 1), MOE_EINVAL, "another shape", "set fewer dims");
            int64_t other[4] = {shape[0], shape[1], shape[2], shape[3]};
            other[ndim - 1] += 1;
            expect(moe_ailut_set_param(g, name, data.data(), other, ndim), MOE_EINVAL, "another shape", "set a longer last axis");
            const float bad[] = {inf, -inf, nan};
            for (float b : bad) {
                std::vector<float> last(data), first(data);
                last.back() = b;          // the last value of an exact-size block
                first[0] = b;
                expect(moe_ailut_set_param(g, name, last.data(), shape, ndim), MOE_EINVAL, "is not finite", "set not finite, last");
                expect(moe_ailut_set_param(g, name, first.data(), shape, ndim), MOE_EINVAL, "value 0 of", "set not finite, first");
            }
            if (i < n - 1 && moe_ailut_set_param(g, name, data.data(), shape, ndim) != MOE_OK) { fprintf(stderr, "set_param(%s) failed: %s\n", name, moe_last_error()); return 1; }
        }
        expect(moe_ailut_finalize(g, 0), MOE_ESTATE, "'adaint.intervals_generator.bias' is not set", "finalize, one unset");
        // ---- moe_ailut_run / moe_ailut_stage on the generator, which is not finalized: every argument check comes first
        alignas(16) static unsigned char buf[1024];
        void* src = buf + 512;
        LutHost same = {d, 0, nullptr, 0}, other = {d == 2 ? 3 : d - 1, 0, nullptr, 0};
        const moe_lut3d* lut = (const moe_lut3d*)&same;
#define RUN(gg, s, sb, H, W, o, l) moe_ailut_run(gg, s, sb, H, W, o, l, nullptr)
        expect(RUN(nullptr, src, 16, 4, 6, 0, lut), MOE_EINVAL, "moe_ailut_run: NULL", "run handle");
        expect(RUN(g, nullptr, 16, 4, 6, 0, lut), MOE_EINVAL, "NULL", "run src");
        expect(RUN(g, src, 16, 4, 6, 0, nullptr), MOE_EINVAL, "NULL", "run lut");
        const int src_bits[] = {-8, 0, 1, 10, 12, 24, 32};
        for (int b : src_bits) expect(RUN(g, src, b, 4, 6, 0, lut), MOE_EINVAL, "src_bits", "run src_bits");
        const int sizes[][2] = {{0, 6}, {4, 0}, {-2, 6}, {4, -6}, {0, 0}};
        for (auto& s : sizes) expect(RUN(g, src, 16, s[0], s[1], 0, lut), MOE_EINVAL, "must be positive", "run size");
        expect(RUN(g, src, 16, 1 << 15, 1 << 15, 0, lut), MOE_EINVAL, "do not fit an int", "run 3 H W");
        expect(RUN(g, src, 16, 1, 1 << 30, 0, lut), MOE_EINVAL, "do not fit an int", "run 3 H W, a long row");
        const int orders[] = {-1, 2, 7};
        for (int o : orders) expect(RUN(g, src, 16, 4, 6, o, lut), MOE_EINVAL, "order", "run order");
        expect(RUN(g, buf + 513, 16, 4, 6, 0, lut), MOE_EINVAL, "src is not 2-byte aligned", "run odd src at 16 bits");
        expect(RUN(g, src, 16, 4, 6, 0, (const moe_lut3d*)&other), MOE_EINVAL, "the table handle has d = ", "run another d");
        expect(RUN(g, buf + 513, 8, 4, 6, 1, lut), MOE_ESTATE, "not finalized", "run, not finalized (an odd src is fine at 8 bits)");
        expect(moe_ailut_stage(g, 0, src, 16, 4, 6, 0, lut, nullptr), MOE_ESTATE, "moe_ailut_stage: the generator is not finalized", "stage, not finalized");
        expect(moe_ailut_stage(g, 0, src, 12, 4, 6, 0, lut, nullptr), MOE_EINVAL, "moe_ailut_stage: src_bits", "stage src_bits");
        expect(moe_ailut_stage(nullptr, 0, src, 16, 4, 6, 0, lut, nullptr), MOE_EINVAL, "moe_ailut_stage: NULL", "stage handle");
        int64_t bad_bytes = 0;
        expect(moe_ailut_guards(nullptr, &bad_bytes, nullptr), MOE_EINVAL, "moe_ailut_guards: NULL", "guards handle");
        expect(moe_ailut_guards(g, nullptr, nullptr), MOE_EINVAL, "NULL", "guards count");
        expect(moe_ailut_guards(g, &bad_bytes, nullptr), MOE_ESTATE, "not finalized", "guards, not finalized");
        moe_ailut_destroy(g);
        g = nullptr;
    }
    expect(moe_ailut_num_params(nullptr), MOE_EINVAL, "moe_ailut_num_params: NULL", "num_params handle");
    moe_ailut_destroy(nullptr);          // (nothing to free: returns)
    // ---- moe_ailut_thumbnail
    alignas(16) static unsigned char buf[1024];
    void* src = buf + 512;
    float* dst = (float*)buf;
#define THUMB(s, sb, H, W, o, d) moe_ailut_thumbnail(s, sb, H, W, o, d, 0, nullptr)
    expect(THUMB(nullptr, 16, 4, 6, 0, dst), MOE_EINVAL, "moe_ailut_thumbnail: NULL", "thumbnail src");
    expect(THUMB(src, 16, 4, 6, 0, nullptr), MOE_EINVAL, "NULL", "thumbnail dst");
    expect(THUMB(src, 10, 4, 6, 0, dst), MOE_EINVAL, "src_bits", "thumbnail src_bits");
    expect(THUMB(src, 16, 0, 6, 0, dst), MOE_EINVAL, "must be positive", "thumbnail H");
    expect(THUMB(src, 16, 4, -1, 0, dst), MOE_EINVAL, "must be positive", "thumbnail W");
    expect(THUMB(src, 16, 1 << 15, 1 << 15, 0, dst), MOE_EINVAL, "do not fit an int", "thumbnail 3 H W");
    expect(THUMB(src, 16, 4, 6, 2, dst), MOE_EINVAL, "order", "thumbnail order");
    expect(THUMB(buf + 513, 16, 4, 6, 0, dst), MOE_EINVAL, "src is not 2-byte aligned", "thumbnail odd src");
    expect(THUMB(src, 8, 4, 6, 0, (float*)(buf + 2)), MOE_EINVAL, "dst is not 4-byte aligned", "thumbnail dst off 4 bytes");
    expect(moe_ailut_thumbnail(src, 16, 4, 6, 0, dst, -1, nullptr), MOE_EINVAL, "device -1", "thumbnail device");
    // ---- moe_lut3d_read
    LutHost h = {2, 0, nullptr, 128};
    float table[24], vert[6];
    expect(moe_lut3d_read(nullptr, table, vert, nullptr), MOE_EINVAL, "moe_lut3d_read: NULL", "read handle");
    expect(moe_lut3d_read((const moe_lut3d*)&h, nullptr, vert, nullptr), MOE_EINVAL, "NULL", "read table");
    expect(moe_lut3d_read((const moe_lut3d*)&h, table, nullptr, nullptr), MOE_EINVAL, "NULL", "read vertices");
    if (n_bad) {
        fprintf(stderr, "ailut_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("ailut_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
