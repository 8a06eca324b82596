// reuse_args_check.cpp -- every refusal of moe_changed_blocks and moe_run_plan_subset (include/moephoto_amd.h), called from a stand-alone program so that the argument
// validation in plan_run.cpp can run under the host sanitizers.  No device is touched: every call must return before its first HIP call.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       plan_run.cpp planner.cpp errors.cpp ../../tools/reuse_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/reuse_args_check
//   /tmp/reuse_args_check          (exit status 0 and "reuse_args_check: N refusals, all as declared")
//
// plan_run.cpp, planner.cpp and errors.cpp are compiled into the program with the sanitizers (the program's definitions win over the library's); the library only
// supplies the kernels' launchers those files refer to.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

int main()
{
    alignas(16) static uint8_t buf[4096] = {0};
    uint8_t *cur = buf, *prev = buf + 1024, *map = buf + 2048;
#define CB(c, p, n, rows, rb, br, bb, m) moe_changed_blocks(c, p, n, rows, rb, br, bb, m, 0, nullptr)
    expect(CB(nullptr, prev, 1, 4, 16, 2, 8, map), MOE_EINVAL, "moe_changed_blocks: NULL", "map: cur");
    expect(CB(cur, nullptr, 1, 4, 16, 2, 8, map), MOE_EINVAL, "NULL", "map: prev");
    expect(CB(cur, prev, 1, 4, 16, 2, 8, nullptr), MOE_EINVAL, "NULL", "map: map");
    const int bad[] = {0, -1, -2147483647 - 1};
    for (int v : bad) {
        expect(CB(cur, prev, v, 4, 16, 2, 8, map), MOE_EINVAL, "must be 1 at least", "map: n");
        expect(CB(cur, prev, 1, v, 16, 2, 8, map), MOE_EINVAL, "must be 1 at least", "map: rows");
        expect(CB(cur, prev, 1, 4, (int64_t)v, 2, 8, map), MOE_EINVAL, "must be 1 at least", "map: row_bytes");
        expect(CB(cur, prev, 1, 4, 16, v, 8, map), MOE_EINVAL, "blocks of", "map: block_rows");
        expect(CB(cur, prev, 1, 4, 16, 2, v, map), MOE_EINVAL, "blocks of", "map: block_bytes");
    }
    expect(CB(cur, prev, 1, 4, INT64_MIN, 2, 8, map), MOE_EINVAL, "must be 1 at least", "map: row_bytes at INT64_MIN");
    expect(CB(cur, cur, 1, 4, 16, 2, 8, map), MOE_EINVAL, "same buffer", "map: cur == prev");
    expect(CB(cur, cur + 63, 1, 4, 16, 2, 8, map), MOE_EINVAL, "overlap", "map: prev inside cur's last byte");
    expect(CB(cur + 63, cur, 1, 4, 16, 2, 8, map), MOE_EINVAL, "overlap", "map: cur inside prev's last byte");
    expect(CB(cur, cur + 1, 1, 4, 16, 2, 8, map), MOE_EINVAL, "overlap", "map: one byte apart");
    expect(CB(cur, cur + 127, 2, 4, 16, 2, 8, map), MOE_EINVAL, "overlap", "map: two matrices, 127 bytes apart");
    expect(CB(cur, prev, 1, 1, INT64_MAX, 2, 8, map), MOE_EINVAL, "overlap", "map: one row of 2^63 - 1 bytes");
    expect(CB(cur, prev, 2147483647, 2147483647, INT64_MAX, 2, 8, map), MOE_EINVAL, "63 bits", "map: a size past 63 bits");
    expect(CB(cur, prev, 1 << 30, 1 << 30, (int64_t)1 << 40, 2, 8, map), MOE_EINVAL, "63 bits", "map: a size past 63 bits (2^100)");
    expect(CB(cur, (uint8_t*)((uintptr_t)cur + ((uintptr_t)1 << 45)), 1, 1 << 20, (int64_t)1 << 20, 1, 1, map), MOE_EINVAL, "cells", "map: 2^40 cells");

    const int64_t rgb[3] = {3, 100, 140};
    moe_plan* p2 = nullptr;
    if (moe_plan_create(rgb, 1e12, 1e-3, 5, 2, 8, 48, &p2)) {
        fprintf(stderr, "moe_plan_create: %s\n", moe_last_error());
        return 2;
    }
    moe_net* net = nullptr;
    if (moe_net_create(MOE_ARCH_NET2X, 2, &net)) {
        fprintf(stderr, "moe_net_create: %s\n", moe_last_error());
        return 2;
    }
    alignas(16) static float img[16] = {0};
    static uint8_t run[64] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    float* pool = img;
#define RS(n, pl, im, r, po) moe_run_plan_subset(n, pl, im, MOE_F32, 14000, 140, 1, r, po, 0, nullptr)
    expect(RS(nullptr, p2, img, run, pool), MOE_EINVAL, "moe_run_plan_subset: NULL", "subset: net");
    expect(RS(net, nullptr, img, run, pool), MOE_EINVAL, "NULL", "subset: plan");
    expect(RS(net, p2, nullptr, run, pool), MOE_EINVAL, "NULL", "subset: img");
    expect(RS(net, p2, img, nullptr, pool), MOE_EINVAL, "NULL", "subset: run");
    expect(RS(net, p2, img, run, nullptr), MOE_EINVAL, "NULL", "subset: pool");
    expect(RS(net, p2, img, run, pool), MOE_ESTATE, "moe_run_plan_subset: net is not finalized", "subset: net state");
    memset(run, 0, sizeof run);
    expect(RS(net, p2, img, run, pool), MOE_ESTATE, "net is not finalized", "subset: net state with an empty mask");
    moe_net_destroy(net);
    moe_plan_destroy(p2);
    if (n_bad) {
        fprintf(stderr, "reuse_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("reuse_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
