// quant_args_check.cpp -- every refusal of the MOE_Q_* flags (include/moephoto_amd.h) in the thirteen entry points that take them, called from a stand-alone program
// so that the argument validation in plan_run.cpp can run under the host sanitizers.  No device is touched: every call must return before its first HIP call.
//
//   cd moephoto_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
//       plan_run.cpp planner.cpp errors.cpp ../../tools/quant_args_check.cpp -L.. -lmoephoto_amd -Wl,-rpath,$PWD/.. -fsanitize=address,undefined -o /tmp/quant_args_check
//   /tmp/quant_args_check          (exit status 0 and "quant_args_check: N refusals, all as declared")
//
// plan_run.cpp, planner.cpp and errors.cpp are compiled into the program with the sanitizers (the program's definitions win over the library's); the library only
// supplies the kernels' launchers those files refer to.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include "../include/moephoto_amd.h"

static int n_checked = 0, n_bad = 0;

static void expect(int rc, int want, const char* text, const char* none, const char* who, const char* what)
{
    ++n_checked;
    const char* msg = moe_last_error();
    if (rc != want || !msg || !strstr(msg, text) || !strstr(msg, who) || (none && strstr(msg, none))) {
        ++n_bad;
        fprintf(stderr, "%s, %s: rc %d (want %d), message \"%s\" (want \"%s\" in it%s%s)\n", who, what, rc, want, msg ? msg : "(null)", text, none ? ", not " : "", none ? none : "");
    }
}

int main()
{
    const int64_t grey[3] = {1, 100, 140}, rgb[3] = {3, 100, 140};
    moe_plan *p1 = nullptr, *p3 = nullptr, *q3 = nullptr;          // Y' at scale 2, three planes at scale 2, three planes at scale 1 (the DN step's)
    if (moe_plan_create(grey, 1e12, 1e-3, 5, 2, 8, 48, &p1) || moe_plan_create(rgb, 1e12, 1e-3, 5, 2, 8, 48, &p3) || moe_plan_create(rgb, 1e12, 1e-3, 5, 1, 8, 48, &q3)) {
        fprintf(stderr, "moe_plan_create: %s\n", moe_last_error());
        return 2;
    }
    moe_net* net = nullptr;
    if (moe_net_create(MOE_ARCH_NET2X, 2, &net)) {
        fprintf(stderr, "moe_net_create: %s\n", moe_last_error());
        return 2;
    }
    alignas(16) float buf[16] = {0};
    void* dst = buf;
    const int R = MOE_Q_ROUND, O = MOE_Q_ORDERED, U = MOE_Q_UNIT;
    auto out_dt = [](int b) { return (b & 0xff) ? MOE_U8 : MOE_F32; };          // (the canvas forms want the canvas dtype)
    struct Edge { const char* who; int low; bool yuv; std::function<int(int)> call; };
    const Edge edges[] = {
        {"moe_to_output", 8, false, [&](int b) { return moe_to_output(buf, MOE_F32, 2, 2, 1, b, dst, MOE_U8, 0, nullptr); }},
        {"moe_stitch_out", 8, false, [&](int b) { return moe_stitch_out(p3, 0, buf, nullptr, 3, MOE_F32, b, dst, MOE_U8, nullptr); }},
        {"moe_run_plan_out", 8, false, [&](int b) { return moe_run_plan_out(net, p3, buf, MOE_F32, 14000, 140, 1, MOE_F32, b, dst, MOE_U8, 0, nullptr); }},
        {"moe_stitch_mix", 8, false, [&](int b) { return moe_stitch_mix(q3, 0, buf, nullptr, 3, buf, MOE_F32, 14000, 140, 1, nullptr, 0, 0, 0.6, b, dst, out_dt(b), nullptr); }},
        {"moe_run_plan_filter", 8, false, [&](int b) { return moe_run_plan_filter(net, q3, buf, MOE_F32, 14000, 140, 1, nullptr, 0, 0, 0.6, b, dst, out_dt(b), 0, nullptr); }},
        {"moe_luma_merge", 8, false, [&](int b) { return moe_luma_merge(buf, MOE_F32, buf, 3, 2, 2, 0, 1, b, dst, out_dt(b), 0, nullptr); }},
        {"moe_stitch_luma", 8, false, [&](int b) { return moe_stitch_luma(p1, 0, buf, nullptr, 1, MOE_F32, buf, 0, 1, b, dst, out_dt(b), nullptr); }},
        {"moe_run_plan_luma", 8, false, [&](int b) { return moe_run_plan_luma(net, p1, buf, MOE_F32, 14000, 140, 1, buf, 0, 1, b, dst, out_dt(b), 0, nullptr); }},
        {"moe_stitch_planes", 10, false, [&](int d) { return moe_stitch_planes(p1, 0, buf, nullptr, 1, MOE_F32, d, dst, nullptr); }},
        {"moe_run_plan_planes", 10, false, [&](int d) { return moe_run_plan_planes(net, p1, buf, MOE_F32, 14000, 140, 1, MOE_F32, d, dst, 0, nullptr); }},
        {"moe_stitch_yuv", 10, true, [&](int d) { return moe_stitch_yuv(p3, 0, buf, nullptr, MOE_F32, d, 0, 0, dst, nullptr); }},
        {"moe_run_plan_yuv", 10, true, [&](int d) { return moe_run_plan_yuv(net, p3, buf, MOE_F32, 14000, 140, 1, MOE_F32, d, 0, 0, dst, 0, nullptr); }},
        {"moe_to_yuv", 10, true, [&](int d) { return moe_to_yuv(buf, MOE_F32, 2, 2, d, 0, 0, dst, 0, nullptr); }},
    };
    for (const Edge& e : edges) {
        expect(e.call(e.low | R | O), MOE_EINVAL, "both set", nullptr, e.who, "both modes");
        expect(e.call(e.low | R | O | U), MOE_EINVAL, "both set", nullptr, e.who, "both modes and the unit scale");
        expect(e.call(e.low | U), MOE_EINVAL, "MOE_Q_UNIT without", nullptr, e.who, "the unit scale without a mode");
        if (e.yuv) {
            expect(e.call(e.low | R | U), MOE_EINVAL, "MOE_Q_UNIT does not apply", nullptr, e.who, "the unit scale on the Y'CbCr edge, round");
            expect(e.call(e.low | O | U), MOE_EINVAL, "MOE_Q_UNIT does not apply", nullptr, e.who, "the unit scale on the Y'CbCr edge, ordered");
        }
        const int flagses[] = {R, O, R | U, O | U};
        for (int f : flagses)
            if (!(e.yuv && (f & U))) expect(e.call(0 | f), MOE_EINVAL, "beside bits = 0", nullptr, e.who, "a flag beside bits = 0");
        const int highs[] = {0x800, 0x1000, 0x8000, 0x10000, 1 << 30, (int)0x80000000u};
        for (int h : highs) {          // any other high bit: the unknown bits / depth it always was, whatever known flags stand beside it
            expect(e.call(e.low | h), MOE_EINVAL, e.who, "MOE_Q", e.who, "another high bit");
            expect(e.call(e.low | h | O), MOE_EINVAL, e.who, "MOE_Q", e.who, "another high bit beside a mode");
        }
        if (strcmp(e.who, "moe_to_output")) expect(e.call(3 | O), MOE_EINVAL, e.who, "MOE_Q", e.who, "the low byte keeps its check");
    }
    // moe_to_output takes any bits from 1 to 16: its own low-byte refusals
    expect(moe_to_output(buf, MOE_F32, 2, 2, 1, 17 | R, dst, MOE_U16, 0, nullptr), MOE_EINVAL, "bad argument", nullptr, "moe_to_output", "17 bits beside a mode");
    expect(moe_to_output(buf, MOE_F32, 2, 2, 1, 16 | O | U, dst, MOE_U8, 0, nullptr), MOE_EINVAL, "do not fit MOE_U8", nullptr, "moe_to_output", "16 bits in bytes beside flags");
    // a flagged call that is otherwise complete passes every argument check: the run_plan forms reach the unfinalised net
    expect(moe_run_plan_out(net, p3, buf, MOE_F32, 14000, 140, 1, MOE_F32, 8 | O | U, dst, MOE_U8, 0, nullptr), MOE_ESTATE, "net is not finalized", nullptr, "moe_run_plan_out", "complete");
    expect(moe_run_plan_planes(net, p1, buf, MOE_F32, 14000, 140, 1, MOE_F32, 12 | R | U, dst, 0, nullptr), MOE_ESTATE, "net is not finalized", nullptr, "moe_run_plan_planes", "complete");
    expect(moe_run_plan_yuv(net, p3, buf, MOE_F32, 14000, 140, 1, MOE_F32, 8 | O, 0, 0, dst, 0, nullptr), MOE_ESTATE, "net is not finalized", nullptr, "moe_run_plan_yuv", "complete");
    expect(moe_run_plan_filter(net, q3, buf, MOE_F32, 14000, 140, 1, nullptr, 0, 0, 0.6, 16 | R, dst, MOE_U16, 0, nullptr), MOE_ESTATE, "net is not finalized", nullptr, "moe_run_plan_filter", "complete");
    expect(moe_run_plan_luma(net, p1, buf, MOE_F32, 14000, 140, 1, buf, 0, 1, 8 | R | U, dst, MOE_U8, 0, nullptr), MOE_ESTATE, "net is not finalized", nullptr, "moe_run_plan_luma", "complete");
    // the integer polyphase kernels take no flags: such values stay unknown depths
    const int16_t cx[2] = {16384, 16384};
    const int8_t ox[2] = {0, 0};
    expect(moe_chroma_resample(buf, 8 | R, 2, 2, dst, 8, 2, 1, cx, ox, cx, ox, 0, nullptr), MOE_EINVAL, "depth", "MOE_Q", "moe_chroma_resample", "a flagged source depth");
    expect(moe_chroma_resample(buf, 8, 2, 2, dst, 8 | O, 2, 1, cx, ox, cx, ox, 0, nullptr), MOE_EINVAL, "depth", "MOE_Q", "moe_chroma_resample", "a flagged destination depth");
    const int32_t fo[2] = {0, 1};
    moe_fit* fit = nullptr;
    expect(moe_fit_create(1, 8, 2, 2, 8 | O, 2, 2, 1, cx, fo, 1, cx, fo, 0, &fit), MOE_EINVAL, "depth", "MOE_Q", "moe_fit_create", "a flagged destination depth");
    moe_net_destroy(net);
    moe_plan_destroy(p1);
    moe_plan_destroy(p3);
    moe_plan_destroy(q3);
    if (n_bad) {
        fprintf(stderr, "quant_args_check: %d of %d refusals differ\n", n_bad, n_checked);
        return 1;
    }
    printf("quant_args_check: %d refusals, all as declared\n", n_checked);
    return 0;
}
