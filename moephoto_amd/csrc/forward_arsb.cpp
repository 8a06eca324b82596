// forward_arsb.cpp -- the forward of the ARSB nets: Net2x / Net3x / Net4x (python/models.py:108-160: stem, conv_input2, six ARSBs, two upsampler branches and their
// sum) and NetDN (the same trunk, no upsamplers).  The paragraphs of the sequence -- the form of the fused tail, one upsampler branch, the trunk, the branch sum --
// are the member functions of ArsbRun below; ArsbRun::run is the sequence itself, with the fork / join of the U branch in its one scope.
#include "net.h"

using namespace moe;

namespace {

// the last up-conv layer of branch br (0: R = convt_R1, on the trunk output; 1: U = u, on the stem output); nullptr: the net has none
const ConvLayer* last_up(const moe_net& n, int br)
{
    const auto it = n.conv_index.find(std::string(br == 0 ? "convt_R1" : "u") + ".up" + std::to_string(n.stages - 1));
    return it == n.conv_index.end() ? nullptr : &n.convs[it->second];
}

bool can_fuse_tail(const moe_net& n, const Fwd& f)
{
    const int B = f.B, h = f.h, w = f.w;
    if (!n.opt.fuse_tail || f.x3 || f.direct || n.debug || n.opt.conv_impl != 2 || n.stages < 1) return false;
    if (!(n.arch == MOE_ARCH_NET2X || n.arch == MOE_ARCH_NET3X || n.arch == MOE_ARCH_NET4X)) return false;
    if (sp_bytes_per_pixel(n) * B * h * w > kSpRange) return false;    // (forward_dev keeps every launch set inside this range)
    int hl = h, wl = w;
    for (int st = 0; st + 1 < n.stages; ++st) { hl *= n.r; wl *= n.r; }
    for (int br = 0; br < 2; ++br) {      // the nine-tap-planes form of conv3x3_sp takes both branches' last up-conv (the other forms are chosen among by plan_tail_form)
        const ConvLayer* L = last_up(n, br);
        if (!L) return false;
        ConvForm c = f.form(*L, hl, wl);
        c.tail = true;
        if (!conv3x3_sp_applicable(c)) return false;
    }
    return true;
}

// one forward: what its paragraphs share
struct ArsbRun {
    const moe_net& n;
    Fwd& f;
    const int B, h, w;
    bool mixed = false;                  // MIXED: the stem output and the trunk stream as hi + lo pairs
    int nx = 0;                          // ... and the leading ARSBs that run with split operands
    Act A, Bb, Cc;                       // the stem's output; the trunk stream and its scratch
    bool chain8 = false;                 // the split-operand chain passes its low parts as fp8 words (see run)
    half_t* lo16x = nullptr;
    bool sr = false, fuse = false, ps4 = false, ps9 = false;      // the form of the branches' last stage (plan_tail_form)
    int H = 0, W = 0;                    // resolution behind the stages a branch has run
    Act fin[2];
    float* tp[2] = {nullptr, nullptr};
    float* ps_plane[2] = {nullptr, nullptr};
    float* ps_apron[2] = {nullptr, nullptr};

    void plan_tail_form();
    template <typename Args, typename Launch>
    int ps_stage(int br, const std::string& key, const Act& cur, size_t plane_bytes, size_t apron_bytes, const char* name, Launch launch);
    int run_branch(int br, Act cur);
    int trunk_conv(const std::string& key, const Act& in, const Act& out, const Act* res, bool exact);
    int run_trunk();
    template <typename Args, typename Launch> void tail_add(Launch launch);
    int branch_sum();
    int run();
};

// ---- the two upsampler branches: R on the trunk output, U on the stem output (models.py:117-123) -- planned before the trunk runs, because a small launch set starts its U branch first, on a second stream ----
void ArsbRun::plan_tail_form()
{
    sr = n.arch != MOE_ARCH_NETDN;
    fuse = sr && can_fuse_tail(n, f);      // last upsampler conv + 64->1 tail conv in one kernel
    if (sr) {   // form of the fused tail's output: phase-class sums when the last stage is a x2 shuffle the register-weight kernel takes
        int hl = h, wl = w;
        for (int st = 0; st + 1 < n.stages; ++st) { hl *= n.r; wl *= n.r; }
        bool ok = fuse && n.opt.tail_form == 1;
        bool ps4_ok = true;
        bool ps9_ok = true;
        for (int br = 0; br < 2; ++br) {
            const ConvLayer* L = last_up(n, br);
            if (ok) {      // (fuse: both layers exist) conv3x3_rw's own predicate for its phase-class-sums epilogue
                ConvForm c = f.form(*L, hl, wl);
                c.tail = true; c.tail_form = 1;
                ok = conv3x3_rw_applicable(c);
            }
            ps4_ok = ps4_ok && L && ps4_tail_applicable(B, hl, wl, L->slope);      // (the launcher's own predicate: common.h)
            ps9_ok = ps9_ok && L && ps9_tail_applicable(B, hl, wl, L->slope);
        }
        f.tail_form = ok ? 1 : 0;
        // the same layer with all four phases in one workgroup (conv3x3_ps4.hip): one fp32 plane + column aprons per branch, added by tailadd
        ps4 = ok && n.opt.up_impl == 1 && ps4_ok && (2 * wl) % 8 == 0;
        // x3 nets: the phase-row form of the same kernel (conv3x3_ps9.hip): three fp32 planes S[dy] + column aprons per branch, added by tailadd3
        ps9 = fuse && n.opt.up_impl == 1 && n.r == 3 && f.groups >= 3 && ps9_ok;
    }
}

// the last stage of a branch with the tail conv fused, all phases in one workgroup (conv3x3_ps4.hip for x2, conv3x3_ps9.hip for x3): plane + aprons per branch
template <typename Args, typename Launch>
int ArsbRun::ps_stage(int br, const std::string& key, const Act& cur, size_t plane_bytes, size_t apron_bytes, const char* name, Launch launch)
{
    ps_plane[br] = (float*)f.ar.take(plane_bytes + 4096);
    ps_apron[br] = (float*)f.ar.take(apron_bytes + 4096);
    if (!f.dry()) {
        const ConvLayer& L = n.convs[n.conv_index.at(key)];
        Args q{};
        q.in = cur.hi; q.wpk = f.blob<half_t>(L.w_hi); q.bias = L.has_bias ? f.blob<float>(L.bias) : f.small<float>("zero_bias");
        q.tail_w = f.small<half_t>(br == 0 ? "tail_r.frag" : "tail_u.frag");
        q.plane = ps_plane[br]; q.apron = ps_apron[br]; q.slope = L.slope; q.B = B; q.H = H; q.W = W;
        q.split = (f.mixed && f.tail_split_for(key)) ? 1 : 0;
        const int rec = f.prof_begin(key, 2.0 * (double)B * H * W * L.cout * L.cin * L.taps);
        bool done = false;
        for (int rep = f.repeats(key); rep > 0; --rep) done = launch(q, f.groups, f.s);
        f.prof_end(rec);
        if (!done) return fail(MOE_EINVAL, "fused tail kernel (%s) rejected layer %s", name, key.c_str());
    }
    H *= n.r; W *= n.r;
    return (int)MOE_OK;
}

int ArsbRun::run_branch(int br, Act cur)      // launches go to f.s (the caller's stream, or the side stream while the U branch is forked)
{
    if (f.mixed) { cur.drop_lo(); cur.lo8 = false; }      // MIXED: the upsampler convs take the fp16 parts (FP16X3 keeps its pairs)
    H = h; W = w;
    for (int st = 0; st < n.stages; ++st) {
        const std::string key = std::string(br == 0 ? "convt_R1" : "u") + ".up" + std::to_string(st);
        if (ps4 && st == n.stages - 1) {
            if (int rc = ps_stage<Ps4Args>(br, key, cur, ps4_plane_bytes(B, H, W), ps4_apron_bytes(B, H, W), "ps4", launch_conv3x3_ps4)) return rc;
            continue;
        }
        if (ps9 && st == n.stages - 1) {
            if (int rc = ps_stage<Ps9Args>(br, key, cur, ps9_plane_bytes(B, H, W), ps9_apron_bytes(B, H, W), "ps9", launch_conv3x3_ps9)) return rc;
            continue;
        }
        if (fuse && st == n.stages - 1) {
            tp[br] = (float*)f.ar.take(f.tail_form == 1 ? (size_t)tailsum_layout(B, H, W).total * 4 + 4096 : (size_t)9 * B * H * n.r * W * n.r * 4 + 4096);
            ConvExtra tail;
            tail.fuse_tail = true; tail.tail_w = f.small<half_t>(br == 0 ? "tail_r.frag" : "tail_u.frag"); tail.tplanes = tp[br];
            if (!f.conv(key, cur, Act{}, nullptr, H, W, tail))
                return fail(MOE_EINVAL, "fused tail kernel rejected layer %s", key.c_str());
            H *= n.r; W *= n.r;
            continue;
        }
        Act nxt = f.act((long long)B * H * n.r * W * n.r);
        f.conv(key, cur, nxt, nullptr, H, W);
        H *= n.r; W *= n.r;
        f.tap(std::string(br == 0 ? "r" : "u") + ".up" + std::to_string(st), nxt, H, W, 64, 64);
        cur = nxt;
    }
    fin[br] = cur;
    return (int)MOE_OK;
}

int ArsbRun::trunk_conv(const std::string& key, const Act& in, const Act& out, const Act* res, bool exact)
{
    ConvExtra e;
    e.exact = exact;
    if (!f.conv(key, in, out, res, h, w, e))
        return fail(MOE_EINVAL, "layer %s: %d planes of %dx%d exceed the conv kernel's addressing range (use smaller tiles)", key.c_str(), B, h, w);
    return (int)MOE_OK;
}

// conv_input2 and the six ARSBs: A -> Bb
int ArsbRun::run_trunk()
{
    if (int rc = trunk_conv("input2", A, Bb, nullptr, mixed)) return rc;
    f.tap("input2", Bb, h, w, 64, n.C);
    // single-pass ARSBs run as ONE kernel (arsb32c.hip: conv_1's output never leaves the CU) that streams cur -> oth;
    // split-operand / debug blocks use the two-launch form, conv_1 into `oth`, conv_2 back onto `cur`
    const bool arsb_fuse = n.opt.arsb_fuse && !f.x3 && !f.direct && n.opt.conv_impl == 2;
    hipStream_t s = f.s;
    Act cur = Bb, oth = Cc;
    for (int i = 1; i <= 6; ++i) {
        const bool ex = mixed && i <= nx;
        const std::string k1 = "c1_" + std::to_string(i), k2 = "c2_" + std::to_string(i);
        const ConvLayer& L1 = n.convs[n.conv_index.at(k1)];
        const ConvLayer& L2 = n.convs[n.conv_index.at(k2)];
        const bool trunk64 = L1.w_arsb != 0;      // a bias-free 64 -> 64 trunk conv (weights.cpp packs w_arsb for exactly those)
        const int cin = (L1.cin == 48 && L2.cin == 48 && n.opt.k48) ? 48 : 64;      // NetDN: channels 48..63 are zeros in activations and weights
        const bool drop6 = mixed && i == 6 && n.arch != MOE_ARCH_NETDN && !n.debug;      // the upsamplers take the fp16 part: nobody reads block 6's low part (arsb32c's drop_lo)
        if (arsb_fuse && !ex && (!mixed || (cur.has_lo && oth.has_lo)) && trunk64 && arsb32c_applicable(B, h, w, L1.slope, mixed, mixed, cin)) {
            if (!f.dry()) {
                ArsbArgs q{};
                q.x_hi = cur.hi; q.x_lo = mixed ? cur.lo : nullptr; q.y_hi = oth.hi; q.y_lo = mixed ? oth.lo : nullptr;
                q.w1 = f.blob<half_t>(L1.w_hi); q.w2 = f.blob<half_t>(L2.w_hi); q.zero = f.small<half_t>("zero");      // (pack_conv order; conv_2's carry the ScaleLayer factor as well)
                q.slope = L1.slope; q.B = B; q.H = h; q.W = w; q.cin = cin;
                q.drop_lo = drop6 ? 1 : 0;
                const bool trace = n.opt.arsb_trace;   // MOE_ARSB_TRACE with a -DARSB_TRACE build: stamps of ARSB 3 -> /tmp/arsb_trace.bin
                const size_t tb = 8 * 16 * 4 * 40 * 8;
                if (trace && i == 3 && hipMalloc((void**)&q.trace, tb) == hipSuccess) (void)hipMemsetAsync(q.trace, 0, tb, s);
                const int rec = f.prof_begin("arsb" + std::to_string(i), 2.0 * 2.0 * (double)B * h * w * L1.cout * L1.cin * 9);
                bool done = false;
                for (int rep = f.repeats("arsb" + std::to_string(i)); rep > 0; --rep) done = launch_arsb32c(q, f.groups, s);
                f.prof_end(rec);
                if (q.trace) {
                    std::vector<unsigned long long> host(tb / 8);
                    (void)hipStreamSynchronize(s);
                    (void)hipMemcpy(host.data(), q.trace, tb, hipMemcpyDeviceToHost);
                    if (FILE* fp = fopen("/tmp/arsb_trace.bin", "wb")) { fwrite(host.data(), 1, tb, fp); fclose(fp); }
                    (void)hipFree(q.trace);
                }
                if (!done) return fail(MOE_EINVAL, "internal error: arsb32c rejected layer %s its predicate took", k1.c_str());
            }
            std::swap(cur, oth); cur.lo8 = oth.lo8 = false;      // (fp16 low parts out; the scratch side's form is its next writer's)
            Act seen = cur;
            if (drop6) seen.drop_lo();      // (cur.lo still points at the bytes block 6 did not write: the tap is the fp16 part alone)
            f.tap("arsb" + std::to_string(i), seen, h, w, 64, n.C);
            continue;
        }
        if (ex && chain8 && n.opt.exact_fuse && n.opt.q8_impl == 1 && cur.lo8 && cur.has_lo && oth.has_lo && L1.wq_hi8 && L2.wq_hi8 && !L1.has_bias && !L2.has_bias && L2.slope == 1.f &&
            arsb_sq_applicable(B, h, w, L1.slope)) {
            // an exact block of the chain in ONE launch (arsb_sq.hip): x = cur (fp16 + fp8 low words) -> oth; the last exact block writes fp16 low parts (the
            // single-pass ARSB kernels behind it read those)
            if (!f.dry()) {
                ArsbSqArgs q{};
                q.x_hi = cur.hi; q.x_lo8 = (const unsigned char*)cur.lo; q.y_hi = oth.hi; q.y_lo = oth.lo;
                q.w16[0] = f.blob<half_t>(L1.w_hi); q.wh8[0] = f.blob<unsigned char>(L1.wq_hi8); q.wl8[0] = f.blob<unsigned char>(L1.wq_lo8);
                q.w16[1] = f.blob<half_t>(L2.w_hi); q.wh8[1] = f.blob<unsigned char>(L2.wq_hi8); q.wl8[1] = f.blob<unsigned char>(L2.wq_lo8);
                q.slope = L1.slope; q.B = B; q.H = h; q.W = w; q.out8 = i < nx;
                const int rec = f.prof_begin("xpair" + std::to_string(i), 2.0 * 2.0 * 3.0 * (double)B * h * w * L1.cout * L1.cin * 9);
                const bool done = launch_arsb_sq(q, f.groups, s);
                f.prof_end(rec);
                if (!done) return fail(MOE_EINVAL, "internal error: arsb_sq rejected layer %s its predicate took", k1.c_str());
            }
            std::swap(cur, oth);
            cur.lo8 = i < nx;
            oth.lo8 = false;             // (scratch now: whoever writes it next decides its form)
            f.tap("arsb" + std::to_string(i), cur, h, w, 64, n.C);
            continue;
        }
        Act m = oth;
        if (mixed && !ex) m.drop_lo();                       // single-pass ARSB: conv_1's output is an fp16 operand only
        m.lo8 = ex && chain8;
        Act bin = cur;
        if (mixed && !ex) bin.drop_lo();
        if (int rc = trunk_conv(k1, bin, m, nullptr, ex)) return rc;
        const Act resid = cur;
        if (ex && chain8 && i == nx) { cur.lo = lo16x ? lo16x : A.lo; cur.lo8 = false; }      // (see chain8: a low part either way)
        if (int rc = trunk_conv(k2, m, cur, &resid, ex)) return rc;
        f.tap("arsb" + std::to_string(i), cur, h, w, 64, n.C);
    }
    Bb = cur;
    return (int)MOE_OK;
}

// the sum of the two branches' fused tails (conv3x3_ps4 -> tailadd, conv3x3_ps9 -> tailadd3): plane + aprons of R and U -> y
template <typename Args, typename Launch>
void ArsbRun::tail_add(Launch launch)
{
    if (f.dry()) return;
    Args t{};
    t.p0 = ps_plane[0]; t.p1 = ps_plane[1]; t.a0 = ps_apron[0]; t.a1 = ps_apron[1];
    t.y = f.io.y; t.y_dtype = f.io.y_dtype; t.y_off = f.io.y_off; t.B = B; t.H = H; t.W = W; t.px = (W / n.r + kTileW - 1) / kTileW;
    t.vec_ok = f.y_vec;
    const int rec = f.prof_begin("tailadd", 0.0);
    f.gate();
    launch(t, f.s);
    f.prof_end(rec);
}

int ArsbRun::branch_sum()
{
    if (ps4) { tail_add<TailAddArgs>(launch_tailadd); return MOE_OK; }
    if (ps9) { tail_add<TailAdd3Args>(launch_tailadd3); return MOE_OK; }
    if (fuse) {
        if (!f.dry()) {
            TapSumArgs t{};
            t.t0 = tp[0]; t.t1 = tp[1]; t.y = f.io.y; t.y_dtype = f.io.y_dtype; t.y_off = f.io.y_off; t.B = B; t.H = H; t.W = W; t.r = n.r;
            t.form = f.tail_form;
            t.vec_ok = n.r == 2 && f.y_vec && W % 8 == 0;
            f.gate();
            launch_tapsum(t, f.s);
        }
        return MOE_OK;
    }
    f.tail(&fin[0], &fin[1], H, W, false);
    return MOE_OK;
}

int ArsbRun::run()
{
    const long long P = (long long)B * h * w;
    hipStream_t s = f.s;
    // MIXED (the default of these nets): the stem output and the trunk stream are kept as hi + lo pairs; conv_input2 and the first
    // `nx` ARSBs run with split operands (three products, ~fp32), the others with fp16 operands and the fp32-equivalent residual
    // add (see Fwd::conv).  DESIGN.md section 5 has the error budget behind this choice.
    mixed = f.mixed;
    nx = mixed ? exact_blocks_of(n) : 0;
    f.drop_taps();      // (the tapped forms leave different taps -- value 1 stores every upsampler stage, value 2 the production form's: none of another forward's stays behind)
    A = f.act(P, 64, mixed); Bb = f.act(P, 64, mixed); Cc = f.act(P, 64, mixed);
    if (mixed && n.opt.conv_impl != 2)
        return fail(MOE_EINVAL, "precision 'mixed' runs on the fast 3x3 kernels only: conv_impl=v1 (MOE_CONV_IMPL=v1) is a debugging switch for 'fp16' / 'fp16x3'");
    // The chain of split-operand layers (conv_input2, the first nx ARSBs) on conv64_q8 passes its low parts as the fp8 words its correction products read
    // (Act::lo8): three quarters of the bytes of layers that are held by bytes (profiles/r03/o_stream_bytes.txt), no conversion of a_lo inside the kernel.
    // The last conv_2 writes an fp16 low part again -- into the stem's low-part buffer, which conv_input2 was the only reader of (its own buffer still
    // holds the fp8 residual it reads) -- for the fused ARSB kernels behind it.  The stem writes its low part in that form too (conv_input2 is its only
    // reader: the U branch takes the fp16 part).  No chain under set_debug's value 1 (its taps were written for fp16 low parts); value 2 taps the chain as it runs (Fwd::tap).
    // NetDN (round 6): its tail convs read the stem's hi + lo pair at the very end -- tail3 takes the stem's low part as the same fp8 words (TailArgs::in1_lo8), so the
    // stem writes ONE low-part form here too.  What NetDN cannot share is the buffer: the two-launch fallback of the last exact block writes its fp16 low part into a
    // buffer of its own (lo16x) instead of over the stem's words.
    const bool dn = n.arch == MOE_ARCH_NETDN;
    chain8 = mixed && f.use_q8() && n.opt.lo8 && !n.debug && !f.direct && nx >= 1 && A.has_lo && Bb.has_lo && Cc.has_lo;      // (flags: lo16x below is planned like everything else)
    if (dn && (int)n.scalars.at("tail_taps") != 9) chain8 = false;      // (the 1x1 tail kernel reads fp16 pairs only)
    for (int i = 0; chain8 && i <= nx; ++i)
        for (int j = (i == 0 ? 2 : 1); chain8 && j <= 2; ++j)
            chain8 = f.q8_capable(n.convs[n.conv_index.at(i == 0 ? std::string("input2") : "c" + std::to_string(j) + "_" + std::to_string(i))]);
    lo16x = (dn && chain8) ? (half_t*)f.ar.take((size_t)P * 64 * 2 + 2048) : nullptr;
    A.lo8 = Bb.lo8 = chain8;
    f.stem(A);
    f.tap("stem", A, h, w, 64, n.C);
    plan_tail_form();
    // Small launch sets (the reference's per-tile loop hands the net 3 planes of <= 256 x 256): a launch of a few planes leaves most CUs idle while its last workgroups
    // finish (702 ARSB patches over 256 workgroups; 24 four-row blocks per ps4 workgroup, two of them recomputed), and the U branch does not depend on the trunk -- it
    // forks here onto a second stream behind the stem and joins in front of the branch sum; its workgroups take the CUs the trunk's launches leave.  Same kernels, same
    // bits (tests); the predicate is a function of the shape alone, so the workspace plan (dry run) allocates in the same order.
    // (not under FP16X3: its three-launch fallback shares one side buffer between the layers)
    const bool forked = sr && f.ctx.fork && !n.debug && !f.direct && !f.x3 && n.opt.conv_impl == 2 && (long long)B * h * w <= 4ll * 65536;      // (up to four planes of 256 x 256: the per-tile call
                                                                                                                                      // with or without alpha; a ragged group of 21 planes of 88 x 256 inside a
                                                                                                                                      // batched frame is NOT small: forked, the headline frame lost 0.5 ms)
    // every exit behind the fork joins the side stream back into the caller's: an early return (a refused layer, a failed HIP call) must not leave kernels in flight on
    // the side stream that the caller's stream never waits for -- the caller may synchronize its own stream and reuse or free the workspace (forward_dev_chunk's regrow does),
    // and an unjoined fork makes hipStreamEndCapture fail.  Disarmed by the regular join in front of the branch sum.
    struct ForkGuard {
        StreamSet* set; hipStream_t s; bool armed = false;
        ~ForkGuard()
        {
            if (!armed) return;
            if (hipEventRecord(set->ev_join, set->side) != hipSuccess || hipStreamWaitEvent(s, set->ev_join, 0) != hipSuccess) (void)hipStreamSynchronize(set->side);
        }
    } fork_guard{f.ctx.set, s};
    // ... each branch on its own share of the chip: side stream g_side persistent workgroups per launch, the caller's stream the rest (f.groups: this forward's own)
    const int all = f.groups;
    int g_side = 0;
    if (forked && all >= 32) {
        g_side = n.opt.branch_groups > 0 ? n.opt.branch_groups : (n.stages >= 2 ? 5 * all / 16 : 3 * all / 16);
        g_side = std::max(8, std::min(g_side, all - 8) / 8 * 8);
    }
    if (forked) {
        if (g_side) f.groups = g_side;
        if (!f.dry()) {
            StreamSet& set = *f.ctx.set;
            if (!set.side) {
                HIP_TRY(hipStreamCreateWithFlags(&set.side, hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&set.ev_fork, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&set.ev_join, hipEventDisableTiming));
            }
            HIP_TRY(hipEventRecord(set.ev_fork, s));
            HIP_TRY(hipStreamWaitEvent(set.side, set.ev_fork, 0));      // behind the stem (and everything before it on the caller's stream: the previous forward's reads of the workspace)
            f.s = set.side;
            fork_guard.armed = true;
        }
        const int rc = run_branch(1, A);
        if (g_side) f.groups = all - g_side;      // the trunk and the R branch: the other CUs
        if (!f.dry()) {
            f.s = s;
            if (!rc) HIP_TRY(hipEventRecord(f.ctx.set->ev_join, f.ctx.set->side));
        }
        if (rc) return rc;
    }
    if (int rc = run_trunk()) return rc;
    if (n.arch == MOE_ARCH_NETDN) { f.tail(&Bb, &A, h, w, false); return MOE_OK; }
    if (mixed) { A.drop_lo(); Bb.drop_lo(); A.lo8 = Bb.lo8 = false; }      // the upsampler convs take the fp16 parts
    if (!forked) { if (int rc = run_branch(0, Bb)) return rc; if (int rc = run_branch(1, A)) return rc; }
    else {
        if (int rc = run_branch(0, Bb)) return rc;
        if (!f.dry()) { HIP_TRY(hipStreamWaitEvent(s, f.ctx.set->ev_join, 0)); fork_guard.armed = false; }      // the branch sum below reads both branches
        f.groups = all;
    }
    return branch_sum();
}

}  // namespace

int moe::forward_arsb(const moe_net& n, Fwd& f)
{
    ArsbRun r{n, f, f.B, f.h, f.w};
    return r.run();
}
