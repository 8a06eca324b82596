// forward.cpp -- one forward of a net: Fwd::route (which kernel a layer resolves to) and Fwd::launch (that kernel's arguments), the workspace plan and its check, the
// launch sets, the calls that run ahead of the caller's stream, and the entry points around them.
//
// PLANNING PASS AND LAUNCHING PASS ARE ONE CODE PATH.  The sequence of a family (forward_arsb / forward_sedn / forward_lite) is run twice per launch set: first by
// workspace_need with an Arena that has no base (Fwd::dry(): Arena::take only counts, launch / stem / tail and every `if (!f.dry())` block launch nothing), then by
// forward_dev_chunk over the workspace of that size.  So every f.ar.take -- f.act included -- must come in the same order, with the same sizes, on both passes:
// what decides whether a buffer is taken may depend on the net, its options and the shape, never on a pointer or on what a kernel launcher answered.
//
// HOW A LAYER FINDS ITS KERNEL.  Fwd::conv = route, then (launching pass only) launch.  route is a pure function of the layer, the options, the shape and the operands'
// forms -- flags: Act::has_lo / lo8, ConvExtra's requests -- and asks each candidate kernel's *_applicable predicate (common.h), the very function its launcher refuses
// by; its answer (kernel, pooled, gated, tail parts, ok) is the same on both passes, so the sequences branch on it freely.  launch fills the arguments of exactly that
// kernel: a launcher that refuses what its predicate promised is an internal error naming layer and kernel, never a fall-through to another kernel.  What route reads
// beyond the net is the forward's own: f.groups and its context (FwdCtx: stream set, workgroups, fork, gate, table capture) -- no forward writes the net's configuration.
//
// THE CHECK.  The arena of the launching pass carries the planned size as its limit: a take beyond it turns the rest of the sequence dry (nothing is launched over
// memory the plan did not size) and fails the forward; behind the sequence forward_dev_chunk compares the two passes' final offsets (plan_matches).
#include "net.h"

using namespace moe;

namespace moe {

const char* kernel_name(ConvKernel k)      // (in ConvKernel's order)
{
    static const char* const names[] = {"no kernel", "conv_direct", "conv1x1", "conv_mfma", "conv3x3_sp", "conv3x3_rw", "conv3x3_ps4 (store form)", "conv3x3_sp (hi + lo residual)",
                                        "conv_mfma (three products)", "conv64_x3", "conv64_q8", "conv64_sq", "conv3x3_sp (three launches)", "conv_mfma (fp32 side buffer)"};
    return names[(int)k];
}

// 3x3 / 64-input-channel layers with shared weights run on the fast kernels (conv3x3_sp.hip and its relatives); everything else (1x1 convs, SEDN's per-plane
// `trans`, MOE_CONV_IMPL=v1) on the generic one
static bool fast_layer(const moe_net& n, const ConvLayer& L) { return L.taps == 9 && L.nseg == 1 && !L.per_plane && n.opt.conv_impl == 2; }

ConvForm Fwd::form(const ConvLayer& L, int H, int W) const
{
    ConvForm c;
    c.B = B; c.H = H; c.W = W; c.in_cs = 64 * L.nseg; c.out_cs = L.r > 1 ? 64 : 64 * L.nchunks; c.r = L.r; c.nchunks = L.nchunks;
    c.py = (H + kTileH - 1) / kTileH;
    const long long items = (long long)B * ((W + kTileW - 1) / kTileW) * c.py;
    // Workgroup (chunk, g) is block ((g / 8) * nchunks + chunk) * 8 + g % 8 and blocks go round-robin to the 8 XCDs, so an XCD gets
    // nchunks * ceil(G / 8) persistent workgroups: keep that within its CUs (one 160-KiB workgroup per CU), or some XCDs need a
    // second round (Net3x: 9 chunks x G = 28 put 36 workgroups on four XCDs of 32 CUs -- 0.67 instead of 0.48 ms per launch)
    const int per_xcd = groups / 8;
    int G = per_xcd >= L.nchunks ? 8 * (per_xcd / L.nchunks) : groups / L.nchunks;
    if (G < 1) G = 1;
    if (G > items) G = (int)items;
    c.G = G;
    c.slope = L.slope; c.scale = L.scale; c.dbg = n.opt.dbg;
    return c;
}

ConvRoute Fwd::route(const std::string& key, const Act& in, const Act& out, const Act* res, int H, int W, const ConvExtra& e) const
{
    ConvRoute r;
    auto take = [&r](ConvKernel k) { r.kernel = k; return r; };
    auto refuse = [&r]() { r.kernel = ConvKernel::none; r.done.ok = false; return r; };
    const ConvLayer& L = n.convs[n.conv_index.at(key)];
    const bool x3 = this->x3 || e.exact;      // split operands for this layer (every layer under FP16X3, selected ones under MIXED)
    const bool res_lo = res && res->has_lo;
    const bool any8 = in.lo8 || out.lo8 || (res && res->lo8);      // fp8 low parts: conv64_q8 / conv64_sq or nothing (the caller planned the chain with q8_capable)
    if (any8 && !(x3 && use_q8() && q8_capable(L) && !direct)) return refuse();
    if (e.fuse_tail1) r.done.tail1_parts = 2;      // (conv_mfma_kernel's two channel halves, unless conv1x1.hip takes the layer)
    ConvForm& c = r.form;
    c = form(L, H, W);
    if (direct) return take(ConvKernel::direct);
    const int px = (W + kTileW - 1) / kTileW;
    c.res = res != nullptr; c.tail1 = e.fuse_tail1;
    c.tail = e.fuse_tail; c.tail_form = e.fuse_tail ? tail_form : 0; c.tail_split = (e.fuse_tail && mixed && tail_split_for(key)) ? 1 : 0;
    if (e.pool && !x3 && L.r == 1 && L.nchunks == 1 && !res && pooled_groups_ok((long long)c.py, (long long)B * c.py, groups)) {      // conv3x3_rw's pooled epilogue (SEDN rblock.2)
        c.pool = true; c.pool_slabs = e.pool_slabs;
        c.G = pooled_groups((long long)c.py, (long long)B * c.py, groups);      // its work items are patch ROWS (conv3x3_rw.hip, EPI 4): slab contents independent of the launch's plane count (common.h)
    }
    const bool fast = fast_layer(n, L);
    if (e.fuse_tail && !(fast && !x3)) return refuse();
    // lite's 1x1 convs (conv_input2, the upsampler stages with or without the folded 48->1 tail): the HBM-bound kernel of conv1x1.hip,
    // in fp16 or with split operands; MOE_CONV1X1=0 keeps them on the generic kernel (A/B)
    if (n.opt.conv1x1 && L.taps == 1 && L.nseg == 1 && !L.per_plane && !res && L.scale == 1.f && !e.fuse_tail && n.opt.conv_impl == 2 && (!x3 || (in.has_lo && L.has_x3)) &&
        conv1x1_applicable(Conv1x1Form{B, H, W, L.r, L.nchunks, c.out_cs, L.slope, x3, e.fuse_tail1, x3 && out.has_lo}, groups)) {
        if (e.fuse_tail1) r.done.tail1_parts = 1;
        return take(ConvKernel::conv1x1);
    }
    const bool traced = !x3 && (c.dbg & 64) && fast && key == n.opt.trace_key;      // the timing trace of one launch (launch): of the layer's plain single-pass form
    if (!x3 && !traced && res_lo && out.has_lo) {
        // MIXED, single-pass layer on the trunk stream: fp16 operands, but the residual is read as hi + lo * 2^-11, added in fp32
        // and the sum stored as hi and lo again (the split-precision final epilogue with the residual's low part as its addend):
        // the stream x + s*conv2(...) is carried to ~22 bits through the six ARSBs, only the MFMA operand is its fp16 part
        c.acc_mode = 3; c.side16 = true; c.out_lo = true;
        r.done.ok = fast && conv3x3_sp_applicable(c);
        return take(ConvKernel::sp_res_lo);
    }
    if (!x3) {
        // the fused tail in its phase-class-sums form: conv3x3_rw is the only producer of that buffer layout
        if (c.tail && c.tail_form == 1) { r.done.ok = conv3x3_rw_applicable(c); return take(ConvKernel::rw); }
        // The x2 upsampler stages that store their tensor: all four phases in one workgroup (conv3x3_ps4.hip, store form) -- when a workgroup gets at least
        // 32 four-row blocks: a range recomputes two blocks at its ends, and a launch of three planes of 256 x 256 (the reference's own per-tile loop) would
        // give each of the 256 workgroups six.  conv3x3_rw<1> below produces the same bits (same MFMAs in the same order), so the choice is invisible.
        if (fast && n.opt.up_impl == 1 && !c.tail && !c.pool && c.r == 2 && c.nchunks == 4 && c.in_cs == 64 && !c.res && c.scale == 1.f && !c.dbg && L.has_bias &&
            (long long)B * px * (H / 4) >= 32ll * groups && ps4_store_applicable(B, H, W, L.slope))
            return take(ConvKernel::ps4_store);
        // PReLU-only epilogues (first upsampler stage of Net4x, SEDN's rblock convs) run on the register-resident-weights kernel
        // (conv3x3_rw.hip: 6 % faster there); option sp_impl = sp keeps them on conv3x3_sp (A/B)
        if (fast && n.opt.sp_impl && !c.tail && conv3x3_rw_applicable(c)) { r.done.pooled = c.pool; return take(ConvKernel::rw); }
        if (fast && conv3x3_sp_applicable(c)) return take(ConvKernel::sp);
        if (c.tail) return refuse();
        return take(ConvKernel::mfma);
    }
    // 1x1 conv: all three products in one launch (K segments (w_lo, a_hi), (w_hi, a_lo), (w_hi, a_hi)); the activations are
    // read once per product from L2/HBM and nothing goes through the fp32 side buffer (2.6x less traffic than three passes)
    if (L.has_x3 && !fast) return take(ConvKernel::mfma_x3);
    // 3x3 64->64 with both weight parts packed for it: all three products in ONE launch (conv64_x3.hip)
    if (n.opt.x3_fuse && fast && L.w_arsb_lo && in.has_lo && out.has_lo && (!res || res_lo) && !e.fuse_tail && !L.has_bias) {
        ConvX3Form q;
        q.B = B; q.H = H; q.W = W; q.slope = L.slope; q.res = res != nullptr; q.res_lo = res_lo;
        const long long P = (long long)px * c.py;      // (conv64_x3's patches are 8 x 32 outputs, as the launcher counts them)
        if (e.pool && !res && (L.slope == 1.f || e.pool_act) && pooled_groups_ok(P, (long long)B * P, groups)) { q.pool = true; q.pool_slabs = e.pool_slabs; }
        if (e.gate && res && !use_q8()) q.gate = true;
        r.x3 = q;
        // (use_q8: the two correction products on fp8 operands, conv64_q8.hip; its chain form streamed down a column, conv64_sq.hip)
        if (use_q8() && L.wq_hi8 && !q.pool && (!res || res->lo8 == in.lo8)) {
            r.x3.in8 = in.lo8; r.x3.out8 = out.lo8;
            if (n.opt.q8_impl == 1 && conv64_sq_applicable(r.x3, groups)) return take(ConvKernel::sq);
            if (conv64_q8_applicable(r.x3)) return take(ConvKernel::q8);
            r.x3 = q;
        }
        if (any8) return refuse();
        if (conv64_x3_applicable(q, groups)) { r.done.pooled = q.pool; r.done.gated = q.gate; return take(ConvKernel::x3); }
    }
    if (fast && L.nchunks <= 16) {
        // 3x3 conv: the two low-order products run on the fast kernel as ordinary fp16-output convolutions --
        //   side = conv(w_lo, a_hi)            (plain epilogue)
        //   side = conv(w_hi, a_lo) + side     (residual epilogue, in place)
        // both in units of 2^-11; the main pass adds side * 2^-11 before its epilogue.  fp16 is plenty for a term that small,
        // and nothing goes through the fp32 side buffer (its read-modify-write traffic bounded the three-pass form).
        // (a residual's low part is in the same units: it rides along as the `residual` of the first low-order launch)
        ConvForm q1 = c; q1.res = res_lo; q1.slope = 1.f; q1.scale = 1.f; q1.tail = false;
        ConvForm q2 = q1; q2.res = true;
        ConvForm q3 = c; q3.acc_mode = 3; q3.side16 = true; q3.out_lo = out.has_lo;      // (res_lo is inside side16)
        if (conv3x3_sp_applicable(q1) && conv3x3_sp_applicable(q2) && conv3x3_sp_applicable(q3)) return take(ConvKernel::sp_three);
        // (a final epilogue the fast kernel does not compile, e.g. a PReLU slope above 1: the layer goes through the fp32 side buffer)
    }
    // hi/lo split: (w_lo * a_hi) -> acc32,  += (w_hi * a_lo),  then (w_hi * a_hi) + acc32/2048 and the epilogue
    if (!acc32_elems) return refuse();                               // (MIXED carries no fp32 side buffer unless a steep PReLU needs one: run_forward)
    return take(ConvKernel::acc32);
}

// the arguments of exactly the kernel the route names; MOE_OK, or the internal error of a launcher that refused what its predicate promised
int Fwd::launch(const ConvRoute& r, const std::string& key, const Act& in, const Act& out, const Act* res, const ConvExtra& e)
{
    const ConvLayer& L = n.convs[n.conv_index.at(key)];
    const ConvForm& c = r.form;
    const int H = c.H, W = c.W;
    if (r.kernel == ConvKernel::direct) {
        DirectConvArgs d{};
        d.in = in.hi; d.out = out.hi; d.res = res ? res->hi : nullptr;
        d.w = blob<float>(L.w_plain);
        d.bias = L.has_bias ? blob<float>(L.bias_plain) : nullptr;
        d.w_batch_stride = 0;
        d.B = B; d.H = H; d.W = W; d.in_cs = c.in_cs; d.out_cs = c.out_cs; d.cin = L.cin; d.cout = L.cout; d.k = L.k; d.r = L.r;
        d.slope = L.slope; d.scale = L.scale;
        if (L.per_plane) { d.w = (const float*)e.plane_w; d.w_batch_stride = (long long)L.cout * L.cin; }
        launch_conv_direct(d, s);
        return MOE_OK;
    }
    ConvArgs a{};
    a.in = in.hi; a.out = out.hi; a.res = res ? res->hi : nullptr;
    a.wpk = L.per_plane ? e.plane_w : blob<half_t>(L.w_hi);
    a.bias = L.has_bias ? blob<float>(L.bias) : small<float>("zero_bias");   // kernels initialise their accumulators from the bias vector
    a.zero = small<half_t>("zero");
    a.bias_img = blob<float>(L.bias_img);
    a.trash = small<half_t>("trash");
    a.w_batch_stride = L.per_plane ? (long long)L.nchunks * L.nfrag() * 512 : 0;
    a.B = B; a.H = H; a.W = W; a.in_cs = c.in_cs; a.out_cs = c.out_cs; a.r = c.r; a.nchunks = c.nchunks;
    a.px = (W + kTileW - 1) / kTileW; a.py = c.py; a.G = c.G;
    a.slope = c.slope; a.scale = c.scale; a.dbg = c.dbg;
    a.tail_w = e.tail_w; a.tplanes = e.tplanes; a.tail_form = c.tail_form; a.tail_split = c.tail_split;
    a.tail1_w = e.tail1_w; a.tail1_out = e.tail1_out;
    if (c.pool) { a.pool = e.pool_out; a.pool_slabs = c.pool_slabs; }
    const bool x3 = this->x3 || e.exact;
    // live timing of the one-launch forms; algorithmic flops (real channel counts), three products with split operands
    const bool timed = r.kernel != ConvKernel::mfma_x3 && r.kernel != ConvKernel::sp_three && r.kernel != ConvKernel::acc32;
    const int rec = timed ? prof_begin(key, (x3 ? 3 : 1) * 2.0 * (double)B * H * W * L.cout * L.cin * L.taps) : -1;
    bool ok = true;
    auto single = [&](const ConvArgs& ca) {      // the single-pass kernels
        if (r.kernel == ConvKernel::rw) return launch_conv3x3_rw(ca, s);
        if (r.kernel == ConvKernel::sp) return launch_conv3x3_sp(ca, s);
        if (r.kernel == ConvKernel::ps4_store) {
            Ps4Args q{};
            q.in = ca.in; q.wpk = ca.wpk; q.bias = ca.bias; q.out = ca.out; q.slope = ca.slope; q.B = ca.B; q.H = ca.H; q.W = ca.W;
            return launch_conv3x3_ps4(q, groups, s);
        }
        launch_conv_mfma(ca, L.taps, L.nseg, s);
        return true;
    };
    switch (r.kernel) {
    case ConvKernel::conv1x1: {
        Conv1x1Args q{};
        q.in_hi = in.hi; q.in_lo = x3 ? in.lo : nullptr; q.out_hi = out.hi; q.out_lo = x3 ? out.lo : nullptr;
        q.w_hi = blob<half_t>(L.w_hi); q.w_lo = x3 ? blob<half_t>(L.w_lo) : nullptr; q.bias = a.bias;
        q.tail_w = e.tail1_w; q.tail_out = e.tail1_out; q.slope = L.slope;
        q.B = B; q.H = H; q.W = W; q.r = L.r; q.nchunks = L.nchunks; q.out_cs = c.out_cs;
        q.nks = (L.cin <= 48 && n.opt.k48) ? 3 : 4;
        ok = launch_conv1x1(q, groups, s);
        break;
    }
    case ConvKernel::mfma: case ConvKernel::sp: case ConvKernel::rw: case ConvKernel::ps4_store: {
        unsigned long long* tr = nullptr;
        const size_t nb = 8 * 32 * 4 * 16 * 8;
        if (!x3 && (c.dbg & 64) && fast_layer(n, L) && key == n.opt.trace_key && hipMalloc((void**)&tr, nb) == hipSuccess) {   // timing trace of one launch -> /tmp/moe_trace.bin
            (void)hipMemsetAsync(tr, 0, nb, s);
            ConvArgs t = a; t.acc32 = (float*)tr;
            ok = single(t);
            std::vector<unsigned long long> host(nb / 8);
            (void)hipStreamSynchronize(s);
            (void)hipMemcpy(host.data(), tr, nb, hipMemcpyDeviceToHost);
            if (FILE* f = fopen("/tmp/moe_trace.bin", "wb")) { fwrite(host.data(), 1, nb, f); fclose(f); }
            (void)hipFree(tr);
        } else
            ok = single(a);
        break;
    }
    case ConvKernel::sp_res_lo: {
        ConvArgs q = a; q.acc_mode = 3; q.side16 = res->lo; q.out_lo = out.lo; q.res_lo = nullptr;
        ok = launch_conv3x3_sp(q, s);
        break;
    }
    case ConvKernel::mfma_x3: {
        ConvArgs f4 = a; f4.wpk = blob<half_t>(L.w_x3); f4.acc_mode = 4; f4.in_lo = in.lo; f4.out_lo = out.lo; f4.res_lo = res ? res->lo : nullptr;
        launch_conv_mfma(f4, 1, 3, s);
        break;
    }
    case ConvKernel::x3: case ConvKernel::q8: case ConvKernel::sq: {
        ConvX3Args q{};
        q.in_hi = in.hi; q.in_lo = in.lo; q.out_hi = out.hi; q.out_lo = out.lo;
        q.res_hi = res ? res->hi : nullptr; q.res_lo = res ? res->lo : nullptr;
        q.w_hi = blob<half_t>(L.w_arsb); q.w_lo = blob<half_t>(L.w_arsb_lo); q.zero = small<half_t>("zero");
        q.slope = L.slope; q.B = B; q.H = H; q.W = W;
        if (r.x3.pool) { q.pool = e.pool_out; q.pool_slabs = e.pool_slabs; }
        if (r.x3.gate) q.gate = e.gate_in;
        if (r.kernel == ConvKernel::x3) { ok = launch_conv64_x3(q, groups, s); break; }
        q.wq_hi16 = blob<half_t>(L.w_hi); q.wq_hi8 = blob<unsigned char>(L.wq_hi8); q.wq_lo8 = blob<unsigned char>(L.wq_lo8);
        q.in8 = r.x3.in8; q.out8 = r.x3.out8;
        ok = r.kernel == ConvKernel::sq ? launch_conv64_sq(q, groups, s) : launch_conv64_q8(q, groups, s);
        break;
    }
    case ConvKernel::sp_three: {      // (see route)
        ConvArgs q1 = a; q1.wpk = blob<half_t>(L.w_lo); q1.out = side16; q1.res = (res && res->has_lo) ? res->lo : nullptr; q1.bias = small<float>("zero_bias");
        q1.bias_img = small<float>("zero_bias_img"); q1.slope = 1.f; q1.scale = 1.f; q1.acc_mode = 0; q1.tail_w = nullptr; q1.tplanes = nullptr;
        ConvArgs q2 = q1; q2.in = in.lo; q2.wpk = blob<half_t>(L.w_hi); q2.res = side16;
        ConvArgs q3 = a; q3.acc_mode = 3; q3.side16 = side16; q3.out_lo = out.lo; q3.res_lo = nullptr;   // res_lo is inside side16
        ok = launch_conv3x3_sp(q1, s) && launch_conv3x3_sp(q2, s) && launch_conv3x3_sp(q3, s);
        break;
    }
    case ConvKernel::acc32: {
        a.acc32 = acc32;
        ConvArgs p1 = a; p1.wpk = L.per_plane ? e.plane_w_lo : blob<half_t>(L.w_lo); p1.acc_mode = 1; p1.res = nullptr; p1.bias = nullptr;
        launch_conv_mfma(p1, L.taps, L.nseg, s);
        ConvArgs p2 = a; p2.in = in.lo; p2.acc_mode = 2; p2.res = nullptr; p2.bias = nullptr;
        launch_conv_mfma(p2, L.taps, L.nseg, s);
        ConvArgs p3 = a; p3.acc_mode = 3; p3.out_lo = out.lo; p3.res_lo = res ? res->lo : nullptr;
        launch_conv_mfma(p3, L.taps, L.nseg, s);
        break;
    }
    default: ok = false;
    }
    prof_end(rec);
    if (!ok) return fail(MOE_EINVAL, "internal error: layer %s (%d planes of %dx%d) was routed to %s, and that launcher refused it", key.c_str(), B, H, W, kernel_name(r.kernel));
    return MOE_OK;
}

// one convolution layer: in [B][H][W][64*nseg] -> out [B][H*r][W*r][r>1 ? 64 : 64*nchunks]
// !ok only when asked for the fused tail / an fp8 chain / a side buffer the forward does not carry and no kernel can take the layer that way: nothing is launched then
ConvDone Fwd::conv(const std::string& key, const Act& in, const Act& out, const Act* res, int H, int W, const ConvExtra& e)
{
    const ConvRoute r = route(key, in, out, res, H, W, e);
    if (r.done.ok && !dry()) {
        rc = launch(r, key, in, out, res, e);
        // a refused launch ends the launching: the arena loses its base, so the rest of the sequence only counts (dry()) -- no kernel is enqueued over the tensor that
        // was not written -- and run_forward returns rc.  (Inside forward_arsb's fork the side stream is joined by ForkGuard's destructor, as on every early exit.)
        if (rc) ar.base = nullptr;
    }
    return r.done;
}

void Fwd::stem(const Act& out, const Act* out2)
{
    if (dry()) return;
    StemArgs a{};
    if (out2) { a.w2 = small<float>("stem.p2"); a.out2 = out2->hi; a.out2_lo = out2->lo; }
    a.x = io.x; a.x_dtype = io.x_dtype; a.x_off = io.x_off; a.sB = io.sB; a.sH = io.sH; a.sW = io.sW;
    a.w = small<float>("stem"); a.slope = n.scalars.at("stem_slope");
    a.out = out.hi; a.out_lo = out.lo; a.out_lo8 = out.lo8; a.B = B; a.H = h; a.W = w; a.taps = (int)n.scalars.at("stem_taps");
    launch_stem(a, s);
}

// forwards that run ahead of the caller's stream (moe_net_forward_ex): everything up to here touched the net's own workspace only; the kernel that writes the caller's y
// must not overtake what the caller enqueued before this call (y's memory may have been in use by it)
void Fwd::gate() { if (ctx.gate_event && !dry()) (void)hipStreamWaitEvent(s, ctx.gate_event, 0); }

void Fwd::tail(const Act* r, const Act* u, int H, int W, bool skip)
{
    gate();
    if (dry()) return;
    TailArgs a{};
    a.in0 = r->hi; a.w0 = small<half_t>("tail_r");
    if (u) { a.in1 = u->hi; a.w1 = small<half_t>("tail_u"); }
    if (r->has_lo && (!u || u->has_lo)) {     // split operands (FP16X3; MIXED on NetDN, whose tail convs read the hi + lo stream directly)
        a.in0_lo = r->lo; a.w0_lo = small<half_t>("tail_r.lo");
        if (u) { a.in1_lo = u->lo; a.w1_lo = small<half_t>("tail_u.lo"); a.in1_lo8 = u->lo8; }
    }
    if (skip) { a.skip = io.x; a.skip_dtype = io.x_dtype; a.skip_off = io.x_off; a.skip_sB = io.sB; a.skip_sH = io.sH; a.skip_sW = io.sW; }
    a.y = io.y; a.y_dtype = io.y_dtype; a.y_off = io.y_off; a.B = B; a.H = H; a.W = W; a.taps = (int)n.scalars.at("tail_taps");
    launch_tail(a, s);
}

static size_t acc32_need(const moe_net& n, int B, int h, int w)
{
    // largest [B][H][W][nchunks*64] fp32 any conv of this net produces (pre-shuffle coordinates)
    size_t best = 0;
    long long HW = (long long)h * w;
    if (n.arch == MOE_ARCH_SEDN) return (size_t)B * (size_t)HW * 256;
    int rr = 1;
    best = (size_t)B * (size_t)HW * 64;
    for (int s = 0; s < n.stages; ++s) {
        best = std::max<size_t>(best, (size_t)B * (size_t)HW * rr * rr * 64 * n.r * n.r);
        rr *= n.r;
    }
    return best;
}

int exact_blocks_of(const moe_net& n)
{
    // leading ARSBs with split operands under MOE_PREC_MIXED.  Emulated error budget (tools/emu_precision.py), worst
    // of uniform-noise tiles: Net4x 7.6e-4 / 6.2e-4 / 5.1e-4 with 0 / 1 / 3 blocks; Net2x (whose trunk is 61 % of the net and whose
    // output swing is three times larger) 1.3e-3 / 9.1e-4 / 6.2e-4 / 3.7e-4 with 0 / 1 / 3 / 6; NetDN 7.8e-4 / 6.5e-4 / 5.0e-4 with 0 / 1 / 3
    if (n.exact_blocks >= 0) return n.exact_blocks > 6 ? 6 : n.exact_blocks;
    const int env = n.opt.exact_blocks_env;
    if (env >= 0) return env > 6 ? 6 : env;
    if (n.calib_valid && n.calib_blocks >= 0) return n.calib_blocks;      // measured on this checkpoint (moe_net_calibrate), never below the architecture's default
    return default_exact_blocks(n.arch);
}

int default_exact_blocks(int arch)
{
    switch (arch) {
        case MOE_ARCH_NET2X: return 4;      // measured on the GPU, worst tile of three 1080p uint8-noise frames vs the exact mode: 1.6e-3 / 1.3e-3 / 8.8e-4 / 7.0e-4 / 5.3e-4
                                            // with 1 / 2 / 3 / 4 / 6 blocks at 14.4 / 16.0 / 17.6 / 19.0 / 22.2 ms per frame (profiles/r03): 4 keeps 30 % of margin
        case MOE_ARCH_NET3X: return 2;
        case MOE_ARCH_NET4X: return 1;
        case MOE_ARCH_NETDN: return 1;
        default: return 0;
    }
}

// The fast 3x3 kernel addresses its stores, residual loads and tap planes with 32-bit BYTE offsets.  Bytes one plane of h x w
// pixels occupies in the largest tensor such a launch touches (so that planes-per-launch = 2^32 / this):
//   trunk / LR layers            128 B per pixel (64 fp16 channels; SEDN's 256-channel rblock.4 output 512 B when unfused)
//   upsampler stage k output     128 B * r^(2(k+1)) per input pixel; the LAST stage stores no tensor when the tail is fused,
//                                its nine fp32 tap planes take 36 B per output pixel instead
long long sp_bytes_per_pixel(const moe_net& n)
{
    long long per = 128;
    if (n.arch == MOE_ARCH_SEDN) per = 512;
    if (n.arch == MOE_ARCH_LITE) {
        // lite: stage k stores 128 B * 4^(k+1) per input pixel, the LAST stage (fused with the 48 -> 1 tail) stores two fp32 partial planes per branch instead -- so the largest
        // tensor a 32-bit-offset kernel (conv1x1.hip) touches is the last stage's INPUT: 128 B * 4^(stages-1).  (Round 5's kernel census found lite8's x4 -> x8 stage on the
        // generic 64-bit kernel at 27 ms a launch: 96 planes of 1024 x 1024 x 128 B overflow the offsets and nothing split the launch set.)
        for (int st = 0; st + 1 < n.stages; ++st) per *= 4;
    }
    if (n.arch == MOE_ARCH_NET2X || n.arch == MOE_ARCH_NET3X || n.arch == MOE_ARCH_NET4X) {
        long long rr = 1;
        for (int st = 0; st < n.stages; ++st) {
            rr *= (long long)n.r * n.r;
            per = std::max(per, st == n.stages - 1 ? 36 * rr : 128 * rr);     // (the unfused fallback of the last stage runs on the 64-bit kernels)
        }
    }
    return per;
}

static int run_forward(const moe_net& n, Fwd& f, const FwdIO& io)
{
    const int B = f.B, h = f.h, w = f.w;
    const long long P = (long long)B * h * w;
    f.io = io;
    if (f.x3) {
        f.acc32_elems = acc32_need(n, B, h, w);
        f.acc32 = (float*)f.ar.take(f.acc32_elems * 4);
        f.side16 = (half_t*)f.ar.take(f.acc32_elems * 2 + 4096);
    } else if (f.mixed) {
        f.side16 = (half_t*)f.ar.take((size_t)P * 64 * 2 + 4096);     // split-operand layers exist at the input resolution only
        bool steep = false;                                            // a PReLU slope above 1 takes the layer off the fast kernel's final pass
        for (int i = 1; i <= exact_blocks_of(n); ++i) steep = steep || n.convs[n.conv_index.at("c1_" + std::to_string(i))].slope > 1.f;
        if (steep) { f.acc32_elems = (size_t)P * 64; f.acc32 = (float*)f.ar.take(f.acc32_elems * 4); }
    }
    int rc = MOE_OK;
    switch (n.arch) {
        case MOE_ARCH_SEDN: rc = forward_sedn(n, f); break;
        case MOE_ARCH_LITE: rc = forward_lite(n, f); break;
        default: rc = forward_arsb(n, f);      // Net2x / Net3x / Net4x, NetDN
    }
    return rc ? rc : f.rc;      // (f.rc: a launcher refused the layer its route promised -- Fwd::launch)
}

// one forward's state: the planning pass (no base in the arena, no stream, no records) and the launching pass are built alike
static Fwd make_fwd(const moe_net& n, const FwdCtx& ctx, NetRuntime* rt, hipStream_t s, int B, int h, int w, Arena ar)
{
    Fwd f{n, ctx, rt, s, B, h, w, ar, ctx.groups, n.precision == MOE_PREC_FP16X3, n.precision == MOE_PREC_DEBUG_DIRECT};
    f.mixed = n.precision == MOE_PREC_MIXED;
    return f;
}

static size_t workspace_need(const moe_net& n, const FwdCtx& ctx, int B, int h, int w)
{
    Fwd f = make_fwd(n, ctx, nullptr, nullptr, B, h, w, Arena{});
    run_forward(n, f, FwdIO{});
    return f.ar.off + 4096;
}

// THE CHECK behind the launching pass: it took exactly what the planning pass counted -- or less, where it legitimately left out work the plan had to assume
static bool plan_matches(const Fwd& f, size_t planned)
{
    if (f.ar.overflow) return false;
    return f.skips_planned_work ? f.ar.off <= planned : f.ar.off == planned;
}

static int forward_dev_chunk(moe_net& n, const FwdIO& io, int B, int h, int w, hipStream_t s, bool y_off_mult8, const FwdCtx& ctx);

// The table of lite's U branch (moe_net::lut), filled on the first fp16 forward of a checkpoint: one forward of the net on a 256 x 256 one-plane image whose pixel
// (i, j) holds the fp16 bit pattern 256 i + j, told through its context (FwdCtx::lut_capture) that forward_lite copies the U branch's plane (part[1]) instead of summing.  Not during stream capture (it allocates), not for
// precisions / options whose fused tail is not the one-part form (then the table stays unavailable and the branch is computed as before).
static void build_lite_lut_on_device(moe_net& n, hipStream_t s, const FwdCtx& ctx)
{
    const int r = n.scale;
    std::vector<unsigned short> pat(65536);
    for (int i = 0; i < 65536; ++i) pat[(size_t)i] = (unsigned short)i;
    half_t* in = nullptr;
    float* scratch = nullptr;
    int rc = MOE_ENOMEM;
    if (hipMalloc((void**)&in, 65536 * 2) == hipSuccess && hipMalloc((void**)&n.lut, (size_t)65536 * r * r * 4) == hipSuccess && hipMalloc((void**)&scratch, (size_t)65536 * r * r * 4) == hipSuccess &&
        hipMemcpyAsync(in, pat.data(), 65536 * 2, hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess) {
        FwdCtx capture = ctx;
        capture.lut_capture = n.lut;
        rc = forward_dev_chunk(n, FwdIO{in, MOE_F16, 65536, 256, 1, nullptr, scratch, MOE_F32, nullptr}, 1, 256, 256, s, true, capture);
        (void)hipStreamSynchronize(s);
    }
    if (in) (void)hipFree(in);
    if (scratch) (void)hipFree(scratch);
    if (rc != MOE_OK) { (void)hipGetLastError(); drop_lut(n); }
    n.lut_state = rc == MOE_OK ? 1 : -1;      // (-1 while the table's own forward runs, too: it computes the branch it captures -- build_lite_lut)
}

static void build_lite_lut(moe_net& n, hipStream_t s, const FwdCtx& ctx)
{
    n.lut_state = -1;
    if (n.arch != MOE_ARCH_LITE || !n.opt.lite_lut || n.debug || !n.opt.fuse_tail || n.precision == MOE_PREC_DEBUG_DIRECT) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); n.lut_state = 0; return; }      // (another forward may try)
    // the table, its input and the scratch live on the net's device, whichever device the caller has current; the caller's current device is left as it was
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || (cur != n.device && hipSetDevice(n.device) != hipSuccess)) { (void)hipGetLastError(); n.lut_state = 0; return; }
    build_lite_lut_on_device(n, s, ctx);
    if (cur != n.device) (void)hipSetDevice(cur);
}

int forward_dev(moe_net& n, const FwdIO& io, int B, int h, int w, hipStream_t s, bool y_off_mult8, const FwdCtx& ctx)
{
    if (!n.finalized) return fail(MOE_ESTATE, "moe_net_forward: net is not finalized (load_state_dict + to(device) first)");
    if (B < 1 || h < 1 || w < 1) return fail(MOE_EINVAL, "moe_net_forward: bad shape B=%d h=%d w=%d", B, h, w);
    if ((io.x_dtype != MOE_F32 && io.x_dtype != MOE_F16) || (io.y_dtype != MOE_F32 && io.y_dtype != MOE_F16))
        return fail(MOE_EINVAL, "moe_net_forward: x/y dtype must be MOE_F32 or MOE_F16");
    // planes per launch set: whatever the caller batched (whole-image tiles under cropsize 'auto', MOE_TILES_PER_BATCH ...), a launch
    // never leaves the fast kernel's addressing range -- larger batches are run as several launch sets
    const long long bmax = kSpRange / (sp_bytes_per_pixel(n) * (long long)h * w);
    if (bmax < 1)
        return fail(MOE_ENOMEM, "a %dx%d tile exceeds the convolution kernels' addressing range (%lld pixels per plane at most for this net): use a smaller cropsize",
                    h, w, kSpRange / sp_bytes_per_pixel(n));
    if (n.arch == MOE_ARCH_LITE && io.x_dtype == MOE_F16 && n.lut_state == 0 && n.opt.lite_lut) build_lite_lut(n, s, ctx);      // (after the checks: a refused call builds nothing)
    if (B <= bmax) return forward_dev_chunk(n, io, B, h, w, s, y_off_mult8, ctx);
    const size_t xe = io.x_dtype == MOE_F32 ? 4 : 2, ye = io.y_dtype == MOE_F32 ? 4 : 2;
    const long long yplane = (long long)h * n.scale * w * n.scale;
    for (int b0 = 0; b0 < B; b0 += (int)bmax) {
        const int cnt = (int)std::min<long long>(bmax, B - b0);
        FwdIO c = io;      // this launch set's planes: the tables advance, or the base pointers do
        if (io.x_off) c.x_off += b0; else c.x = (const char*)io.x + (size_t)b0 * io.sB * xe;
        if (io.y_off) c.y_off += b0; else c.y = (char*)io.y + (size_t)b0 * yplane * ye;
        const bool al = y_off_mult8 && (io.y_off || ((size_t)b0 * yplane * ye) % 16 == 0);
        if (int rc = forward_dev_chunk(n, c, cnt, h, w, s, al, ctx)) return rc;
    }
    return MOE_OK;
}

static int forward_dev_chunk(moe_net& n, const FwdIO& io, int B, int h, int w, hipStream_t s, bool y_off_mult8, const FwdCtx& ctx)
{
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != n.device) HIP_TRY(hipSetDevice(n.device));
    const size_t need = workspace_need(n, ctx, B, h, w);
    StreamSet& set = *ctx.set;
    if (int rc = set.ws.grow(need, s, "workspace of %zu bytes for %d planes of %dx%d does not fit", need, B, h, w)) return rc;
    const size_t planned = need - 4096;
    Fwd f = make_fwd(n, ctx, &n.rt, s, B, h, w, Arena{(char*)set.ws.p, 0, planned});
    f.y_vec = y_off_mult8 && ((uintptr_t)io.y % 16 == 0);   // every output plane starts 16-byte aligned: wide stores allowed
    int rc = run_forward(n, f, io);
    if (rc) return rc;
    if (!plan_matches(f, planned))
        return fail(MOE_EINVAL, "internal error: the launching pass took %zu bytes of workspace%s, the planning pass %zu (%d planes of %dx%d)", f.ar.off,
                    f.ar.overflow ? " (beyond the plan: the launches behind that point were not issued)" : "", planned, B, h, w);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    return MOE_OK;
}

void free_set(StreamSet& set)
{
    if (set.side) { (void)hipStreamSynchronize(set.side); (void)hipStreamDestroy(set.side); }
    for (hipEvent_t e : {set.ev_fork, set.ev_join}) if (e) (void)hipEventDestroy(e);
    set.ws.release();
    set = StreamSet{};
}

void free_records(NetRuntime& rt)
{
    for (auto& ev : rt.prof_ev) { (void)hipEventDestroy(ev.e0); (void)hipEventDestroy(ev.e1); }
    for (auto& sl : rt.off_ring) {
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.dev) (void)hipFree(sl.dev);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    for (auto& t : rt.taps) if (t.second.dev) (void)hipFree(t.second.dev);
    rt = NetRuntime{};
}

void pipe_destroy(moe_net& n)
{
    for (auto& ps : n.pipe) {
        if (ps.main) { (void)hipStreamSynchronize(ps.main); (void)hipStreamDestroy(ps.main); }
        for (hipEvent_t e : {ps.entry, ps.done}) if (e) (void)hipEventDestroy(e);
        free_set(ps);
        ps = PipeSet{};
    }
    n.pipe_prev_valid = false;
    n.pipe_last_stream = nullptr;
}

// Small forwards of the SR nets that may run ahead of the caller's stream (the per-tile calls of the reference's loop: up to four planes of 256 x 256)
static bool overlap_eligible(const moe_net& n, int B, int h, int w)
{
    const bool sr = n.arch == MOE_ARCH_NET2X || n.arch == MOE_ARCH_NET3X || n.arch == MOE_ARCH_NET4X;
    return sr && n.finalized && n.opt.overlap_calls && !n.debug && n.opt.conv_impl == 2 && (n.precision == MOE_PREC_MIXED || n.precision == MOE_PREC_FP16) &&
           (long long)B * h * w <= 4ll * 65536 && n.prof_keys.empty() && n.opt.repeat_key.empty();
}

// The reference's tile loop (python/imageProcess.py:164-170) is  r = model(x[..., tile]); blend(r, canvas)  per tile: on ONE stream forward k+1 queues behind the blend of
// tile k, which waits for forward k -- although forward k+1 needs nothing tile k produced.  A 3-plane forward cannot fill 256 CUs (its kernels' workgroups each preload 288
// weight registers; 702 ARSB patches over 256 persistent workgroups: DESIGN.md section 4.10), so the drop-in loop ran at 0.84-0.86 of the device-resident path.  With
// MOE_FWD_INPUT_SINCE_PREV the caller states what makes the overlap legal -- "x was complete on `stream` when the PREVIOUS forward of this net was enqueued" -- and the forward
// runs on one of two internal (stream, workspace) sets behind the previous call's ENTRY event instead of behind everything enqueued since; its last kernel, the only one that
// touches the caller's memory (y), waits for this call's own entry event, and the caller's stream waits for the forward's completion before the call returns: whatever the
// caller enqueues next (the blend) is ordered as before.  Without the flag (or for the first call of a burst) the dependency is this call's entry event: plain stream order.
static int forward_pipelined(moe_net* n, const void* x, int x_dtype, int B, int h, int w, int64_t sB, int64_t sH, int64_t sW, void* y, int y_dtype, hipStream_t s, unsigned flags)
{
    HIP_TRY(hipSetDevice(n->device));
    PipeSet& ps = n->pipe[n->pipe_next];
    PipeSet& prev = n->pipe[n->pipe_next ^ 1];
    if (!ps.main) {
        HIP_TRY(hipStreamCreateWithFlags(&ps.main, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ps.entry, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ps.done, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(ps.entry, s));
    const bool since_prev = (flags & MOE_FWD_INPUT_SINCE_PREV) && n->pipe_prev_valid && n->pipe_last_stream == s && prev.entry;
    HIP_TRY(hipStreamWaitEvent(ps.main, since_prev ? prev.entry : ps.entry, 0));
    n->pipe_next ^= 1;
    // its own set, its share of the chip (two forwards in flight: half each by default), its last kernel behind this call's entry; forking the U branch as well is an option
    const int groups = n->opt.overlap_groups > 0 ? std::max(16, std::min(n->opt.overlap_groups, n->max_groups)) : std::max(16, n->max_groups / 2);
    const FwdCtx ctx{&ps, groups, n->opt.overlap_fork && n->opt.branch_streams, since_prev ? ps.entry : nullptr, nullptr};
    const int rc = forward_dev(*n, FwdIO{x, x_dtype, sB, sH, sW, nullptr, y, y_dtype, nullptr}, B, h, w, ps.main, true, ctx);
    // the caller's stream continues behind this forward -- also when it failed half-way (kernels may be in flight on the set's streams)
    if (hipEventRecord(ps.done, ps.main) != hipSuccess || hipStreamWaitEvent(s, ps.done, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(ps.main); }
    n->pipe_prev_valid = rc == MOE_OK;
    n->pipe_last_stream = s;
    return rc;
}

}  // namespace moe

extern "C" {

int moe_net_forward_ex(moe_net* n, const void* x, int x_dtype, int B, int h, int w, int64_t sB, int64_t sH, int64_t sW,
                       const int64_t* x_off, void* y, int y_dtype, const int64_t* y_off, void* stream, unsigned flags)
{
    if (!n || !x || !y) return fail(MOE_EINVAL, "moe_net_forward: NULL argument");
    if (flags & ~(unsigned)MOE_FWD_INPUT_SINCE_PREV) return fail(MOE_EINVAL, "moe_net_forward_ex: unknown flags 0x%x", flags);
    if ((flags & MOE_FWD_INPUT_SINCE_PREV) && !x_off && !y_off && B >= 1 && h >= 1 && w >= 1 && overlap_eligible(*n, B, h, w)) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone)
            return forward_pipelined(n, x, x_dtype, B, h, w, sB, sH, sW, y, y_dtype, (hipStream_t)stream, flags);
        (void)hipGetLastError();
    }
    n->pipe_prev_valid = false;          // (a forward on the caller's own stream ends a burst)
    return moe_net_forward(n, x, x_dtype, B, h, w, sB, sH, sW, x_off, y, y_dtype, y_off, stream);
}

int moe_net_forward(moe_net* n, const void* x, int x_dtype, int B, int h, int w, int64_t sB, int64_t sH, int64_t sW,
                    const int64_t* x_off, void* y, int y_dtype, const int64_t* y_off, void* stream)
{
    if (!n || !x || !y) return fail(MOE_EINVAL, "moe_net_forward: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    long long* xo = nullptr;
    long long* yo = nullptr;
    NetRuntime::OffSlot* slot = nullptr;
    if (x_off || y_off) {
        // The host tables ride to the device on the launch stream: a slot of a small ring (pinned host copy + device copy) per call,
        // reused once the event recorded behind the forward that reads it has fired -- no hipMalloc, no blocking copy, no stream synchronisation.
        HIP_TRY(hipSetDevice(n->device >= 0 ? n->device : 0));
        NetRuntime::OffSlot& sl = n->rt.off_ring[n->rt.off_next];
        n->rt.off_next = (n->rt.off_next + 1) % 4;
        if (sl.used) HIP_TRY(hipEventSynchronize(sl.done));          // (only when four such forwards are still in flight)
        const size_t need = (size_t)B * 2;
        if (need > sl.cap) {
            if (sl.host) { (void)hipHostFree(sl.host); sl.host = nullptr; }
            if (sl.dev) { (void)hipFree(sl.dev); sl.dev = nullptr; }
            sl.cap = 0;
            const size_t cap = std::max<size_t>(need, 256);
            HIP_TRY(hipHostMalloc((void**)&sl.host, cap * 8, hipHostMallocDefault));
            HIP_TRY(hipMalloc((void**)&sl.dev, cap * 8));
            sl.cap = cap;
        }
        if (!sl.done) HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        for (int i = 0; i < B; ++i) { sl.host[i] = x_off ? x_off[i] : 0; sl.host[B + i] = y_off ? y_off[i] : 0; }
        HIP_TRY(hipMemcpyAsync(sl.dev, sl.host, need * 8, hipMemcpyHostToDevice, s));
        sl.used = true;
        slot = &sl;
        if (x_off) xo = sl.dev;
        if (y_off) yo = sl.dev + B;
    }
    bool mult8 = true;
    if (y_off) for (int i = 0; i < B; ++i) mult8 = mult8 && (y_off[i] % 8 == 0);
    const int rc = forward_dev(*n, FwdIO{x, x_dtype, sB, sH, sW, xo, y, y_dtype, yo}, B, h, w, s, mult8, own_ctx(*n, &n->set));
    // the slot's event covers the copy AND every kernel of this forward that reads the tables: recorded behind them, on their stream, so that a later call on
    // ANOTHER stream cannot overwrite the tables while this forward is still in flight (the host wait above is on this event)
    if (slot && hipEventRecord(slot->done, s) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(s); }
    return rc;
}

int64_t moe_net_workspace_bytes(const moe_net* n, int B, int h, int w)
{
    if (!n || B < 1 || h < 1 || w < 1) return fail(MOE_EINVAL, "moe_net_workspace_bytes: bad argument");
    if (!n->finalized) return fail(MOE_ESTATE, "moe_net_workspace_bytes: net is not finalized");
    return (int64_t)workspace_need(*n, own_ctx(*n, nullptr), B, h, w);
}

int moe_net_set_profile(moe_net* n, const char* layer_substrings)
{
    if (!n) return fail(MOE_EINVAL, "moe_net_set_profile: NULL net");
    n->prof_keys.clear();
    std::string all = layer_substrings ? layer_substrings : "";
    size_t pos = 0;
    while (pos <= all.size() && !all.empty()) {
        const size_t c = all.find(',', pos);
        const std::string k = all.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
        if (!k.empty()) n->prof_keys.push_back(k);
        if (c == std::string::npos) break;
        pos = c + 1;
    }
    n->rt.prof_used = 0;
    return MOE_OK;
}

int moe_net_get_profile_at(moe_net* n, int index, double* total_ms, int64_t* launches, double* flops)
{
    if (!n || !total_ms || !launches || !flops) return fail(MOE_EINVAL, "moe_net_get_profile: NULL argument");
    double ms = 0, fl = 0;
    int64_t cnt = 0;
    for (size_t i = 0; i < n->rt.prof_used; ++i) {
        const NetRuntime::ProfRec& r = n->rt.prof_ev[i];
        if (r.key != index) continue;
        HIP_TRY(hipEventSynchronize(r.e1));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.e0, r.e1));
        ms += t; fl += r.flops; ++cnt;
    }
    *total_ms = ms; *launches = cnt; *flops = fl;
    return MOE_OK;
}

int moe_net_get_profile(moe_net* n, double* total_ms, int64_t* launches, double* flops)
{
    int rc = moe_net_get_profile_at(n, 0, total_ms, launches, flops);
    if (rc == MOE_OK) n->rt.prof_used = 0;
    return rc;
}

int64_t moe_net_max_tile_pixels(const moe_net* n)
{
    if (!n) return fail(MOE_EINVAL, "moe_net_max_tile_pixels: NULL net");
    return (int64_t)(kSpRange / sp_bytes_per_pixel(*n));
}

int moe_net_set_debug(moe_net* n, int enable)
{
    if (!n) return fail(MOE_EINVAL, "moe_net_set_debug: NULL net");
    if (enable == 2 && n->arch == MOE_ARCH_LITE)
        return fail(MOE_EINVAL, "moe_net_set_debug: value 2 (taps of the production forward) is defined for SEDN, Net2x / Net3x / Net4x and NetDN; 1 taps lite's unfused forward");
    n->debug = enable != 0 && enable != 2;
    n->tap_only = enable == 2;
    return MOE_OK;
}

int64_t moe_net_debug_tap(moe_net* n, const char* tap, float* host, int64_t capacity, int64_t shape[4], void* stream)
{
    if (!n || !tap) return fail(MOE_EINVAL, "moe_net_debug_tap: NULL argument");
    auto it = n->rt.taps.find(tap);
    if (it == n->rt.taps.end() || !it->second.dev) return fail(MOE_EINVAL, "no tap named \"%s\" (enable moe_net_set_debug before the forward)", tap);
    const auto& t = it->second;
    const int64_t nel = t.shape[0] * t.shape[1] * t.shape[2] * t.shape[3];
    if (shape) for (int d = 0; d < 4; ++d) shape[d] = t.shape[d];
    if (!host) return nel;
    if (capacity < nel) return fail(MOE_EINVAL, "moe_net_debug_tap: capacity %lld < %lld", (long long)capacity, (long long)nel);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(host, t.dev, (size_t)nel * 4, hipMemcpyDeviceToHost));
    return nel;
}

}  // extern "C"
