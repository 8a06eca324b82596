// net.h -- what the host sources of libmoephoto_amd.so share (internal, not part of the C ABI): error plumbing, the model object and its
// options, the state of one forward (Fwd) and the few functions that cross files.
//
// Reference for every sequence: python/models.py:108-223 (MyNet, Net2x/3x/4x, NetDN, SEDN/_Conv_Block),
// python/MoeNet_lite2.py:22-54 (Net), python/imageProcess.py:157-172 (doCrop).  See include/moephoto_amd.h.
#pragma once
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <utility>

namespace moe {

// =====================================================================================================
// errors (errors.cpp)
// =====================================================================================================
int fail(int code, const char* fmt, ...);      // the message moe_last_error returns (thread-local); returns `code`
int launched(const char* who);                 // behind a kernel launch: MOE_OK, or MOE_EHIP with "<who> launch failed: <hipGetLastError's text>"

inline bool plane_depth(int depth) { return depth == 8 || depth == 10 || depth == 12 || depth == 16; }      // the depths of planar samples

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(e_ == hipErrorOutOfMemory ? MOE_ENOMEM : MOE_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// A grow-only device buffer (the forwards' workspace, the plan's tile pool, the ensemble's scratch).  Work already enqueued on `s` may still read the old block:
// growing synchronises that stream before it frees.  A block that does not fit is MOE_ENOMEM with the caller's own message, and the buffer is empty.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    template <typename... A> int grow(size_t need, hipStream_t s, const char* does_not_fit, A... a)
    {
        if (need <= bytes) return MOE_OK;
        if (p) { HIP_TRY(hipStreamSynchronize(s)); HIP_TRY(hipFree(p)); p = nullptr; bytes = 0; }
        if (hipMalloc(&p, need) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return fail(MOE_ENOMEM, does_not_fit, a...); }
        bytes = need;
        return MOE_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }      // (the caller knows that nothing in flight reads it)
};

}  // namespace moe

// the 3D LUT colour step's handle (lut3d_api.cpp; ailut_api.cpp's generator writes its table)
struct moe_lut3d {
    int d, device;
    void* dev;              // one allocation: d^3 entries {R, G, B, 0}, then the 3 d vertices
    size_t table_bytes;
};

namespace moe {

// =====================================================================================================
// model
// =====================================================================================================
struct Param {
    std::string name;
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool set = false;
    int64_t numel() const { int64_t n = 1; for (auto d : shape) n *= d; return n; }
};

struct ConvLayer {               // one MFMA convolution
    int taps = 9, nseg = 1, nchunks = 1, r = 1;
    int cin = 64, cout = 64, k = 3;
    float slope = 1.f, scale = 1.f;
    bool per_plane = false;      // SEDN trans: weights rebuilt per plane by the SE kernel
    size_t w_hi = 0, w_lo = 0, bias = 0, bias_img = 0, w_plain = 0, bias_plain = 0, w_pk32 = 0;   // offsets into the device blob
    size_t w_arsb_lo = 0;        // ... and their low parts ((w - fp16(w)) * 2^11) in the same order, for conv64_x3.hip
    size_t wq_hi8 = 0, wq_lo8 = 0;   // ... w_hi 2^8 and w_lo 2^8 as fp8 e4m3 A fragments of v_mfma_scale_f32_32x32x64_f8f6f4 (conv64_q8.hip): [tap 9][half 2][lane 64][32 B]
    size_t w_arsb = 0;           // 3x3 64->64 trunk convs: A fragments of v_mfma_f32_16x16x32_f16 in conv64_x3.hip's order (the register-weight 16x16x32 form; round 2's arsb_fused.hip, retired, introduced it)
    size_t w_x3 = 0;             // 1x1, one segment, split precision: [chunk][w_lo | w_hi | w_hi] for the single-launch path (acc_mode 4)
    bool has_x3 = false;
    bool has_bias = false;
    int nfrag() const { return nseg * taps * 8; }
};

// an activation tensor: fp16 [B][H][W][C] and (split operands / the trunk stream of 'mixed') its low part, (v - fp16(v)) 2^11, as fp16 in the same layout --
// or, lo8, as the fp8 e4m3 word of that value / 4 (one byte a channel): the form conv64_q8.hip reads and writes between its own layers
// has_lo says whether the tensor HAS a low part: the flag is what decides a route or a buffer -- it is the same on the planning pass, where every pointer is null
struct Act {
    half_t* hi = nullptr; half_t* lo = nullptr; bool lo8 = false; bool has_lo = false;
    void drop_lo() { lo = nullptr; has_lo = false; }      // the reader takes the fp16 part only
};

struct Arena {                   // bump allocator over the net's workspace (dry run when base == nullptr)
    char* base = nullptr;
    size_t off = 0;
    size_t limit = 0;            // bytes behind base (what the planning pass sized)
    bool overflow = false;
    void* take(size_t bytes)
    {
        const size_t a = (off + 255) & ~(size_t)255;
        off = a + bytes;
        // a buffer the plan did not size: the rest of the sequence only counts (dry), so that no kernel is launched over it; forward_dev_chunk reports it
        // (inside forward_arsb's fork the side stream is joined by ForkGuard's destructor, as on every early exit)
        if (base && off > limit) { overflow = true; base = nullptr; }
        return base ? base + a : nullptr;
    }
};

// Kernel-form switches of one net.  Process-wide defaults come from the environment ONCE, when the net is created (MOE_* variables,
// kept for command-line A/B runs); after that only moe_net_set_option changes them -- the forward path reads no environment.
struct NetOptions {
    int conv_impl = 2;        // conv_impl   sp (2, default: the fast 3x3 kernels) | v1 (0: the generic kernel everywhere; debugging, not with 'mixed')
    int sp_impl = 1;          // sp_impl     auto (1: conv3x3_rw where it wins) | rw (2: conv3x3_rw for every epilogue it compiles) | sp (0: conv3x3_sp only)
    int tail_split = 1;       // tail_split  0 | r (1, default: the R branch's fused tail also splits its activation operand) | ru (2)
    int tail_form = 1;        // tail_form   sums (1, default: phase-class sums + aprons from conv3x3_rw, tapsum4) | planes (0: nine tap planes per phase, tapsum2)
    int up_fuse2 = 1;         // up_fuse2    1 (default): lite's last two upsampler stages + the folded tail in ONE launch (conv1x1_f2.hip, split operands) | 0: stage by stage (conv1x1.hip; same bits)
    int up_impl = 1;          // up_impl     ps4 (1, default: the fused-tail up-conv with all four phases in one workgroup, conv3x3_ps4.hip + tailadd) | rw (0: conv3x3_rw
                              //             per phase, phase-class sums, tapsum4 -- round 3's form, kept for A/B and for shapes ps4 does not take)
    int conv1x1 = 1;          // conv1x1     lite's 1x1 layers on conv1x1.hip (0: generic kernel)
    int x3_fuse = 1;          // x3_fuse     split-operand 3x3 64->64 layers as ONE launch (conv64_x3.hip; 0: three launches)
    int arsb_fuse = 1;        // arsb_fuse   single-pass ARSBs as one launch (0: two launches)
    int lo8 = 1;              // lo8         on (default): between conv64_q8 layers the low parts travel as fp8 words (64 instead of 128 bytes a pixel) | off
    int x3_impl = 0;          // x3_impl     auto (0, default: q8 for the SR nets, x3 for the DN nets -- see forward) | x3 (1: conv64_x3.hip, three fp16 products) |
                              //             q8 (2: conv64_q8.hip, the two correction products on fp8 operands)
    int k48 = 1;              // k48         1 (default): kernels that can skip the zero k-slice of the 48-channel nets do | 0: they run all four (A/B)
    int s64 = 1;              // s64         1 (default): SEDN's fused block tail on conv64_s.hip (streamed, per-plane weights in registers) | 0: conv3x3_sp<6>
    int branch_streams = 1;   // branch_streams  1 (default): small launch sets (the reference's own per-tile loop: 3 planes of <= 256 x 256 per forward) run the U branch on a second
                              //             HIP stream beside the trunk + R branch -- a launch of a few planes leaves CUs idle at its tail (702 ARSB patches over 256 workgroups) and the
                              //             other branch's workgroups take them; same kernels, same bits | 0: one stream
    int branch_groups = 0;    // branch_groups   persistent workgroups of the side stream's launches in that mode (0: 5/16 of the CUs for the x4 nets, 3/16 for x2 / x3 -- about the U
                              //             branch's share of the forward; a4: 29.0 / 27.4 / 27.9 / 28.4 ms per frame with 64 / 80 / 96 / 112, 34.1 with 48; a2: 20.1-20.2 with 24 .. 64,
                              //             21.6 on one stream -- profiles/r05/g_branch_streams.txt); the trunk + R branch launch max_groups minus that many.  A launch of 3 planes scales badly over 256
                              //             workgroups -- the per-tile loop takes 30.6 / 31.3 / 38.2 / 66.4 ms per frame with 256 / 192 / 128 / 64 (profiles/r05/f_small_launch_scaling.txt)
                              //             -- so the two branches are given disjoint shares of the chip instead of each launch spreading over all of it
    int exact_fuse = 1;       // exact_fuse  1 (default): an exact ARSB of a chain runs as ONE launch (arsb_sq.hip: conv_1's rows stay in LDS) | 0: conv_1, conv_2 on conv64_sq / conv64_q8
    int q8_impl = 1;          // q8_impl     s (1, default: conv64_sq.hip, the chain layers streamed down a column by an fp16 wave + an fp8 wave) | p (0: conv64_q8.hip, 8 x 32 patches)
                              // (the one-launch ARSB of the single-pass blocks is arsb32c.hip.  Earlier generations -- arsb_fused.hip, arsb32.hip (history at 689845f) and the streamed
                              // form arsb_s.hip (round 4: bit-identical, 7 % slower, both at the package power cap; history at 321d022, profiles/r04/d_arsb_streamed_vs_patch.txt) -- are
                              // no longer built)
    int fuse_tail = 1;        // fuse_tail   last upsampler conv + 64->1 / 48->1 tail conv in one kernel
    int sedn_fuse = 1;        // sedn_fuse   SEDN's fused block tail
    int pool_fuse = 1;        // pool_fuse   SE / FRM channel sums out of the producing conv's epilogue
    int lite_lut = 1;         // lite_lut    lite, fp16 inputs: the U branch as a table lookup inside the final sum (see moe_net::lut) | 0: computed
    int stem2 = 1;            // stem2       lite: conv_input2's output written by the stem in closed form (x times a fixed vector: StemArgs::w2), the 48 -> 48 1x1 conv not launched | 0: launched
    int frm_pre = 1;          // frm_pre     lite (fp16x3): the FRM gate of an LB from conv_2's INPUT (frm_pre_kernel), conv_2 stores gate * conv + x -- no frm_apply pass | 0: gate from conv_2's output, frm_apply
    int overlap_calls = 1;    // overlap_calls  1 (default): consecutive small forwards that the CALLER marks as independent of each other (moe_net_forward_ex with MOE_FWD_INPUT_SINCE_PREV:
                              //             "my input was complete when the previous forward of this net was enqueued" -- true of the reference's tile loop, whose inputs are slices of
                              //             ONE padded image, python/imageProcess.py:164-170) alternate between two internal (stream, workspace) sets: forward k+1 starts beside forward k
                              //             instead of behind it and the caller's blend; only its LAST kernel (the one that writes y) waits for the caller's stream | 0: every forward on
                              //             the caller's stream
    int overlap_fork = 0;     // overlap_fork   0 (default): such a forward does not fork its U branch onto a side stream as well -- two forwards in flight ARE the second stream | 1: it does
    int overlap_groups = 0;   // overlap_groups  persistent workgroups per launch of such a forward; 0 (default): half of the CUs -- two forwards in flight on half the chip each.
                              //             Measured on the reference-style loop of bench.py (profiles/r06/d_dropin_overlap_queues.txt; option off: 29.4 ms = 0.86 of the headline):
                              //             fork 0 / 128 groups 28.5 ms (0.89; 27.6 = 0.92 with moe_blend_tile), fork 1 / all groups 28.4 (0.89; 28.1), fork 0 / all groups 29.4,
                              //             fork 1 / 128 groups 35.8; GPU_MAX_HW_QUEUES = 8 or 16 instead of HIP's 4: 36-39 ms.  The chip is saturated either way: what separates the
                              //             loop from the device-resident path is the fixed cost of forty 3-plane launch sets (weight preloads, ramp-up and tail of every kernel), which
                              //             two forwards in flight hide only in part
    int calib_log = 0;        // calib_log   1: moe_net_calibrate prints every count's (SEDN: fp16's) measured and predicted error to stderr (tools/calib_report.py)
    int auto_calibrate = 1;   // auto_calibrate  1 (default): moe_net_finalize(MOE_PREC_AUTO) measures the count of split-operand ARSBs (SEDN: whether fp16 holds) on the loaded weights | 0: per-architecture defaults
    int exact_blocks_env = -1;   // MOE_EXACT_BLOCKS (moe_net_set_exact_blocks overrides)
    int tiles_per_batch = 0;  // tiles_per_batch   tiles of 256^2 pixels per launch set when the caller passes 0 (0: 32)
    int max_groups = 0;       // max_groups  persistent workgroups per launch (0: one per CU), applied at finalize
    int dbg = 0;              // dbg         timing-ablation bits of the conv kernels (results are wrong when set)
    std::string trace_key = "convt_R1.up1";
    bool arsb_trace = false;
    std::string repeat_key;   // repeat      "<layer key substring>:<n>": the bracketed launches (prof_begin sites) of matching layers are issued n times -- measurement only (tools/kernel_power.py:
    int repeat_n = 1;         //             one kernel looped by itself while rocm-smi samples the package power and clock); the launches are idempotent, results do not change


    // false: unknown key or value, and the option is as it was (options.cpp: one table, walked by both)
    bool set(const std::string& key, const char* v);
    void from_env();
};

// the device resources one forward at a time runs on (the forward grows / creates them on demand): its workspace, and the second stream of small launch sets (option
// branch_streams) -- the U branch forks behind the stem and joins in front of the branch sum
struct StreamSet { DevBuf ws; hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; };
// ... with a stream of its own: one of the two sets consecutive small forwards alternate between when the caller declares them independent (option overlap_calls, moe_net_forward_ex)
struct PipeSet : StreamSet { hipStream_t main = nullptr; hipEvent_t entry = nullptr, done = nullptr; };

// what a forward WRITES of its net besides its stream set -- records, never configuration (a sequence sees the net itself as const)
struct NetRuntime {
    // live kernel timing of selected conv layers (bench.py's roofline leg): hipEvent pairs on the launch stream
    struct ProfRec { hipEvent_t e0 = nullptr, e1 = nullptr; int key = 0; double flops = 0; };
    std::vector<ProfRec> prof_ev;                // event pairs, reused across steps
    size_t prof_used = 0;
    // debug taps
    struct Tap { float* dev = nullptr; int64_t shape[4] = {0, 0, 0, 0}; };
    std::map<std::string, Tap> taps;
    // moe_net_forward's host offset tables: a ring of pinned host slots + device slots, copied asynchronously on the launch stream
    struct OffSlot { long long* host = nullptr; long long* dev = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool used = false; };
    OffSlot off_ring[4];
    int off_next = 0;
};

}  // namespace moe

struct moe_net {
    int arch = 0, scale = 1;
    moe::NetOptions opt;
    int C = 64;                  // real channel count (48 for NetDN / lite); tensors are padded to 64
    int stages = 1, r = 2;       // upsampler stages and their shuffle factor
    std::vector<moe::Param> params;
    std::map<std::string, int> index;
    bool finalized = false;
    int device = -1, precision = MOE_PREC_FP16;
    int exact_blocks = -1;       // MOE_PREC_MIXED: leading ARSBs computed with split operands (-1: the calibrated count if there is one, else the per-architecture default)
    // calibration of THESE weights (moe_net_calibrate; run by moe_net_finalize(MOE_PREC_AUTO) on the ARSB nets and on SEDN): valid until a parameter changes
    bool calib_valid = false;
    // lite, fp16 inputs (round 6): the U branch (MoeNet_lite2.py:47,50: conv_input, uim, convt_I1) is POINTWISE -- 1x1 convs, pixel shuffles, PReLUs on a one-channel input -- so its
    // output at an HR pixel is a function of ONE input value and the pixel's phase: a table over the 65,536 fp16 bit patterns, filled once per checkpoint by the U branch's own
    // kernels run on an image of all patterns (bit-identical to computing it), [256 r][256 r] fp32.  lut_state: 0 not tried, 1 ready, -1 not available
    float* lut = nullptr; int lut_state = 0;
    int calib_blocks = -1;       // smallest count of split-operand ARSBs whose worst noise-tile error against the exact mode is within the target (-1: none is -> FP16X3);
                                 // SEDN: 0 = plain fp16 is within it, -1 = it is not -> FP16X3
    double calib_err = 0.0;      // that error, as predicted for the worst tile of a full frame (measured x the family's inflation factor)
    int auto_resolved = -1;      // what MOE_PREC_AUTO resolved to at the last finalize with it (-1: not finalized that way since the parameters changed)
    // device weights
    char* blob = nullptr;
    size_t blob_bytes = 0;
    std::vector<moe::ConvLayer> convs;
    std::map<std::string, int> conv_index;
    std::map<std::string, size_t> small;     // name -> blob offset of small fp32 / fp16 tables
    std::map<std::string, float> scalars;
    int max_groups = 256;        // persistent workgroups per launch (one per CU, or option max_groups): set at finalize
    std::vector<std::string> prof_keys;          // comma-separated substrings of moe_net_set_profile
    bool debug = false;          // debug taps wanted (moe_net_set_debug, value 1): the forwards also leave their fused forms, so that every layer has a tensor to tap
    bool tap_only = false;       // moe_net_set_debug, value 2 (every family but lite): taps wanted and NOTHING else changes -- no kernel choice reads this, the forward is the production one
    bool tapping() const { return debug || tap_only; }
    // what forwards write: the stream set of ordinary forwards, the two sets of forwards that run ahead of the caller's stream, the records
    moe::StreamSet set;
    moe::PipeSet pipe[2];
    int pipe_next = 0;
    bool pipe_prev_valid = false;
    hipStream_t pipe_last_stream = nullptr;
    moe::NetRuntime rt;
    // moe_run_plan_ens: the padded transformed image and the canvas of one symmetry's doCrop (device, grow-only like the workspace)
    moe::DevBuf ens_pad, ens_canvas;

    const moe::Param* get(const std::string& n) const
    {
        auto it = index.find(n);
        return it == index.end() ? nullptr : &params[it->second];
    }
    void add(const std::string& n, std::vector<int64_t> shape)
    {
        index[n] = (int)params.size();
        moe::Param p; p.name = n; p.shape = std::move(shape);
        params.push_back(std::move(p));
    }
};

namespace moe {

// =====================================================================================================
// forward (forward.cpp; the families' sequences: forward_arsb.cpp, forward_sedn.cpp, forward_lite.cpp)
// =====================================================================================================
// where a forward reads its planes and writes its result: caller's memory, strided, or gathered / scattered through device offset tables (the plan runners)
struct FwdIO {
    const void* x = nullptr; int x_dtype = MOE_F32; long long sB = 0, sH = 0, sW = 0; const long long* x_off = nullptr;
    void* y = nullptr; int y_dtype = MOE_F32; const long long* y_off = nullptr;
};

// what a forward is told from outside that is not the net's configuration.  Every forward gets one and none changes the net's: Fwd::route reads the net, f.groups and this.
struct FwdCtx {
    StreamSet* set = nullptr;         // the workspace and side stream it runs on (null: a planning pass alone -- moe_net_workspace_bytes)
    int groups = 0;                   // persistent workgroups per launch
    bool fork = false;                // a small launch set may run its U branch on the set's side stream
    hipEvent_t gate_event = nullptr;  // a forward ahead of the caller's stream: the kernel that writes the caller's y waits for this event (the caller's stream position at THIS call)
    float* lut_capture = nullptr;     // lite: this forward fills the U-branch table -- its input is the image of all fp16 patterns; part[1] is copied here instead of summed
};
// the ordinary forward: the given set (the net's own), every workgroup, the fork as option branch_streams says
inline FwdCtx own_ctx(const moe_net& n, StreamSet* set) { return FwdCtx{set, n.max_groups, n.opt.branch_streams != 0, nullptr, nullptr}; }

// what a layer is asked for beyond in / out / residual, named per call (all null: a plain convolution) ...
struct ConvExtra {
    const half_t* plane_w = nullptr;      // per-plane weights (SEDN trans: rebuilt per plane by the SE kernel) ...
    const half_t* plane_w_lo = nullptr;   // ... and their low parts (FP16X3)
    const half_t* tail_w = nullptr;       // fused tail (last up-conv + 64->1 / 48->1 3x3 tail conv in one kernel): the tail's A fragments ("<key>.frag") ...
    float* tplanes = nullptr;             // ... and where its tap planes / phase-class sums go (Fwd::tail_form)
    const float* tail1_w = nullptr;       // lite's fused 1x1 tail: the tail weights in fp32 ("<key>.f32") ...
    float* tail1_out = nullptr;           // ... and the partial planes (Fwd::tail1_parts of them per branch)
    bool exact = false;                   // MIXED: split operands for this layer (every layer has them under FP16X3)
    float* pool_out = nullptr;   // let the conv pool its output per plane (conv64_x3's pooled epilogue), [B][pool_slabs][64]
    int pool_slabs = 0;
    bool pool_act = false;       // ... with pool_out: the conv may pool BEHIND its PReLU (conv64_x3 EPI 4: lite's conv_1, whose output's sums make the FRM gate -- frm_pre)
    const float* gate_in = nullptr;   // with a residual: out = gate[plane][channel] * conv + residual (conv64_x3 EPI 5), [2][B][64]
    // WHAT is asked, as flags: these decide the route (the pointers above are null on the planning pass; they are arguments, never conditions)
    bool fuse_tail = false, fuse_tail1 = false, pool = false, gate = false;
};
// ... and what the kernel that takes the layer does with it (the same answer on both passes: it is the route's)
struct ConvDone {
    bool ok = true;              // false only when asked for the fused tail / an fp8 chain / split operands without a side buffer and no kernel can take the layer
    bool pooled = false;         // the conv pools into pool_out
    bool gated = false;          // the conv applies gate_in
    int tail1_parts = 0;         // fuse_tail1: partial planes per branch the fused 1x1 tail writes (conv_mfma_kernel: 2, conv1x1.hip: 1)
    explicit operator bool() const { return ok; }
};
// the kernel a layer resolves to: computed by Fwd::route from the layer, the net's options, the shape and the operands' forms; Fwd::launch fills the arguments of exactly that one
enum class ConvKernel {
    none, direct, conv1x1,
    mfma, sp, rw, ps4_store,     // single-pass layers: the generic kernel, conv3x3_sp, conv3x3_rw, conv3x3_ps4's store form
    sp_res_lo,                   // MIXED, single pass on the trunk stream: conv3x3_sp with the residual's low part as the addend of its split final epilogue
    mfma_x3,                     // split operands, 1x1: three products in one launch of the generic kernel (acc_mode 4)
    x3, q8, sq,                  // split operands, 3x3 64->64 in one launch: conv64_x3, conv64_q8, conv64_sq
    sp_three, acc32,             // split operands, the fallbacks: three launches of conv3x3_sp through side16; three of the generic kernel through the fp32 side buffer
};
struct ConvRoute {
    ConvKernel kernel = ConvKernel::none;
    ConvDone done;
    ConvForm form;               // the ConvArgs kernels' launch: shape, grid, epilogue flags
    ConvX3Form x3;               // the ConvX3Args kernels'
};
const char* kernel_name(ConvKernel k);

struct Fwd {
    const moe_net& n;
    const FwdCtx& ctx;
    NetRuntime* rt;              // (null on a planning pass, which launches and records nothing)
    hipStream_t s;
    int B, h, w;
    Arena ar;
    int groups;                  // persistent workgroups per launch, from ctx; forward_arsb gives each of its two streams a share while the U branch is forked
    bool x3, direct;
    bool mixed = false;          // MOE_PREC_MIXED: fp16 operands, fp32-equivalent (hi + lo) trunk stream, split operands on selected layers
    bool y_vec = false;
    float* acc32 = nullptr;
    size_t acc32_elems = 0;
    half_t* side16 = nullptr;    // fp16 sum of the two low-order products of a 3x3 conv (split precision), output layout
    bool dry() const { return ar.base == nullptr; }
    int rc = 0;                  // the internal error of a launch (Fwd::launch): the forward turns dry behind it (Fwd::conv), run_forward returns it
    bool skips_planned_work = false;   // the launching pass legitimately leaves out buffers the plan had to assume (today: lite's table lookup in place of the U branch)
    int tail_form = 0;           // fused tail of this forward: 0 nine tap planes (conv3x3_sp), 1 phase-class sums (conv3x3_rw + tapsum4)
    FwdIO io;

    Act act(long long pixels, int ch = 64, bool want_lo = false)
    {
        Act a;
        // + 2 KiB slack: the branch-free conv epilogue parks its predicated-off lanes just behind the last element
        a.hi = (half_t*)ar.take((size_t)pixels * ch * 2 + 2048);
        if (x3 || want_lo) { a.lo = (half_t*)ar.take((size_t)pixels * ch * 2 + 2048); a.has_lo = true; }
        return a;
    }
    template <typename T> T* blob(size_t off) const { return (T*)(n.blob + off); }
    template <typename T> T* small(const std::string& k) const { return (T*)(n.blob + n.small.at(k)); }

    // tap `name`: the activation as fp32, hi + lo 2^-11 where it has a low part.  That sum does not say which fp16 value a single-pass reader of the pair takes
    // (a low part of exactly half an ulp puts the sum midway between two fp16 values), so a pair also leaves tap `name`.hi: its fp16 part alone
    // A pair of the fp8 low-part chain (Act::lo8: value 2 on the ARSB nets, the chain does not exist under value 1) is hi + word 2^-9, what its readers add; it leaves
    // `name`.hi and `name`.w8, the words as fp32: (hi, word) is then the stored pair exactly.  An activation whose low part was dropped leaves neither.
    void tap(const std::string& name, const Act& a, int H, int W, int cs, int C)
    {
        if (!n.tapping() || dry()) return;
        auto forget = [&](const std::string& k) {      // (no stale part of an earlier forward that kept another form here)
            auto it = rt->taps.find(k);
            if (it != rt->taps.end()) { if (it->second.dev) (void)hipFree(it->second.dev); rt->taps.erase(it); }
        };
        if (a.lo && a.lo8) {
            float* v = tap_alloc(name, H, W, C);
            float* w8 = tap_alloc(name + ".w8", H, W, C);
            if (v && w8) launch_nhwc8_to_nchw_f32(a.hi, (const unsigned char*)a.lo, v, w8, B, H, W, cs, C, s);
            else { forget(name); forget(name + ".w8"); }      // (out of memory: no tap, never an unwritten one)
        } else {
            tap_part(name, a.hi, a.lo, H, W, cs, C);
            forget(name + ".w8");
        }
        if (a.lo) tap_part(name + ".hi", a.hi, nullptr, H, W, cs, C);
        else forget(name + ".hi");
    }
    float* tap_alloc(const std::string& name, int H, int W, int C)
    {
        auto& t = rt->taps[name];
        if (t.dev) { (void)hipFree(t.dev); t.dev = nullptr; }
        if (hipMalloc((void**)&t.dev, (size_t)B * C * H * W * 4) != hipSuccess) { t.dev = nullptr; return nullptr; }
        t.shape[0] = B; t.shape[1] = C; t.shape[2] = H; t.shape[3] = W;
        return t.dev;
    }
    void tap_part(const std::string& name, const half_t* hi, const half_t* lo, int H, int W, int cs, int C)
    {
        auto& t = rt->taps[name];
        if (t.dev) { (void)hipFree(t.dev); t.dev = nullptr; }
        const size_t nel = (size_t)B * C * H * W;
        if (hipMalloc((void**)&t.dev, nel * 4) != hipSuccess) return;
        t.shape[0] = B; t.shape[1] = C; t.shape[2] = H; t.shape[3] = W;
        launch_nhwc_to_nchw_f32(hi, lo, t.dev, B, H, W, cs, C, s);
    }
    void drop_taps()
    {
        if (!n.tapping() || dry()) return;
        for (auto& t : rt->taps) if (t.second.dev) (void)hipFree(t.second.dev);      // (hipFree waits for the device: no copy of an earlier forward is still writing)
        rt->taps.clear();
    }
    // ... a buffer as it lies in memory: per plane `per` fp16 values widened to fp32 (fragment-ordered weights), or `per` fp32 values copied on the launch stream; shape (B, per, 1, 1)
    void tap_raw16(const std::string& name, const half_t* p, long long per)
    {
        if (!n.tapping() || dry()) return;
        tap_part(name, p, nullptr, 1, 1, (int)per, (int)per);
    }
    void tap_f32(const std::string& name, const float* p, long long per)
    {
        if (!n.tapping() || dry()) return;
        auto& t = rt->taps[name];
        if (t.dev) { (void)hipFree(t.dev); t.dev = nullptr; }
        if (hipMalloc((void**)&t.dev, (size_t)B * per * 4) != hipSuccess) return;
        t.shape[0] = B; t.shape[1] = per; t.shape[2] = 1; t.shape[3] = 1;
        if (hipMemcpyAsync(t.dev, p, (size_t)B * per * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(t.dev); t.dev = nullptr; }
    }

    // MIXED: which fused-tail launches also split the activation operand.  The R branch (trunk -> upsampler -> tail) carries the larger
    // share of the remaining error (emulation: r.tail activations 3.8e-4 vs u.tail 1.3e-4 on noise); MOE_TAIL_SPLIT = 0 | r (default) | ru
    bool tail_split_for(const std::string& key) const
    {
        const int mode = n.opt.tail_split;
        return mode == 2 || (mode == 1 && key.compare(0, 8, "convt_R1") == 0);
    }

    // live timing (bench.py's roofline legs): a hipEvent pair on the launch stream around the launches of a layer whose key matches
    // one of the profile substrings.  Returns the record index or -1.
    int prof_begin(const std::string& key, double flops)
    {
        for (size_t i = 0; i < n.prof_keys.size(); ++i) {
            if (key.find(n.prof_keys[i]) == std::string::npos) continue;
            if (rt->prof_used == rt->prof_ev.size()) {
                NetRuntime::ProfRec r;
                if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return -1;
                rt->prof_ev.push_back(r);
            }
            NetRuntime::ProfRec& r = rt->prof_ev[rt->prof_used];
            r.key = (int)i; r.flops = flops;
            (void)hipEventRecord(r.e0, s);
            return (int)rt->prof_used++;
        }
        return -1;
    }
    void prof_end(int rec) { if (rec >= 0) (void)hipEventRecord(rt->prof_ev[rec].e1, s); }
    int repeats(const std::string& key) const { return (!n.opt.repeat_key.empty() && key.find(n.opt.repeat_key) != std::string::npos) ? n.opt.repeat_n : 1; }

    // The two correction products on fp8 operands (conv64_q8.hip): 'mixed' only -- 'fp16x3' promises 2e-5, fp8 corrections deliver ~15 bits.
    // auto: the SR nets, whose all-tile sweep keeps its margin with it (worst 8.1e-4 either way, profiles/r03/m_conv64_q8.txt); the DN nets
    // (dn_lite5 7.2e-4 -> 8.6e-4 of the 1e-3 bar) stay on three fp16 products.
    bool use_q8() const { return mixed && (n.opt.x3_impl == 2 || (n.opt.x3_impl == 0 && (n.scale > 1 || n.arch == MOE_ARCH_NETDN))); }      // (round 6: NetDN too -- dn_lite5 7.6e-4 against 8.1e-4 on conv64_x3, and faster)
    // what route() asks of a layer before it hands it to conv64_q8 in a chain of fp8 low parts (besides the tensors' own conditions), at the trunk's resolution
    bool q8_capable(const ConvLayer& L) const
    {
        ConvX3Form c;
        c.B = B; c.H = h; c.W = w; c.slope = L.slope; c.in8 = c.out8 = true;
        return n.opt.x3_fuse && n.opt.conv_impl == 2 && L.k == 3 && L.r == 1 && L.nchunks == 1 && L.nseg == 1 && !L.per_plane && L.wq_hi8 && L.w_arsb_lo && !L.has_bias && conv64_q8_applicable(c);
    }

    // one convolution layer: in [B][H][W][64*nseg] -> out [B][H*r][W*r][r>1 ? 64 : 64*nchunks] = route, then (launching pass) launch
    ConvDone conv(const std::string& key, const Act& in, const Act& out, const Act* res, int H, int W, const ConvExtra& extra = ConvExtra{});
    // which kernel takes the layer: a pure function of the layer, the options, the shape and the operands' FORMS (Act::has_lo / lo8, ConvExtra's flags) -- no pointer, no launcher
    ConvRoute route(const std::string& key, const Act& in, const Act& out, const Act* res, int H, int W, const ConvExtra& extra = ConvExtra{}) const;
    ConvForm form(const ConvLayer& L, int H, int W) const;      // the layer's plain launch at H x W: shape, grid, slope / scale
    int launch(const ConvRoute& r, const std::string& key, const Act& in, const Act& out, const Act* res, const ConvExtra& extra);
    // the first and the last kernel of every family: x -> stem (lite: + conv_input2's output in closed form), and the unfused tail conv(s) -> y
    void stem(const Act& out, const Act* out2 = nullptr);
    void tail(const Act* r, const Act* u, int H, int W, bool skip);
    void gate();
};

// the families' sequences (run_forward dispatches; each takes its workspace from f.ar in the SAME order on the planning pass and on the launching one: forward.cpp)
int forward_arsb(const moe_net& n, Fwd& f);
int forward_sedn(const moe_net& n, Fwd& f);
int forward_lite(const moe_net& n, Fwd& f);

// forward.cpp
int exact_blocks_of(const moe_net& n);
int default_exact_blocks(int arch);
long long sp_bytes_per_pixel(const moe_net& n);
constexpr long long kSpRange = (1ll << 32) - (1ll << 16);
int forward_dev(moe_net& n, const FwdIO& io, int B, int h, int w, hipStream_t s, bool y_off_mult8, const FwdCtx& ctx);
void free_set(StreamSet& set);      // (synchronizes its side stream first)
void pipe_destroy(moe_net& n);
void free_records(NetRuntime& rt);
inline void free_ens_scratch(moe_net& n) { n.ens_pad.release(); n.ens_canvas.release(); }
// weights.cpp
int build_device_weights(moe_net& n, int precision);
void drop_lut(moe_net& n);
// calibrate.cpp
bool calibratable(const moe_net& n);
int calibrate_blocks(moe_net& n, double target, hipStream_t s);
int calibrate_sedn(moe_net& n, double target, hipStream_t s, bool adopt);

}  // namespace moe
