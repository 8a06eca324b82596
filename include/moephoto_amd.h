/* moephoto_amd.h -- C ABI of libmoephoto_amd.so: the MI355X (gfx950) engine behind MoePhoto's
 * tiled SR / denoise hot path.  Plain pointers and sizes only; no torch types.
 *
 * Every entry point replaces one piece of the reference's Python/PyTorch path (paths relative to
 * the MoePhoto repo; see INTEGRATION.md for the ctypes stub a maintainer adds):
 *
 *   moe_net_create        the model constructors of the plugin tables' "constructor slot":
 *                         Net2x/Net3x/Net4x/NetDN/SEDN (python/models.py:125-223) and
 *                         MoeNet_lite2.Net(upscale) (python/MoeNet_lite2.py:22-37), as selected by
 *                         runSR.mode_switch (python/runSR.py:10-24) / runDN.mode_switch (runDN.py:10-21)
 *   moe_net_set_param     nn.Module.load_state_dict, one call per state-dict entry
 *                         (python/imageProcess.py:319-328: model.load_state_dict(weights))
 *   moe_net_finalize      castModel / model.to(dtype, device) (python/imageProcess.py:309-317)
 *   moe_net_forward       modelCached(x): the torch.nn forward invoked from Option.__call__
 *                         (python/imageProcess.py:391-395) inside doCrop's tile loop (:164-166)
 *   moe_plan_*            the tile planner prepare/getAnchors (python/imageProcess.py:19-35,73-118)
 *   moe_stitch            the blend + slice-assign part of doCrop (python/imageProcess.py:120-131,167-170)
 *   moe_run_plan          doCrop as a whole (python/imageProcess.py:157-172): tile gather -> net -> stitch,
 *                         device resident, batched over same-shaped tiles
 *   moe_run_plan_ens      the SR self-ensemble around doCrop (python/imageProcess.py:563-572, runSR.py:26): moe_sym_pad / moe_sym_fold are its two passes
 *   moe_to_float/_output  toTorch / toOutput (python/imageProcess.py:245-263)
 *   moe_*_planes*         no counterpart: a video chain on the decoder's own Y'CbCr 4:2:0 planes instead of the bgr24 / bgr48le pipe (python/video.py:24,219)
 *
 * All functions return 0 on success or a negative MOE_E* code; moe_last_error() returns a
 * thread-local description (the Python wrapper raises RuntimeError / MemoryError from it, matching
 * worker.enhance's error envelope, python/worker.py:52-74).  Device work is enqueued on the caller's
 * hipStream_t (passed as void*) and never synchronised here: the reference runs on torch's current
 * stream in one thread (python/worker.py:89-93), so must we.
 */
#ifndef MOEPHOTO_AMD_H
#define MOEPHOTO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOE_ABI_VERSION 4      /* 4: moe_net_forward_ex / MOE_FWD_INPUT_SINCE_PREV (round 6); still 4 with moe_sym_pad / moe_sym_fold / moe_run_plan_ens and with moe_stitch_out / moe_run_plan_out: additions only, every earlier entry point is unchanged, so a caller built against the earlier 4 runs as before (a caller of the new ones looks the symbols up); 3: moe_net_calibrate / moe_net_exact_blocks, MOE_PREC_AUTO measures the checkpoint at finalize, moe_blend_tile (round 5); 2: MOE_PREC_AUTO, moe_net_resolved_precision, moe_plan_rows / moe_stitch_band, moe_plan_seams / moe_wire_* (round 4); 1 also lacked a bump for moe_net_set_option / moe_device_info / moe_stitch_dev */

/* error codes */
#define MOE_OK 0
#define MOE_EINVAL (-1)   /* bad argument / unknown parameter name / shape mismatch */
#define MOE_ENOMEM (-2)   /* host or device allocation failed, or a tile does not fit (-> MemoryError) */
#define MOE_EHIP (-3)     /* a HIP runtime call failed (no device, launch failure, ...) */
#define MOE_ESTATE (-4)   /* call order violated (forward before finalize, missing parameters) */

/* architectures: the constructor slot of the plugin tables */
#define MOE_ARCH_NET2X 0  /* models.Net2x  : a2/p2 */
#define MOE_ARCH_NET3X 1  /* models.Net3x  : a3/p3 */
#define MOE_ARCH_NET4X 2  /* models.Net4x  : a4/p4 */
#define MOE_ARCH_NETDN 3  /* models.NetDN  : dn_lite5/10/15 */
#define MOE_ARCH_SEDN 4   /* models.SEDN   : l15/l25/l50 */
#define MOE_ARCH_LITE 5   /* MoeNet_lite2.Net(upscale = `scale` in {2,4,8}) */

/* element types of caller-visible buffers */
#define MOE_F32 0
#define MOE_F16 1
#define MOE_U8 2
#define MOE_U16 3

/* arithmetic of the MFMA convolutions (weights/activations as operands; accumulate is always fp32,
 * the 1-channel stem and the final branch sum are always fp32) */
#define MOE_PREC_FP16 0        /* fp16 operands, one MFMA pass: the reference's GPU fp16 mode (config.fp16) */
#define MOE_PREC_FP16X3 1      /* hi/lo split operands, three MFMA passes: ~fp32 products */
#define MOE_PREC_DEBUG_DIRECT 2 /* slow scalar device convolution, fp32 accumulate; kernel debugging only */
#define MOE_PREC_MIXED 3       /* Net2x/3x/4x, NetDN: fp16 operands; the trunk stream x + s*conv2(..) of the six ARSBs
                                * (python/models.py:76-80) and the stem output are carried as hi + lo pairs (~fp32),
                                * conv_input2 and the first moe_net_set_exact_blocks() ARSBs use split operands, the 64->1
                                * tail convs see their weights to ~22 bits: <= 1e-3 vs the fp32 reference on every input
                                * class at ~1.1-1.2x the FP16 time */

#define MOE_PREC_AUTO 4        /* the family's default: MIXED for Net2x/3x/4x and NetDN, FP16 for SEDN, FP16X3 for lite -- the arithmetic that
                                * holds 1e-3 max-abs against the reference's fp32 CPU path on every input class.  What a drop-in caller passes
                                * (INTEGRATION.md section 1): the reference's own dtype policy is one line too (python/imageProcess.py:309-317) */

typedef struct moe_net moe_net;
typedef struct moe_plan moe_plan;

const char* moe_last_error(void);
int moe_abi_version(void);
/* number of visible HIP devices (0 when none); never fails */
int moe_device_count(void);

/* info[0..7] = compute units, max engine clock (kHz), memory clock (kHz), memory bus width (bits), L2 bytes, total memory bytes,
 * wall-clock rate (kHz), LDS bytes per CU -- what bench.py derives the MFMA / HBM peaks of the roofline from
 * (the reference reads its device through NVML, python/readgpu.py; config.py:61-71) */
int moe_device_info(int device, int64_t info[8]);

/* ---- model ------------------------------------------------------------------------------------ */
int moe_net_create(int arch, int scale, moe_net** out);
void moe_net_destroy(moe_net* net);
/* scale factor per side (1 for denoisers) */
int moe_net_scale(const moe_net* net);
/* number of state-dict entries this architecture expects, and the i-th name/shape
 * (shape receives up to 4 dims, *ndim their count) */
int moe_net_num_params(const moe_net* net);
int moe_net_param_info(const moe_net* net, int index, const char** name, int64_t shape[4], int* ndim);
/* one load_state_dict entry: fp32, C-contiguous, host memory; copied */
int moe_net_set_param(moe_net* net, const char* name, const float* data, const int64_t* shape, int ndim);
/* pack + upload weights to HIP device `device`; strict like load_state_dict (every parameter set).
 * May be called again to move / change precision.  precision: MOE_PREC_AUTO for the family's default (what a drop-in caller
 * passes), or a specific arithmetic (MIXED is refused for SEDN / lite, which have no such recipe).  MOE_PREC_AUTO also measures the
 * loaded checkpoint once (moe_net_calibrate below): Net2x/3x/4x and NetDN get their count of split-operand blocks or FP16X3, SEDN
 * keeps FP16 when that holds the contract on these weights and runs in FP16X3 when it does not; lite always runs in FP16X3. */
int moe_net_finalize(moe_net* net, int device, int precision);
/* what `precision` resolves to for this net's family (MOE_PREC_AUTO -> FP16 / FP16X3 / MIXED; anything else -> itself).  After a finalize with MOE_PREC_AUTO:
 * what that finalize settled on for the loaded weights (see moe_net_calibrate). */
int moe_net_resolved_precision(const moe_net* net, int precision);
/* The precision policy for checkpoints the build has never seen (the reference's contract is "load any state dict, get the fp32 answer":
 * python/imageProcess.py:319-334; its own dtype policy is castModel, :309-317).  Net2x/3x/4x and NetDN under MOE_PREC_MIXED run their first `blocks` ARSBs with
 * split operands; how many a checkpoint needs depends on how wide its trunk swings.  moe_net_calibrate measures it on the device: uniform uint8-noise tiles (12 seeds
 * x 3 planes of 256 x 256, the tile size that ships; compared on the device) through the exact arithmetic (FP16X3) and through MIXED with blocks = the architecture's default .. 6.  The worst
 * max-abs difference of that sample times 1.10 -- the inflation observed between such a sample and the worst tile of full frames -- is the PREDICTED worst tile of a
 * full frame; *blocks = the smallest count whose prediction is <= target (target <= 0: 8.5e-4; the architecture's default count is kept up to 5 % above it, so that a
 * zoo key next to the target does not flip with the device or driver), *err = that prediction; *blocks = -1 when six blocks do not reach it (*err = what they reach).
 * The count is kept (moe_net_exact_blocks) until a parameter changes or moe_net_set_exact_blocks overrides it.  moe_net_finalize(MOE_PREC_AUTO) runs this by itself,
 * once per checkpoint, and finalizes in MOE_PREC_FP16X3 when no count reaches the target: a drop-in caller needs no extra line.
 * SEDN (finalized in FP16 or FP16X3) has no count, and a two-way answer: the same sample runs in FP16 -- with the net's current options, as it ships -- and in FP16X3;
 * *err = the worst difference times SEDN's inflation factor (the predicted worst tile of a full frame in FP16), *blocks = 0.  The net keeps the arithmetic it was
 * finalized with; moe_net_finalize(MOE_PREC_AUTO) keeps FP16 while *err <= target x 1.05 (FP16 is the family's default: the same 5 %) and runs the checkpoint in FP16X3
 * otherwise (moe_net_resolved_precision(net, MOE_PREC_AUTO) then says so); option auto_calibrate = 0 keeps FP16 unmeasured.
 * lite: *blocks = 0, *err = 0, nothing is measured (its AUTO arithmetic is the exact mode).
 * Synchronises `stream`; ~0.2-0.4 s.  (moe_net_finalize runs its measurement on a private non-blocking stream.) */
int moe_net_calibrate(moe_net* net, double target, int* blocks, double* err, void* stream);
/* the count of split-operand ARSBs the next forward runs with (0 when the net is not in MOE_PREC_MIXED) */
int moe_net_exact_blocks(const moe_net* net);
/* device bytes of scratch a forward of B planes of h x w needs (allocated lazily, grow-only, owned by the net) */
int64_t moe_net_workspace_bytes(const moe_net* net, int B, int h, int w);
/* largest tile (pixels of one input plane) a forward accepts: the convolution kernels address their tensors with 32-bit byte
 * offsets.  Batches of planes beyond that range are split into several launch sets internally; a single larger plane is
 * refused with MOE_ENOMEM (the planner's "tile does not fit" convention, python/imageProcess.py:58-59). */
int64_t moe_net_max_tile_pixels(const moe_net* net);
/* y[b] = Net(x[b]),  x: B planes of h x w (h, w >= 1), element (b,i,j) at x + x_off[b] + i*sH + j*sW
 * (strides in elements; x_off == NULL means b*sB), dtype MOE_F32/MOE_F16.  y: B contiguous planes of
 * (scale*h) x (scale*w), plane b at y + (y_off ? y_off[b] : b*scale*h*scale*w), dtype MOE_F32/MOE_F16.
 * x_off / y_off are HOST arrays of B element offsets.  Asynchronous on `stream`. */
int moe_net_forward(moe_net* net, const void* x, int x_dtype, int B, int h, int w,
                    int64_t sB, int64_t sH, int64_t sW, const int64_t* x_off,
                    void* y, int y_dtype, const int64_t* y_off, void* stream);
/* moe_net_forward with flags.  MOE_FWD_INPUT_SINCE_PREV: the caller states that x was COMPLETE on `stream` when the previous forward of this net was enqueued on it --
 * true of the reference's tile loop, whose inputs are slices of one padded image that exists before the loop (python/imageProcess.py:157-170: s = x[..., top:bottom,
 * left:right]; r = opt(s); blend; assign).  Small forwards of the SR nets (up to four planes of 256 x 256, no offset tables, option overlap_calls) then alternate between
 * two internal (stream, workspace) sets: forward k+1 starts beside forward k instead of behind it and behind the caller's blend of tile k.  What the caller sees is
 * unchanged: y is written by the forward's LAST kernel, which waits for everything enqueued on `stream` before this call, and `stream` waits for the forward before the
 * call returns, so the next thing the caller enqueues (its blend) finds y complete.  Without the flag, for other shapes / nets, for the first call of a burst (or after
 * a call on another stream) and under stream capture this IS moe_net_forward.  The torch wrapper (moephoto_amd/models.py) sets the flag when x is a view of the same
 * live storage, at the same version counter, as the previous call's input. */
#define MOE_FWD_INPUT_SINCE_PREV 1u
int moe_net_forward_ex(moe_net* net, const void* x, int x_dtype, int B, int h, int w,
                       int64_t sB, int64_t sH, int64_t sW, const int64_t* x_off,
                       void* y, int y_dtype, const int64_t* y_off, void* stream, unsigned flags);
/* Live kernel timing for the roofline report: bracket the MFMA-conv launches of every layer whose key contains one of the
 * comma-separated `layer_substrings` (e.g. "up1,c2_": the 64->256 upsampler convs at 2x resolution, and conv_2 of the ARSBs)
 * with hipEvents on the launch stream.  NULL / "" disables.  moe_net_get_profile_at waits for the recorded events of the
 * index-th substring and returns their summed kernel time, the number of launches and their algorithmic FLOPs
 * (2*pixels*Cout*Cin*taps, real channel counts); moe_net_get_profile = index 0, and resets the recording. */
int moe_net_set_profile(moe_net* net, const char* layer_substrings);
int moe_net_get_profile_at(moe_net* net, int index, double* total_ms, int64_t* launches, double* flops);
int moe_net_get_profile(moe_net* net, double* total_ms, int64_t* launches, double* flops);
/* MOE_PREC_MIXED only: how many leading ARSBs run with split operands (0..6; -1 = the calibrated count of these weights if there is one, else the
 * architecture's default: Net2x 4, Net3x 2, Net4x 1, NetDN 1).  Takes effect at the next forward. */
int moe_net_set_exact_blocks(moe_net* net, int blocks);
/* Kernel-form switches of one net, for A/B measurements and the parity tests that compare forms of one layer in-process.  Every key (the rows of
 * the option table in csrc/options.cpp; defaults and the measurements behind them: NetOptions in csrc/net.h) with its values, the default first:
 *   flags, "1" | "on" | "0" | "off":  "arsb_fuse", "x3_fuse", "exact_fuse", "conv1x1", "up_fuse2", "fuse_tail", "sedn_fuse", "s64", "pool_fuse",
 *       "frm_pre", "stem2", "lite_lut", "k48", "lo8" (fp8 low parts between conv64_q8 layers), "branch_streams", "overlap_calls",
 *       "auto_calibrate"; off by default: "overlap_fork", "calib_log"
 *   "conv_impl" = "sp" | "v1";  "sp_impl" = "auto" | "rw" | "sp";  "up_impl" = "ps4" | "rw";  "tail_split" = "r" | "ru" | "0";
 *   "tail_form" = "sums" | "planes";  "q8_impl" = "s" | "p";  "x3_impl" = "auto" | "x3" | "q8" (the split-operand layers' kernel: three fp16
 *       products, or the two corrections on fp8 operands; auto = q8 for the SR nets and NetDN)
 *   counts, a non-negative integer with 0 = the built-in choice:  "branch_groups", "overlap_groups", "tiles_per_batch", "max_groups"
 *   "dbg" = an integer (timing-ablation bits of the conv kernels: results are wrong when set), "trace_key" = a layer key
 *   "repeat" = "<layer key>:<n>", n >= 1 (measurement: the matching bracketed launches are issued n times -- tools/kernel_power.py); "" | "0" clears
 * A value the key does not have is refused with MOE_EINVAL and leaves the option as it was.
 * Defaults come from the environment variables MOE_<KEY> ONCE, at moe_net_create ("calib_log" and "repeat" have none; a value the option does not
 * have is reported on stderr and ignored); the forward path itself reads no
 * environment.  The reference has no such switches: its forward is torch.nn (python/imageProcess.py:391-395). */
int moe_net_set_option(moe_net* net, const char* key, const char* value);
/* keep fp32 copies of named intermediates during forwards (slow; debugging / layer-by-layer parity only).
 * enable = 0: off.  1 (any other non-zero value): taps, and the forwards leave their fused forms so that every layer has a tensor to tap.
 * 2: taps and nothing else -- no kernel choice changes, the forward is the production one and its result is bit-identical to enable = 0.  MOE_EINVAL for lite.
 *    Net2x / Net3x / Net4x / NetDN: stem, input2, arsb1..6 and the upsampler stages the production form stores (the fused tail leaves none).  A pair of the fp8 low-part
 *    chain is tapped as hi + word 2^-9 and leaves NAME.hi (its fp16 part) and NAME.w8 (its e4m3 words as fp32) beside it; an fp16 pair leaves NAME.hi; block 6 of an SR
 *    net, whose low part is not written, neither.
 *    SEDN: its fused block tail then leaves per block K: bK.rb0, bK.rb2 (fp16 activations), bK.mean (the 256 fp32
 *    channel means, shape (B, 256, 1, 1)), bK.weff (the per-plane 64 x 64 x 9 weights as the fp16 MFMA A fragments lie in memory, shape (B, 72 * 512, 1, 1):
 *    fragment tap * 8 + ks * 2 + nblk, lane l, element e = W_eff[cout 32 nblk + l % 32][cin 16 ks + 8 (l / 32) + e][tap]) and blockK.
 * Where SEDN's forward takes the unfused form (enable = 1; more planes than workgroups; FP16X3) it leaves bK.rb0, bK.rb2, bK.rb4, bK.wtrans (the gated
 * per-plane 1x1 weights in fragment order, shape (B, 64 * 256, 1, 1): fragment (seg * 4 + ks) * 2 + nblk = W[cout 32 nblk + l % 32][cin 64 seg + 16 ks + 8 (l / 32) + e])
 * and blockK.  A tapped SEDN forward drops the taps of the forward before it. */
int moe_net_set_debug(moe_net* net, int enable);
/* copy a named intermediate of the LAST forward to host as fp32 NCHW (debug / layer-by-layer parity);
 * synchronises the stream.  Returns the element count written (<= capacity) or a negative error. */
int64_t moe_net_debug_tap(moe_net* net, const char* tap, float* host, int64_t capacity, int64_t shape[4], void* stream);

/* ---- tile planner (host only, no device needed) ------------------------------------------------ */
/* shape = (C, H, W) of the image as handed to doCrop (before planes-as-batch); ram / ram_coef as in
 * Option.ramCoef & config.calcFreeMem(); cropsize 0 = unlimited */
int moe_plan_create(const int64_t shape[3], double ram, double ram_coef, int pad, int scale, int align,
                    int cropsize, moe_plan** out);
void moe_plan_destroy(moe_plan* plan);
/* info[0..11] = n_tiles, step_h, step_w, out_h, out_w, pad_h_to, pad_w_to, pad_sc, tile_h, tile_w, clip_h, clip_w */
int moe_plan_info(const moe_plan* plan, int64_t info[12]);
/* tiles[k*8 .. k*8+7] = (top, bottom, left, right, topT, leftT, bsc, rsc) in raster order */
int moe_plan_tiles(const moe_plan* plan, int32_t* tiles);
/* blend ramp b[k] = sigmoid(9*(k/padSc - .5)), k < padSc, fp32 */
int moe_plan_ramp(const moe_plan* plan, float* ramp);
/* per tile row i (moe_plan_info: step_h of them) four ints: first output row the tile row writes, first un-blended row S(i) ("solid"), output row of the
 * tiles' own row 0, height of the tiles' output extent -- what the stitch kernel folds with (python/imageProcess.py:120-131,167-170) */
int moe_plan_rows(const moe_plan* plan, int32_t* rows);

/* ---- rounding and ordered dither in the quantising edges (the definition: moephoto_amd/quant.py) -----------------
 * Every edge that turns a float into a sample truncates by default, as the reference does (python/imageProcess.py:245-257: v * 2^bits, clamp, truncate).  These flags are
 * OR-ed into the `bits` argument of moe_to_output, moe_stitch_out, moe_run_plan_out, moe_stitch_mix, moe_run_plan_filter, moe_luma_merge, moe_stitch_luma and
 * moe_run_plan_luma, and into the `depth` argument of moe_stitch_planes, moe_run_plan_planes, moe_stitch_yuv, moe_run_plan_yuv and moe_to_yuv; the low byte keeps its
 * meaning and its checks.  With a mode the sample is trunc(clamp(fl32(fl32(v * S) + T / 128), 0, 2^bits - 1)), NaN = 0, the product and the sum rounded separately:
 *     MOE_Q_ROUND      T = 64: round to nearest (halves up)
 *     MOE_Q_ORDERED    T = 2 * B8[y & 7][x & 7] + 1, B8 the 8 x 8 Bayer matrix, (x, y) the sample's coordinates in the plane or image written; the interleaved channels of
 *                      a pixel share one threshold, a chroma sample uses its chroma-plane coordinates
 *     MOE_Q_UNIT       S = 2^bits - 1 instead of 2^bits: the inverse of moe_to_float's MOE_U8 reader (v / 255), so that exact 8-bit codes come back as they went in
 * In the three *yuv* calls the 16-bit samples stay the truncating quantiser's and the two rounding constants of the integer conversion become thresholds (1 << (37 - D) ->
 * T << (31 - D), 1 << (39 - D) -> T << (33 - D)): MOE_Q_ROUND is then today's frame.  Refused with MOE_EINVAL before any device call: both modes, MOE_Q_UNIT without a
 * mode, MOE_Q_UNIT on a *yuv* call, any flag beside bits = 0 (the canvas forms), any other high bit. */
#define MOE_Q_ROUND 0x100
#define MOE_Q_ORDERED 0x200
#define MOE_Q_UNIT 0x400

/* ---- device-side stitch / whole-image run ------------------------------------------------------ */
/* Fold the per-tile results into the canvas exactly as doCrop's sequential blend does.
 * tiles_dev: device buffer holding every tile's result as C contiguous fp32 planes of
 * ((bottom-top)*scale) x ((right-left)*scale); tile k starts at element tile_off[k] (HOST array; NULL = the
 * default layout of moe_plan_tile_offsets).
 * out: (C, out_h, out_w) contiguous, dtype MOE_F32/MOE_F16. */
int moe_stitch(const moe_plan* plan, int device, const float* tiles_dev, const int64_t* tile_off, int C,
               void* out, int out_dtype, void* stream);
/* The same with the tile offsets already on the device (n_tiles int64 elements): no table upload, no cache lookup --
 * moephoto_amd/dist.py keeps one device table per frame it stitches. */
int moe_stitch_dev(const moe_plan* plan, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C,
                   void* out, int out_dtype, void* stream);
/* One ROW BAND of the canvas: the output rows [S(row0), S(row1)) (S(i) = first un-blended row of tile row i, moe_plan_rows; S(step_h) = out_h) folded
 * from tile rows row0 .. row1 into out = (C, S(row1) - S(row0), out_w).  The band ends with the blend band of tile row row1 (when row1 < step_h);
 * strip != 0: the entries of tile_off_dev for that tile row point at STRIPS -- the pad_sc rows [first, solid) of each plane, C planes of pad_sc x width --
 * instead of whole tiles.  Lets the ranks of a single-frame job each fold their own band of the canvas (moephoto_amd/dist.py: band-sharded stitch;
 * only those strips cross between neighbouring bands), bit-identical to the rows of moe_stitch's canvas. */
int moe_stitch_band(const moe_plan* plan, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C,
                    void* out, int out_dtype, int row0, int row1, int strip, void* stream);
/* The fold of moe_stitch_dev, the rounding of a canvas of `canvas_dtype` (MOE_F16 | MOE_F32) and the quantiser of moe_to_output in ONE pass over the pool: replaces
 * python/imageProcess.py:120-131,167-170 (blend + slice-assign), :238-243 (toFloat) and :245-257 (toOutput) for a caller that only wants the encoder's samples.
 * dst: out_h x out_w x C interleaved, MOE_U8 (bits = 8) or MOE_U16 (bits = 8 | 16), the bytes moe_stitch -> fp32 -> moe_to_output give; tile_off_dev: n_tiles int64
 * on the DEVICE, NULL = the plan's own layout.  C = 1 .. 4, any out_w.  Asynchronous on `stream`; the canvas itself never exists.  bits may carry MOE_Q_ROUND /
 * MOE_Q_ORDERED / MOE_Q_UNIT: the quantiser rounds or dithers at the pixel's coordinates, the bytes of moe_stitch -> moe_to_output with the same flags. */
int moe_stitch_out(const moe_plan* plan, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, int canvas_dtype, int bits,
                   void* dst, int dst_dtype, void* stream);
/* The DN step's edge inside that fold, for plans of scale 1: replaces RGBFilter's passes behind doCrop -- strengthOp's `s * x + (1 - s) * inp` (python/imageProcess.py:562,
 * three elementwise passes) and mergeAlpha's concatenation (:359-366, within RGBFilter :368-377) -- and, with bits != 0, toFloat / toOutput as moe_stitch_out does (:238-257).  Per pixel-plane
 * c = the fold rounded to the canvas dtype T = inp_dtype (MOE_F16 | MOE_F32), then y = T(T(sf * c) + T(tf * inp)) with sf = (float)strength, tf = (float)(1.0 - strength)
 * and every product and the sum formed in fp32 -- the bits torch gives for the expression on device tensors; strength == 1: y = c.  (Where torch's own kernels
 * round an fp16 product once instead of fp32-then-fp16 -- the last partial block of 2048 elements of a dense tensor, every element of a strided view -- so does this
 * one: an inp with unit column stride on a 16-byte aligned base counts as the dense image or its padded copy, any other inp as a strided view.)  inp: the image the net saw, element
 * (c,i,j) at inp + c*sC + i*sH + j*sW (elements; may be a view), read at the output's coordinates; alpha (NULL: none): one more plane of dtype T, element (i,j) at
 * alpha + i*aH + j*aW, copied unchanged behind the C planes.  bits = 0: dst = the canvas (C [+ 1], out_h, out_w) contiguous, dst_dtype = inp_dtype; bits = 8 | 16:
 * dst = out_h x out_w x (C [+ 1]) interleaved samples, MOE_U8 (8) or MOE_U16, as moe_stitch_out writes them; no canvas exists.  C + alpha = 1 .. 4; strength finite;
 * tile_off_dev: on the DEVICE, NULL = the plan's own layout.  Asynchronous on `stream`.  bits = 8 | 16 may carry the MOE_Q_* flags (the sample form's quantiser; alpha is a
 * channel of its pixel and shares the threshold); beside bits = 0 they are refused. */
int moe_stitch_mix(const moe_plan* plan, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C,
                   const void* inp, int inp_dtype, int64_t sC, int64_t sH, int64_t sW, const void* alpha, int64_t aH, int64_t aW,
                   double strength, int bits, void* dst, int dst_dtype, void* stream);
/* The body of the reference's tile loop behind the net call, for a caller that KEEPS that loop -- python/imageProcess.py:167-170:
 *     t = tmp_image[..., top*sc:bsc, left*sc:rsc];  q, _ = blend(*blend(unpad(r), t, topT, padSc, -2, bl.t()), leftT, padSc, -1, bl);  tmp_image[..., bsc-h:bsc, rsc-w:rsc] = q
 * as one kernel, in place on the canvas.  r: the tile result, C planes, element (c,i,j) at r + c*r_sC + i*r_sH + j (its first bsc-top_sc rows and rsc-left_sc
 * columns are used: opt.unpad); canvas: element (c,i,j) at canvas + c*c_sC + i*c_sH + j; (top_sc, left_sc, bsc, rsc, topT, leftT) = the tile tuple of iterClip
 * with top, left already multiplied by the scale; ramp: opt.blend, pad_sc values.  r, canvas and ramp share `dtype` (MOE_F16 on the reference's GPU path, MOE_F32)
 * and live on the device; the arithmetic is the reference's expression b = bx + blend * (b - bx) evaluated in that dtype, operation by operation: the canvas gets
 * the very bits the two torch calls produce.  Asynchronous on `stream`. */
int moe_blend_tile(const void* r, int64_t r_sC, int64_t r_sH, void* canvas, int64_t c_sC, int64_t c_sH, int dtype, int C,
                   int top_sc, int left_sc, int bsc, int rsc, int topT, int leftT, int pad_sc, const void* ramp, void* stream);

/* ---- wire format of tile results between ranks (moephoto_amd/dist.py, wire = 'f16s') ------------------------------------------------
 * The reference has no multi-device code; this belongs to the tile-parallel layer around doCrop (python/imageProcess.py:120-172).  A tile's fp32
 * value is needed exactly only where a blend reads it: in the tile's own blend band and under the blend bands of later tiles (imageProcess.py:
 * 120-131); elsewhere it is rounded to the canvas dtype or overwritten.  moe_plan_seams gives those rows / columns per tile (8 ints: two row ranges,
 * two column ranges, tile-local, half-open); a record then travels as [fp16 image of all values | fp32 seam rows | fp32 seam columns]
 * (moe_wire_words 4-byte words; a record whose seam rows cover it -- a band-mode strip -- is its fp32 values alone).  Unpacked tiles hold the exact
 * fp32 value in the seams and float(half(v)) elsewhere: an fp16 canvas folded from them is bit-identical to the fp32-wire one. */
typedef struct moe_wire_rec {
    int64_t tile_off;                /* fp32 elements into the tile buffer */
    int64_t wire_off;                /* 4-byte words into the wire buffer */
    int32_t C, th, tw;               /* planes, rows, columns of the tile (or strip) */
    int32_t ra0, ra1, rb0, rb1;      /* seam rows [ra0, ra1) and [rb0, rb1), ra1 <= rb0 */
    int32_t ca0, ca1, cb0, cb1;      /* seam columns likewise */
    int32_t reserved;
} moe_wire_rec;
int moe_plan_seams(const moe_plan* plan, int32_t* seams /* n_tiles x 8 */);
int64_t moe_wire_words(const moe_wire_rec* rec);
/* recs_dev: n records on the device; max_elems: the largest C*th*tw among them (sizes the launch). */
int moe_wire_pack(const float* tiles_dev, void* wire_dev, const moe_wire_rec* recs_dev, int n, int64_t max_elems, void* stream);
int moe_wire_unpack(float* tiles_dev, const void* wire_dev, const moe_wire_rec* recs_dev, int n, int64_t max_elems, void* stream);

/* doCrop on device: img = (C, Hp, Wp) planes (already padded per moe_plan_info's pad_*_to, see
 * python wrapper), element (c,i,j) at img + c*sC + i*sH + j*sW; out as in moe_stitch.
 * max_tiles_per_batch <= 0 picks a default. */
int moe_run_plan(moe_net* net, const moe_plan* plan, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                 void* out, int out_dtype, int max_tiles_per_batch, void* stream);

/* General form: `pool` (device, fp32, >= moe_plan_pool_elems) receives the raw per-tile results (NULL: internal);
 * only tiles with raster index k % shard_count == shard_index are computed (tile-parallel sharding across GPUs:
 * the ranks then exchange pool slices, see moephoto_amd/dist.py); do_stitch = 0 skips the final fold. */
int moe_run_plan_ex(moe_net* net, const moe_plan* plan, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                    void* out, int out_dtype, int max_tiles_per_batch, float* pool, int shard_index, int shard_count,
                    int do_stitch, void* stream);

/* doCrop + toFloat + toOutput (python/imageProcess.py:157-172,238-257): moe_run_plan_ex without shard on the plan's internal pool, its final fold replaced by
 * moe_stitch_out.  dst, canvas_dtype, bits (with its MOE_Q_* flags), dst_dtype as there; asynchronous on `stream`. */
int moe_run_plan_out(moe_net* net, const moe_plan* plan, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                     int canvas_dtype, int bits, void* dst, int dst_dtype, int max_tiles_per_batch, void* stream);

/* ---- the encoder's planar Y'CbCr 4:2:0 frame ------------------------------------------------------------
 * The reference fixes the pixel format of its output pipe to bgr24 / bgr48le (python/video.py:24,219,230) and the encoder converts every frame on the CPU.  These
 * entry points write the encoder's own planes instead: limited-range Y'CbCr at `depth` 8 (uint8 planes), 10, 12 or 16 bits (little-endian uint16 planes), 4:2:0 with
 * centre siting, the Y plane (out_h x out_w), then Cb, then Cr (ceil(out_h / 2) x ceil(out_w / 2) each), contiguous -- ffmpeg's rawvideo yuv420p, yuv420p10le,
 * yuv420p12le, yuv420p16le.  Per pixel the three samples are first taken at 16 bits exactly as moe_stitch_out / moe_to_output give them with bits = 16 (the canvas
 * dtype's rounding, * 65536, clamp, truncate, NaN = 0); the integer conversion behind them is defined in moephoto_amd/pixfmt.py (14-bit coefficients, a chroma sample
 * from the sums of its 2 x 2 block, the edge pixel repeated on odd sizes).  Three planes only.  dst: any 2-byte aligned address (any address for depth 8). */
#define MOE_YUV_BT709 0
#define MOE_YUV_BT601 1
#define MOE_YUV_BT2020NC 2
#define MOE_ORDER_BGR 0        /* plane 0 is blue: the video path's frames */
#define MOE_ORDER_RGB 1
/* moe_stitch_out's fold with that frame behind it, for a plan of three planes; tile_off_dev: on the DEVICE, NULL = the plan's own layout.  Asynchronous on `stream`.
 * depth may carry MOE_Q_ROUND (today's bytes) or MOE_Q_ORDERED (the conversion's rounding constants become Bayer thresholds: quant.yuvFromSamples16); MOE_Q_UNIT is refused. */
int moe_stitch_yuv(const moe_plan* plan, int device, const float* tiles_dev, const int64_t* tile_off_dev, int canvas_dtype, int depth, int matrix, int order,
                   void* dst, void* stream);
/* moe_run_plan_out with its final fold replaced by moe_stitch_yuv (depth and its flags as there). */
int moe_run_plan_yuv(moe_net* net, const moe_plan* plan, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                     int canvas_dtype, int depth, int matrix, int order, void* dst, int max_tiles_per_batch, void* stream);

/* ---- chains on the decoder's own Y'CbCr 4:2:0 planes ------------------------------------------------------
 * The reference asks its decoder for bgr24 / bgr48le (python/video.py:24,219) and sends three full planes through the net.  None of the SR / DN nets convolves planes
 * jointly (planes are the batch: python/runSR.py:37-40), so a chain can run on the decoder's planes as they are: Y' as a (1, H, W) image, Cb and Cr as a (2, H / 2, W / 2)
 * image -- half the plane-pixels, no colour matrix at either end, limited range kept as it is.  The definition is moephoto_amd/pixfmt.py (toPlanes / fromPlanes): a value is
 * code * 2^-depth at every depth (8 bits: / 256, so a depth change is a shift and neutral chroma is 0.5), a sample is moe_to_output's quantiser with bits = depth.
 *
 * moe_planes_to_float: src = a planar frame of H x W on the device (uint8 for depth 8, little-endian uint16 for depth 10, 12, 16; the Y plane, then Cb, then Cr; codes
 * are taken as they are, high bits are not masked) -> dst_y = (1, H, W), dst_c = (2, H / 2, W / 2), contiguous, of dst_dtype MOE_F32 (exact) / MOE_F16 (rounded to
 * nearest even), in one launch.  H and W even, 2 at least; src 2-byte aligned for depth > 8 (16-byte aligned is the fast path). */
int moe_planes_to_float(const void* src, int depth, int H, int W, void* dst_y, void* dst_c, int dst_dtype, int device, void* stream);
/* moe_stitch_out's fold with a planar result at `depth` 8, 10, 12 or 16: dst = C (1 .. 4) planes of out_h x out_w samples, plane c at dst + c * out_h * out_w elements,
 * uint8 for depth 8, else uint16 -- per sample the bytes moe_stitch -> moe_to_output(H = C * out_h, W = out_w, C = 1, bits = depth) give, and for C = 1 at depth 8 or 16
 * those of moe_stitch_out.  dst: any 2-byte aligned address (any address for depth 8) -- the Cb plane of a frame starts wherever its Y plane ends.  tile_off_dev: on the
 * DEVICE, NULL = the plan's own layout.  Asynchronous on `stream`.  depth may carry MOE_Q_ROUND / MOE_Q_ORDERED / MOE_Q_UNIT: each sample is rounded or dithered at its
 * coordinates in its OWN plane (the bytes of moe_stitch -> one flagged moe_to_output per plane). */
int moe_stitch_planes(const moe_plan* plan, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, int canvas_dtype, int depth,
                      void* dst, void* stream);
/* moe_run_plan_out with its final fold replaced by moe_stitch_planes (C = the plan's planes; depth and its flags as there). */
int moe_run_plan_planes(moe_net* net, const moe_plan* plan, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                        int canvas_dtype, int depth, void* dst, int max_tiles_per_batch, void* stream);

/* The chroma planes of a LUMA-ONLY chain: the net runs on Y' alone and Cb / Cr are brought to the new size by a fixed resampling filter, in integers -- the definition
 * is moephoto_amd/pixfmt.py (chromaTable, resampleChroma) and the device matches it byte for byte.  src = two planes of h x w codes, one after the other (uint8 at
 * depth 8, little-endian uint16 at 10, 12, 16; high bits are not masked); dst = two planes of h * scale x w * scale at dst_depth, likewise.  Any 2-byte aligned
 * address (any address at depth 8): the Cb plane of a frame starts wherever its Y plane ends.  cx / ox and cy / oy are HOST tables, per axis scale x taps 14-bit
 * coefficients and scale offsets: output index o = q * scale + p reads the source samples clamp(q + off[p] + j, 0, n - 1), j < taps (1, 2 or 4).  Row pass in int32,
 * column pass in int64, sample = clamp((v + 2^27) >> 28, 0, 2^src_depth - 1), then << (dst_depth - src_depth) or >> (src_depth - dst_depth).  Refused (MOE_EINVAL,
 * before any device call): a NULL pointer, a depth outside {8, 10, 12, 16}, h, w or scale below 1, scale above 16, taps outside {1, 2, 4}, a misaligned pointer, a
 * coefficient row that does not sum to 2^14 or whose sum of magnitudes exceeds 32767 (so the int32 row pass holds for any uint16 code), an offset outside [-2, 1].
 * Asynchronous on `stream`. */
int moe_chroma_resample(const void* src, int src_depth, int h, int w, void* dst, int dst_depth, int scale, int taps,
                        const int16_t* cx, const int8_t* ox, const int16_t* cy, const int8_t* oy, int device, void* stream);

/* The same planes steered by the finished luma: a joint bilateral filter, in integers -- the definition is moephoto_amd/pixfmt.py (guidedTable, guidedRange, lumaGuide,
 * guidedChroma) and the device matches it byte for byte.  src_c = the two planes of h x w chroma codes of the SOURCE frame and src_y its 2 h x 2 w luma plane, at
 * src_depth; dst_c = two planes of h * scale x w * scale at dst_depth, written; dst_y = the OUTPUT frame's luma plane, 2 h * scale x 2 w * scale at dst_depth, read
 * as the chain wrote it.  Any 2-byte aligned address (any address at depth 8).  loc sites the horizontal axis of the guide (the tables carry the filter's own siting).
 * cx / ox and cy / oy are HOST tables, per axis scale x 4 8-bit coefficients and scale offsets: output index o = q * scale + p reads the source samples
 * clamp(q + off[p] + j, 0, n - 1), j < 4; range64 = 64 range weights.  Per sample w = cy cx range64[min(|GH - GL| >> 10, 63)] over the 16 taps,
 * s = (sum w code + den / 2) / den with den = sum w, then << (dst_depth - src_depth) or >> (src_depth - dst_depth).  Refused (MOE_EINVAL, before any device call): a
 * NULL pointer, a depth outside {8, 10, 12, 16}, h or w below 1 or sizes beyond int, scale outside 2 .. 16, an unknown loc, a misaligned pointer, a coefficient row
 * that does not sum to 256, an offset outside [-2, 1], a range table with a zero entry, a dst_c that overlaps dst_y.  Asynchronous on `stream`. */
#define MOE_CHROMA_CENTER 0
#define MOE_CHROMA_LEFT 1
int moe_chroma_guided(const void* src_c, const void* src_y, int src_depth, int h, int w, void* dst_c, const void* dst_y, int dst_depth, int scale, int loc,
                      const uint8_t* cx, const int8_t* ox, const uint8_t* cy, const int8_t* oy, const uint8_t* range64, int device, void* stream);

/* RGB frames from a chain on 4:2:0 planes: the integer Y'CbCr -> RGB edge -- the definition is moephoto_amd/pixfmt.py (toRGB, rgbCoefficients) and the device matches it
 * byte for byte.  src = a planar frame of H x W at `depth` (uint8 at depth 8, little-endian uint16 at 10, 12, 16; the Y plane, then Cb, then Cr; high bits are not masked);
 * dst = H x W x 3 interleaved samples, uint8 for bits = 8, uint16 for bits = 16, red first for MOE_ORDER_RGB, blue first for MOE_ORDER_BGR.  Per pixel the chroma
 * planes are brought to luma size by moe_chroma_resample's filter at scale 2 (cx / ox and cy / oy: HOST tables of 2 x taps 14-bit coefficients and 2 offsets per axis,
 * pixfmt.chromaTable; the sample clamped to [0, 2^depth - 1]) -- the upsampled planes never exist in memory -- then y = Y - (16 << (depth - 8)), u = Cb' - (128 << (depth - 8)),
 * v = Cr' - (128 << (depth - 8)) and, with coef = (cY, cRV, cGU, cGV, cBU) = pixfmt.rgbCoefficients(matrix, depth, bits), 20 fractional bits, in int64:
 *     R = (cY y + cRV v + r) >> 20      G = (cY y + cGU u + cGV v + r) >> 20      B = (cY y + cBU u + r) >> 20      each clamped to [0, 2^bits - 1]
 * r = 1 << 19, or with MOE_Q_ORDERED in `bits` T << 13 (T of the pixel's coordinates, shared by its three samples: moephoto_amd/quant.py); MOE_Q_ROUND is accepted and
 * changes nothing.  One launch.  Refused (MOE_EINVAL, before any device call): a NULL pointer, a depth outside {8, 10, 12, 16}, bits outside {8, 16}, MOE_Q_UNIT or any
 * other high bit, an odd H or W, one below 2, H * W * 3 beyond int, an unknown matrix or order, taps outside {1, 2, 4}, a misaligned pointer, a coefficient row that
 * does not sum to 2^14 or whose sum of magnitudes exceeds 32767, an offset outside [-2, 1], cY outside [1, 2^30] or another constant whose magnitude exceeds 2^30
 * (the three products and r then stay below 2^49 for any uint16 code and the shifted sum fits an int), a dst that overlaps src.  Asynchronous on `stream`. */
int moe_planes_to_rgb(const void* src, int depth, int H, int W, void* dst, int bits, int matrix, int order, int taps,
                      const int16_t* cx, const int8_t* ox, const int16_t* cy, const int8_t* oy, const int32_t* coef, int device, void* stream);

/* ---- luma-only steps on RGB images ------------------------------------------------------------------------
 * The reference sends every plane of a colour image through the net (planes are the batch: python/runSR.py:37-40); none of these entry points has a counterpart in
 * it.  None of the SR / DN nets convolves planes jointly, so a step may run on Y' alone while Cb / Cr go to the output's size through moe_resize: a third of the net's
 * work.  The definition is moephoto_amd/luma.py (lumaCoefficients, lumaSplit, lumaMerge): full range, no offset, all arithmetic fp32 with every product and every sum
 * rounded separately in the written order (no FMA); the device matches it bit for bit (NaN payloads aside).  matrix MOE_YUV_BT709 / BT601 / BT2020NC gives the constants
 * kr, kg = 1 - kr - kb, kb, ib = 1 / (2 (1 - kb)), ir = 1 / (2 (1 - kr)), eb = 2 (1 - kb), er = 2 (1 - kr), gr = kr er / kg, gb = kb eb / kg, each computed in double and
 * rounded once; order says whether plane 0 is blue (MOE_ORDER_BGR) or red.  T = dtype, MOE_F16 / MOE_F32.
 *
 * moe_luma_split replaces handing the whole image to the net: img = (C = 3 | 4, H, W) of T, element (c, i, j) at img + c sC + i sH + j sW (strides in elements) ->
 * dst_y = (C - 2, H, W) dense of T: y = (kr r + kg g) + kb b rounded to T, and behind it the fourth plane (alpha) unchanged, as the reference's SR path sends it through
 * the net; dst_c = (2, H, W) dense fp32: cb = (b - y) ib, cr = (r - y) ir from the unrounded y.  One launch.  Refused (MOE_EINVAL, before any device call): a NULL
 * pointer, C outside {3, 4}, a dtype other than MOE_F16 / MOE_F32, a size below 1, an unknown matrix / order, a pointer not aligned to its elements. */
int moe_luma_split(const void* img, int dtype, int C, int64_t sC, int64_t sH, int64_t sW, int H, int W, int matrix, int order, void* dst_y, void* dst_c,
                   int device, void* stream);
/* moe_luma_merge replaces nothing of the reference's (it has no merge): y = (C - 2, H, W) dense of T (Y', alpha), c = (2, H, W) dense fp32 (Cb, Cr), C = 3 | 4 the planes
 * written.  y' = fp32(T(Y')), r' = y' + er cr, b' = y' + eb cb, g' = y' - (gr cr + gb cb), each rounded to T, planes in `order`, alpha behind them unchanged.
 * bits = 0: dst = the canvas (C, H, W) of dst_dtype = dtype; bits = 8 | 16: dst = (H, W, C) interleaved MOE_U8 / MOE_U16 samples, each value through moe_to_output's
 * quantiser.  Serves the chains whose Y' is a canvas (an ensemble, a blended DN, a step that is not last).  Refused as above, and: unknown bits, a dst_dtype that does
 * not fit them.  bits = 8 | 16 may carry the MOE_Q_* flags (the sample form's quantiser at pixel (i % W, i / W)); beside bits = 0 they are refused. */
int moe_luma_merge(const void* y, int dtype, const void* c, int C, int H, int W, int matrix, int order, int bits, void* dst, int dst_dtype, int device, void* stream);
/* moe_stitch_luma replaces moe_stitch -> moe_luma_merge (same bytes): the fold of a pool of P = 1 (Y') or 2 (Y', alpha) planes with the merge as its edge, so the Y'
 * canvas never exists.  c = (2, out_h, out_w) dense fp32; dst and bits as moe_luma_merge's with C = P + 2 and T = canvas_dtype.  tile_off_dev: on the DEVICE, NULL =
 * the plan's own layout.  Refused as above, and: P outside {1, 2}.  Asynchronous on `stream`.  bits and its MOE_Q_* flags as moe_luma_merge's. */
int moe_stitch_luma(const moe_plan* plan, int device, const float* tiles_dev, const int64_t* tile_off_dev, int P, int canvas_dtype, const void* c, int matrix, int order,
                    int bits, void* dst, int dst_dtype, void* stream);
/* moe_run_plan_luma replaces moe_run_plan (or moe_run_plan_out) on the three colour planes: moe_run_plan on img_y (the plan's 1 or 2 planes, padded where the plan
 * pads) with its final fold replaced by moe_stitch_luma (bits and its MOE_Q_* flags as there). */
int moe_run_plan_luma(moe_net* net, const moe_plan* plan, const void* img_y, int dtype, int64_t sC, int64_t sH, int64_t sW, const void* c, int matrix, int order,
                      int bits, void* dst, int dst_dtype, int max_tiles_per_batch, void* stream);

/* Planes of codes brought to a FITTED size: a rational (any n -> m) integer polyphase filter per axis, antialiasing where the axis shrinks -- the definition is
 * moephoto_amd/pixfmt.py (fitTable, fitPlanes) and the device matches it byte for byte.  A handle holds one geometry: `planes` (1 .. 4) planes of h x w codes at
 * src_depth -> as many planes of oh x ow at dst_depth (uint8 at depth 8, little-endian uint16 at 10, 12, 16; high bits are not masked), planes one after the other.
 * cx / ox and cy / oy are HOST tables, per axis m x taps 14-bit coefficients and m offsets (m = ow or oh): output index o reads the source samples
 * clamp(off[o] + j, 0, n - 1), j < taps (1 .. 16).  Row pass in int32, column pass in int64, sample = clamp((v + 2^27) >> 28, 0, 2^src_depth - 1), then
 * << (dst_depth - src_depth) or >> (src_depth - dst_depth).  Refused (MOE_EINVAL, before any device call): a NULL pointer, a depth outside {8, 10, 12, 16}, planes outside
 * 1 .. 4, a size below 1 or beyond int, taps outside 1 .. 16, a coefficient row that does not sum to 2^14 or whose sum of magnitudes exceeds 32767 (so the int32 row pass
 * holds for any uint16 code), an offset whose taps do not reach the plane (off + taps - 1 < 0 or off > n - 1), offsets that decrease along the axis, and offsets that
 * step so far that the source window of the smallest output tile does not fit the kernel's LDS.  The tables are then uploaded to `device` (synchronously) and stay
 * there until the handle is destroyed. */
typedef struct moe_fit moe_fit;
int moe_fit_create(int planes, int src_depth, int64_t h, int64_t w, int dst_depth, int64_t oh, int64_t ow, int taps_x, const int16_t* cx, const int32_t* ox,
                   int taps_y, const int16_t* cy, const int32_t* oy, int device, moe_fit** out);
/* The same filter on ONE INTERLEAVED image (bgr24 / bgr48le frames, RGBA arrays): src = h x w pixels of `channels` (1 .. 4) codes each, dst = oh x ow pixels of as many;
 * the definition is pixfmt.fitPixels = fitPlanes on each channel.  The tables are moe_fit_create's, per PIXEL (m = ow or oh rows); the handle is of the same type and
 * moe_fit_run / _info / _destroy serve it (info[3] = channels).  The kernel's tile is info[0] ELEMENTS wide, so it may end inside a pixel.  Refused (MOE_EINVAL, before any
 * device call): everything moe_fit_create refuses, channels outside 1 .. 4, and a row of w or ow pixels whose elements do not fit an int. */
int moe_fit_create_px(int channels, int src_depth, int64_t h, int64_t w, int dst_depth, int64_t oh, int64_t ow, int taps_x, const int16_t* cx, const int32_t* ox,
                      int taps_y, const int16_t* cy, const int32_t* oy, int device, moe_fit** out);
/* One resample with the handle's geometry, asynchronous on `stream`.  src / dst: any 2-byte aligned address (any address at depth 8) -- the Cb plane of a frame starts
 * wherever its Y plane ends.  Refused: a NULL pointer, a misaligned one. */
int moe_fit_run(const moe_fit* fit, const void* src, void* dst, void* stream);
/* info[0 .. 4) = the kernel's output tile (width, height), the LDS bytes of a workgroup, the planes (moe_fit_create_px: the channels). */
int moe_fit_info(const moe_fit* fit, int64_t info[4]);
void moe_fit_destroy(moe_fit* fit);

/* ---- the 3D LUT colour step ---------------------------------------------------------------------------------
 * The reference's "Retouch" transform (python/AiLUT.py -> site-packages/ailut/csrc/ailut_transform_cuda.cu, the CPU twin ailut_transform_cpu.cpp:20-113): per pixel a
 * trilinear lookup in a 3D table whose lattice has non-uniform intervals.  The definition is moephoto_amd/lut3d.py (transform, apply) and the device matches it byte
 * for byte: i_c = clamp(lower_bound(v_c, x_c) - 1, 0, d - 2), t_c = (x_c - v_c[i]) / ((v_c[i + 1] - v_c[i]) + 1e-10f), eight three-factor weights, eight products
 * summed left to right in the order 000, 100, 010, 110, 001, 101, 011, 111 -- every operation rounded to fp32 on its own.  Values outside the vertices extrapolate.
 * moe_lut3d_create: table_host = float (3, d, d, d) indexed [c][b][g][r], red fastest (the reference's luts[0]); vertices_host = float (3, d), non-decreasing per row
 * (its vertices[0]); both on the HOST, copied: the device keeps one 16-byte entry {R, G, B, 0} per lattice point.  Refused (MOE_EINVAL, before any device call): a NULL
 * pointer, d outside 2 .. 65, a table or vertex value that is not finite, a vertex below the one before it. */
typedef struct moe_lut3d moe_lut3d;
int moe_lut3d_create(int d, const float* table_host, const float* vertices_host, int device, moe_lut3d** out);
/* One frame, one launch, asynchronous on `stream`.  src = H x W x 3 interleaved samples on the device, uint8 (src_bits 8: x = code / 255) or uint16 (16: x = code 2^-16);
 * dst = as many samples, uint8 for bits = 8, uint16 for bits = 16; red first for MOE_ORDER_RGB, blue first for MOE_ORDER_BGR, on both sides.  y = the transform of x;
 * with strength s != 1 y = fl32(fl32(s y) + fl32(fl32(1 - s) x)) (moe_stitch_mix's blend); then the chain's quantiser: bits may carry MOE_Q_ROUND / MOE_Q_ORDERED /
 * MOE_Q_UNIT, thresholds at the pixel's coordinates, its three samples sharing one.  Refused (MOE_EINVAL, before any device call): a NULL pointer, src_bits or bits
 * outside {8, 16}, unknown or contradictory MOE_Q_* flags, MOE_Q_UNIT without a mode, H or W below 1, 3 H W beyond int, an unknown order, a strength that is not
 * finite, a misaligned pointer to 16-bit samples, a dst that overlaps src. */
int moe_lut3d_run(const moe_lut3d* lut, const void* src, int src_bits, int H, int W, void* dst, int bits, int order, float strength, void* stream);
/* info[0 .. 4) = d, the bytes of the device's table, the LDS bytes of a workgroup (the vertices), the pixels a thread owns. */
int moe_lut3d_info(const moe_lut3d* lut, int64_t info[4]);
void moe_lut3d_destroy(moe_lut3d* lut);
/* The handle's table back on the HOST in moe_lut3d_create's layout: table_host = float (3, d, d, d), vertices_host = float (3, d).  Synchronises `stream`.  For a
 * caller that wants the table a generator wrote for a frame (as a .cube file: moephoto_amd/lut3d.py, formatCube), and for tests.  Refused: a NULL pointer. */
int moe_lut3d_read(const moe_lut3d* lut, float* table_host, float* vertices_host, void* stream);

/* ---- the AiLUT generator net --------------------------------------------------------------------------------
 * The other half of the reference's "Retouch": the net that looks at a 256 x 256 thumbnail of the frame and writes the frame's own table and vertices
 * (python/AiLUT.py:167-181 AiLUT.forward up to ailut_transform: F.interpolate, :26-46 TPAMIBackbone(extra_pooling=True), :57-80 LUTGenerator, :82-121 AdaInt; the
 * AiLUT_sRGB_3 / AiLUT_XYZ_3 rows of python/dehaze.py:27-28).  The definition is moephoto_amd/ailut.py (thumbnail, generate); the device computes it in fp32 with
 * fp64 statistics (the reference: fp16 autocast), eight launches a frame, no atomics: two runs on the same input give the same bits.
 * moe_ailut_create .. moe_ailut_finalize are shaped as moe_net's loader (AiLUT(n_ranks, n_vertices) and load_state_dict, python/imageProcess.py:319-328):
 * d = n_vertices (2 .. 65), ranks = n_ranks (1 .. 8); the names are the reference's state-dict keys (backbone.{0..4}.0.weight|bias, backbone.{0..3}.2.weight|bias,
 * lut_generator.weights_generator.weight|bias, lut_generator.basis_luts_bank.weight, adaint.intervals_generator.weight|bias); data is fp32, C-contiguous, on the
 * HOST, copied.  Refused (MOE_EINVAL, before any device call): a NULL pointer, d or ranks outside their range, an index outside the list, an unknown name, another
 * shape than the generator's, a value that is not finite; MOE_ESTATE: a finalize with a parameter unset. */
typedef struct moe_ailut moe_ailut;
int moe_ailut_create(int d, int ranks, moe_ailut** out);
int moe_ailut_num_params(const moe_ailut* g);
int moe_ailut_param_info(const moe_ailut* g, int index, const char** name, int64_t shape[4], int* ndim);
int moe_ailut_set_param(moe_ailut* g, const char* name, const float* data, const int64_t* shape, int ndim);
/* uploads the parameters and allocates the workspace (about 2.7 MB beside the parameters) on `device`; may be called again after a parameter changed: the earlier
 * device block is freed behind a synchronise of its device, so runs still in flight finish on it (moe_ailut_destroy likewise) */
int moe_ailut_finalize(moe_ailut* g, int device);
/* One frame: thumbnail, five conv blocks, the heads, the table -- eight launches, asynchronous on `stream`, no host round trip.  src = H x W x 3 interleaved samples
 * on the device as moe_lut3d_run reads them (uint8 for src_bits 8, uint16 for 16; red first for MOE_ORDER_RGB, blue first for MOE_ORDER_BGR), left untouched.
 * lut = a moe_lut3d of the same d on the same device: its table and vertices are OVERWRITTEN (the const is the host object's), so a moe_lut3d_run queued behind
 * this call on the same stream applies this frame's table.  The handle owns one workspace: its runs belong on one stream at a time.  Refused (before any device
 * call): a NULL pointer, a generator that is not finalized (MOE_ESTATE), a table handle of another d or on another device, src_bits outside {8, 16}, H or W below 1,
 * 3 H W beyond int, an unknown order, a misaligned pointer to 16-bit samples. */
int moe_ailut_run(const moe_ailut* g, const void* src, int src_bits, int H, int W, int order, const moe_lut3d* lut, void* stream);
/* MEASUREMENT ONLY, not for callers (tools/ailut_bench.py): launch `stage` of moe_ailut_run alone (0 the thumbnail, 1 .. 5 the conv blocks, 6 the heads, 7 the table) */
int moe_ailut_stage(const moe_ailut* g, int stage, const void* src, int src_bits, int H, int W, int order, const moe_lut3d* lut, void* stream);
/* moe_ailut_run's first launch alone: dst = float (3, 256, 256) RGB planes on the device (ailut.thumbnail).  It has no handle, so it takes
 * the device as moe_to_float does.  Refusals as moe_ailut_run's, and a dst off 4 bytes or a negative device. */
int moe_ailut_thumbnail(const void* src, int src_bits, int H, int W, int order, float* dst, int device, void* stream);
/* TESTS ONLY, not for callers: *bad = how many bytes of the guard bands between the handle's device buffers no longer hold their pattern, plus how many parameters differ from the host's
 * copies (0 for an intact handle).  Synchronises `stream`.  For tests. */
int moe_ailut_guards(const moe_ailut* g, int64_t* bad, void* stream);
void moe_ailut_destroy(moe_ailut* g);

/* The whole DN step (procDN: python/procedure.py:52-55 -> RGBFilter, python/imageProcess.py:350-377,562): moe_run_plan on the plan's internal pool with its final fold
 * replaced by moe_stitch_mix.  img: the colour planes doCrop would be handed, already padded where the plan pads; the blend reads its top-left out_h x out_w region.
 * alpha, strength, bits (with its MOE_Q_* flags), dst, dst_dtype as in moe_stitch_mix with C = the plan's planes and T = img_dtype.  Asynchronous on `stream`. */
int moe_run_plan_filter(moe_net* net, const moe_plan* plan, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                        const void* alpha, int64_t aH, int64_t aW, double strength, int bits, void* dst, int dst_dtype,
                        int max_tiles_per_batch, void* stream);

/* Multi-frame, owner-sharded form of the tile loop (the multi-GPU step of moephoto_amd/dist.py; the reference runs frames one
 * after the other through doCrop, python/video.py:349-360 -> python/imageProcess.py:157-172).  `imgs` holds n_frames equally
 * shaped padded images, frame f at imgs + f*frame_stride elements; frame f's raw tile results go to pools + f*pool_stride
 * (fp32 elements, >= moe_plan_pool_elems each).  Only pairs with (f * n_tiles + k) % owner_count == owner_index are
 * computed; same-shaped tiles of different frames share launches.  No stitch: exchange, then moe_stitch per frame. */
int moe_run_plan_frames(moe_net* net, const moe_plan* plan, const void* imgs, int img_dtype, int64_t frame_stride,
                        int64_t sC, int64_t sH, int64_t sW, int n_frames, float* pools, int64_t pool_stride,
                        int owner_index, int owner_count, int max_tiles_per_batch, void* stream);
/* The same tile loop with an explicit destination per (frame, tile): tile k of frame f is computed iff
 * tile_dst[f * n_tiles + k] >= 0 and its C result planes go to dst + tile_dst[f * n_tiles + k] (fp32 elements; HOST table).
 * dist.py points the entries straight into its all-to-all send buffer (tiles another rank stitches) and into the stitch
 * buffer (tiles this rank stitches itself), so nothing is copied between the net, the collective and moe_stitch. */
int moe_run_plan_tiles(moe_net* net, const moe_plan* plan, const void* imgs, int img_dtype, int64_t frame_stride,
                       int64_t sC, int64_t sH, int64_t sW, int n_frames, float* dst, const int64_t* tile_dst,
                       int max_tiles_per_batch, void* stream);
/* elements of the fp32 tile pool for C planes, and the element offset of every tile inside it (default layout:
 * tile k = C contiguous planes of its HR extent, tiles in raster order) */
int64_t moe_plan_pool_elems(const moe_plan* plan, int C);
int moe_plan_tile_offsets(const moe_plan* plan, int C, int64_t* off);

/* ---- reuse between the frames of a stream ------------------------------------------------------------------
 * The reference computes every tile of every frame (python/video.py:349-360 -> python/imageProcess.py:157-172).  A tile's result depends on its own input rectangle
 * alone, so a stream may keep each step's tile pool, run the tiles whose input changed and fold the whole pool as always: the same bytes (DESIGN.md section 14;
 * moephoto_amd/reuse.py holds the rules, procedure.genFrameStream(reuse=True) the wiring).
 *
 * moe_changed_blocks: cur and prev each hold n dense byte matrices of rows x row_bytes, one after the other, on the device; map (device, ceil(rows / block_rows) x
 * ceil(row_bytes / block_bytes) bytes, row-major, every byte written) gets map[i][j] = 1 iff some byte of block (i, j) -- block_rows x block_bytes, clipped at the
 * bottom and right edges -- differs between cur and prev in any of the n matrices, else 0.  The same pass copies cur into prev: afterwards prev holds cur's bytes.  Bytes
 * are compared, so NaN patterns and -0 need no special case.  One launch; 16-byte loads when cur, prev, row_bytes and block_bytes are multiples of 16, single bytes
 * otherwise.  An interleaved bgr24 / bgr48le frame is one matrix with block_bytes = 16 * 3 * sample size, a planar frame's Y plane one matrix, its Cb and Cr planes
 * n = 2 matrices folded into one map.  Refused before any device call: a NULL pointer, n, rows, row_bytes or a block size below 1, cur == prev, overlapping cur / prev,
 * a map of more than 2^31 - 1 cells.  Asynchronous on `stream`. */
int moe_changed_blocks(const void* cur, void* prev, int n, int rows, int64_t row_bytes, int block_rows, int block_bytes, uint8_t* map, int device, void* stream);
/* moe_run_plan_ex(.., pool, 0, 1, do_stitch = 0, ..) for the tiles of a mask: tile k is computed iff run[k] != 0 (HOST array of n_tiles bytes) and its C planes go to
 * pool + moe_plan_tile_offsets(plan, C)[k], the plan's own layout -- every moe_stitch* then takes the pool with tile_off_dev = NULL; nothing else in pool is touched.
 * An all-ones mask launches exactly what moe_run_plan_ex launches, an all-zero mask nothing.  The call's offset tables do not go through the cache that serves
 * moe_run_plan_tiles (a new mask per frame would cost it a synchronise, a free, an allocation and a blocking copy per call): they travel through a ring of 32 device
 * buffers the plan owns, filled with hipMemcpyAsync from pinned memory on `stream`, a buffer taken again only behind the event recorded after the launch sets that
 * read it.  After the first call on a plan nothing is allocated or freed; the host waits only when it is 32 calls ahead of the device.  Asynchronous on `stream`. */
int moe_run_plan_subset(moe_net* net, const moe_plan* plan, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW, const uint8_t* run /* n_tiles, HOST */,
                        float* pool, int max_tiles_per_batch, void* stream);

/* ---- self-ensemble ------------------------------------------------------------------------------ */
/* The reference's ensemble (python/imageProcess.py:563-572) with runSR.sr's average (python/runSR.py:26):
 *     v = doCrop(opt, x);  for i < n: v = v + transInv[i](doCrop(opt, trans[i](x)));  v / (n + 1)
 * Symmetry index sym = 0..6 follows the `trans` list (python/imageProcess.py:563-569): transpose, flip, flip2, flip.transpose, transpose.flip,
 * transpose.flip.transpose, flip2.transpose ("a.b" applies a first; flip reverses the width, flip2 width and height).
 *
 * moe_sym_pad: dst = padImage(trans[sym](src)) in one pass -- trans[i](x) (python/imageProcess.py:570) and the right / bottom padding doCrop applies to its input
 * (getPad, python/imageProcess.py:47-56, 160: per axis a reflection with the edge not repeated, up to len - 1 samples, then zeros).  src: C planes of H x W, element
 * (c,i,j) at src + c*sC + i*sH + j*sW (strides in elements); dst: C contiguous planes of Hp x Wp, Hp >= Ht and Wp >= Wt with (Ht, Wt) = (W, H) for the symmetries
 * that transpose (0, 3, 4, 6) and (H, W) otherwise; Hp == Ht and Wp == Wt: a pure transform.  Values are copied, never converted (dtype MOE_F32 / MOE_F16). */
int moe_sym_pad(const void* src, int dtype, int C, int H, int W, int64_t sC, int64_t sH, int64_t sW,
                int sym, void* dst, int Hp, int Wp, int device, void* stream);
/* moe_sym_fold: acc <- acc + transInv[sym](t) in place -- one step of `v + transInv[i](..)` (python/imageProcess.py:571).  acc: C contiguous planes of H x W;
 * t: C contiguous planes of Ht x Wt, the canvas doCrop returned for the transformed image; both of `dtype`.  Each element is formed as torch forms `v + view` in that
 * dtype: operands widened to fp32, added once, rounded once.  final_div = n + 1 > 1 also applies the closing `/ (n + 1)` of python/runSR.py:26 to the freshly rounded
 * sum, with the bits torch produces for tensor / python_int in that dtype; 0 or 1: no division. */
int moe_sym_fold(void* acc, const void* t, int dtype, int C, int H, int W, int sym, int final_div,
                 int device, void* stream);
/* The whole of sr(opt)(x) for ensemble = n_sym (0..7; python/runSR.py:26 around python/imageProcess.py:563-572) on the device: img is the UNPADDED (C, H, W) image with
 * element strides, plan the plan of (C, H, W), plan_t the plan of (C, W, H) (may be NULL for n_sym == 0 only: symmetry 0 transposes), out = (C, out_h, out_w) of plan.
 * Pads with the identity and runs moe_run_plan into out; then per symmetry: pad, moe_run_plan with the matching plan into a scratch canvas, fold into out, the last
 * fold dividing by n_sym + 1 (n_sym == 0: nothing is divided).  The two scratch buffers belong to the net and only grow (a growth waits for `stream`, as the tile pool's
 * does); otherwise everything is asynchronous on `stream`.  Plans whose output shapes are not each other's transpose are refused.  The caller's current device is restored. */
int moe_run_plan_ens(moe_net* net, const moe_plan* plan, const moe_plan* plan_t, int n_sym,
                     const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                     void* out, int out_dtype, int max_tiles_per_batch, void* stream);

/* ---- image I/O edges ---------------------------------------------------------------------------- */
/* src: H x W x C interleaved MOE_U8 (v/255) or MOE_U16 (v/2^bits); dst: C planes H x W, MOE_F32/MOE_F16 */
int moe_to_float(const void* src, int src_dtype, int bits, int H, int W, int C, void* dst, int dst_dtype, int device, void* stream);
/* src: C planes H x W (MOE_F32/MOE_F16); dst: H x W x C interleaved, v*2^bits clamped to [0, 2^bits-1], truncated.  bits may carry MOE_Q_ROUND / MOE_Q_ORDERED / MOE_Q_UNIT
 * (above): the rounding or ordered-dither quantiser, the threshold of pixel (x, y) shared by its C channels. */
int moe_to_output(const void* src, int src_dtype, int H, int W, int C, int bits, void* dst, int dst_dtype, int device, void* stream);
/* src: three planes H x W (MOE_F32/MOE_F16); dst: the Y'CbCr 4:2:0 frame of moe_stitch_yuv, from the samples moe_to_output gives with bits = 16; depth and its flags
 * (MOE_Q_ROUND, MOE_Q_ORDERED) as moe_stitch_yuv's */
int moe_to_yuv(const void* src, int src_dtype, int H, int W, int depth, int matrix, int order, void* dst, int device, void* stream);

/* the pipeline's `resize` step: resizeByTorch = F.interpolate(x[None], size=(h, w), mode, align_corners=False)
 * (python/imageProcess.py:174-195, 555-556; python/procedure.py:104-107).  src: C planes H x W, dst: C planes h x w, same dtype
 * (MOE_F32 / MOE_F16); arithmetic in fp32 in torch's operation order. */
#define MOE_RESIZE_NEAREST 0
#define MOE_RESIZE_BILINEAR 1
#define MOE_RESIZE_BICUBIC 2
int moe_resize(const void* src, void* dst, int dtype, int C, int H, int W, int h, int w, int mode, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOEPHOTO_AMD_H */
