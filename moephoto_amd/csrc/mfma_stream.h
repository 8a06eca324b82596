// mfma_stream.h -- the compile-time machinery the register-weight kernels share (conv3x3_rw.hip, conv3x3_ps4.hip, conv3x3_ps9.hip, arsb32c.hip, conv64_q8.hip,
// conv64_sq.hip, arsb_sq.hip, conv64_s.hip; DESIGN.md section 4, "how a register-weight kernel is written").
//
// Such a kernel runs one wave per SIMD with the weights in registers and an unbroken stream of MFMAs; everything else a row step needs -- the epilogue of a
// finished row, the LDS-DMA of a later block, finishing work -- is cut into micro-ops, a few instructions each.  A constexpr function of the kernel builds the
// op list (OpList), the kernel deals it proportionally to the slots behind its MFMA groups (static_for over the list, `if constexpr` on the slot's index range),
// and pin_mfmas tells the scheduler to keep what was dealt to a slot there.  Nothing of this exists at run time.
//
// Beside that: the vector / LDS-pointer types, the column-major split of the work into strips, and the few address formulas these kernels have in common.
// Epilogue arithmetic is rowtile.h's.
#pragma once
#include "common.h"
#include <type_traits>
#include <utility>

typedef unsigned u4_t __attribute__((ext_vector_type(4)));
typedef unsigned u2_t __attribute__((ext_vector_type(2)));
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef int i8v_t __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(3))) half8_t* lds_h8_t;
typedef const __attribute__((address_space(3))) u4_t* lds_u4_t;

constexpr unsigned kOOR = 0xFFFF0000u;         // a buffer offset no descriptor here covers: the load returns zeros / fetches nothing, the store is dropped
constexpr float16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

// ---- the micro-op table ---------------------------------------------------------------------------------------------------------------------------------
// kind: the kernel's own OpKind; a, b, c: its compile-time arguments.  A table that outgrows its array does not compile: lists are only ever built in constant
// expressions, and there an index past op[] is an error, not a dropped op.
struct Op { int kind, a, b, c; };
struct OpList {
    int n = 0;
    Op op[64] = {};
    constexpr void push(int kind, int a = 0, int b = 0, int c = 0) { op[n] = Op{kind, a, b, c}; ++n; }
    constexpr void append(const OpList& o) { for (int i = 0; i < o.n; ++i) push(o.op[i].kind, o.op[i].a, o.op[i].b, o.op[i].c); }
};
constexpr int count_kind(const OpList& l, int lo, int hi, int kind) { int n = 0; for (int i = lo; i < hi; ++i) n += l.op[i].kind == kind; return n; }

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order: the loop over a table's ops (N = the table's n) or over a step's chunks
template <int... I, typename F> __device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) { static_for_seq(std::make_integer_sequence<int, N>{}, f); }

// Pins a group of NM MFMAs: each followed by FILL VALU / SALU instructions, NDS DS reads behind the first (a group without MFMAs still places its reads).  What the
// kernel dealt to the group stays between its MFMAs instead of drifting to wherever the scheduler sees a shorter critical path.
template <int NM, int NDS, int FILL>
__device__ __forceinline__ void pin_mfmas()
{
#pragma unroll
    for (int i_ = 0; i_ < (NM > 0 ? NM : 1); ++i_) {
        if (i_ < NM) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (i_ == 0 && NDS > 0) __builtin_amdgcn_sched_group_barrier(0x100, NDS, 0);
        if (i_ < NM) __builtin_amdgcn_sched_group_barrier(0x006, FILL, 0);
    }
}

// ---- the work of a launch: (plane b, tile column pxi, row block s), column-major -- s fastest -- cut into G contiguous ranges; a range is walked strip by
// strip, a strip being its blocks [s0, s1) of one column.  (conv3x3_ps4 / ps9 compile to other code through it and keep their own spelling; conv3x3_rw,
// arsb32c and conv64_q8 walk patches, not strips.)
struct Strip { int b, pxi, s0, s1; };
struct StripRange {
    int item, item_end, px, nyb;
    __device__ __forceinline__ StripRange(int B, int px_, int nyb_, int g, int G) : px(px_), nyb(nyb_)
    {
        const long long nitems = (long long)B * px * nyb;
        item = (int)(nitems * g / G);
        item_end = (int)(nitems * (g + 1) / G);
    }
    __device__ __forceinline__ bool more() const { return item < item_end; }
    __device__ __forceinline__ Strip next()
    {
        const int s0 = item % nyb;
        const int t_ = item / nyb;
        const int pxi = t_ % px, b = t_ / px;
        const int s1 = min(nyb, s0 + (item_end - item));
        item += s1 - s0;
        return Strip{b, pxi, s0, s1};
    }
};

// MFMA row i = 8q + 4h' + e of a 32-row A fragment (register 4q + e of the lanes hh = h') is given channel 16 (q >> 1) + 8 h' + 4 (q & 1) + e: a lane's
// registers 8g .. 8g+7 are then eight consecutive channels, one 16-byte slot.  The weight row (of 64: two k-halves) that lane (wi = lane & 31, hh = lane >> 5)
// loads.  (Through this helper arsb32c, arsb_sq, conv3x3_rw and conv1x1 compile to other instruction orders: they spell it out.)
__device__ __forceinline__ int weight_row(int wi, int hh)
{
    const int wq = wi >> 3;
    return (hh << 5) | (16 * (wq >> 1) + 8 * ((wi >> 2) & 1) + 4 * (wq & 1) + (wi & 3));
}

// fp16 rows in LDS: pixel col at col * 128, 16-byte slot s at s ^ ((col >> 1) & 7).  The B fragment (column cc, k-slice ks) is read by lane half hh at slot
// 2 ks + hh: this address for ks = 0, XOR 32 ks for the others
__device__ __forceinline__ unsigned frag_addr(unsigned lds0, int cc, int hh) { return lds0 + (unsigned)(cc * 128 + ((((cc >> 1) & 7) ^ hh) << 4)); }

// four packed fp16 pairs -> two words of four fp8 (E4M3) each, the values times 1/4 (the source is DIVIDED by the scale operand; with MODE.FP16_OVFL set the
// conversions saturate).  One block, the two words' conversions alternating, a wait state at its end: a conversion writes HALF a register, and gfx950 wants one
// wait state between such a write and the next VALU use of the register (the half-word is not forwarded).  The compiler's hazard recognizer places that state
// for its own instructions and cannot see into inline asm: issued back to back, the second conversion of a word at times kept a stale first half -- results
// that changed from run to run (tools/diag_q8_batch.py).
// (inline asm: through __builtin_amdgcn_cvt_scalef32_pk_fp8_f16 this compiler converted the first word of a slot four times and read nothing else of it --
// found with the constant-image experiment of tools/diag_q8.py)
__device__ __forceinline__ void cvt4(unsigned a0, unsigned a1, unsigned b0, unsigned b1, unsigned& p0, unsigned& p1)
{
    const float quarter = 4.0f;
    asm volatile("v_cvt_scalef32_pk_fp8_f16 %0, %2, %6\n\t"
                 "v_cvt_scalef32_pk_fp8_f16 %1, %4, %6\n\t"
                 "v_cvt_scalef32_pk_fp8_f16 %0, %3, %6 op_sel:[0,0,1]\n\t"
                 "v_cvt_scalef32_pk_fp8_f16 %1, %5, %6 op_sel:[0,0,1]\n\t"
                 "s_nop 0"
                 : "=&v"(p0), "=&v"(p1) : "v"(a0), "v"(a1), "v"(b0), "v"(b1), "v"(quarter));
}
// the two 16-byte slots of 16 channels -> their 16 fp8 bytes
__device__ __forceinline__ u4_t cvt16(const u4_t& w0, const u4_t& w1)
{
    u4_t d = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        unsigned p0, p1;
        cvt4(w0[2 * k], w0[2 * k + 1], w1[2 * k], w1[2 * k + 1], p0, p1);
        d[k] = p0; d[2 + k] = p1;
    }
    return d;
}
