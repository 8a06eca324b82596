// polyphase.cpp -- the entry points of the two integer polyphase resamplers of planar codes: moe_chroma_resample (chroma.hip: the chroma planes of a luma-only
// chain, integer scales; moe_chroma_guided, chroma_guided.hip: the same planes steered by the finished luma; moe_planes_to_rgb, planes_rgb.hip: a planar frame's RGB form) and moe_fit_create / moe_fit_create_px / _run / _info / _destroy (fit.hip, fit_px.hip: planes / an interleaved image brought to a fitted size).  What they check of the caller's tables is the
// contract the kernels rely on (polyphase.h): the kernels check nothing.
#include "net.h"

using namespace moe;

// One row of an axis' coefficient table (`word`: what the entry point calls a row, "phase" or "output").  sum |c| <= 32767: the row pass's int32 sum holds for any
// uint16 code (32767 * 65535 < 2^31), and the column pass's result fits an int behind its shift.
static int poly_row_check(const char* who, const char* axis, const char* word, long long row, const int16_t* c, int taps)
{
    int sum = 0, mag = 0;
    for (int j = 0; j < taps; ++j) { sum += c[j]; mag += c[j] < 0 ? -c[j] : c[j]; }
    if (sum != 16384 || mag > 32767)
        return fail(MOE_EINVAL, "%s: %s coefficients of %s %lld sum to %d (must be 16384) with magnitudes %d (32767 at most)", who, axis, word, row, sum, mag);
    return MOE_OK;
}

static int poly_depths_check(const char* who, int ds, int dd) { return plane_depth(ds) && plane_depth(dd) ? MOE_OK : fail(MOE_EINVAL, "%s: depth %d -> %d (8, 10, 12 or 16)", who, ds, dd); }
static int poly_aligned_check(const char* who, const void* src, int ds, const void* dst, int dd)
{
    if (ds > 8 && ((uintptr_t)src & 1)) return fail(MOE_EINVAL, "%s: src is not 2-byte aligned (depth %d: uint16 samples)", who, ds);
    if (dd > 8 && ((uintptr_t)dst & 1)) return fail(MOE_EINVAL, "%s: dst is not 2-byte aligned (depth %d: uint16 samples)", who, dd);
    return MOE_OK;
}
static const char* axis_name(int a) { return a ? "vertical" : "horizontal"; }

extern "C" {

int moe_chroma_resample(const void* src, int src_depth, int h, int w, void* dst, int dst_depth, int scale, int taps,
                        const int16_t* cx, const int8_t* ox, const int16_t* cy, const int8_t* oy, int device, void* stream)
{
    if (!src || !dst || !cx || !ox || !cy || !oy) return fail(MOE_EINVAL, "moe_chroma_resample: NULL argument");
    if (int rc = poly_depths_check("moe_chroma_resample", src_depth, dst_depth)) return rc;
    if (h < 1 || w < 1) return fail(MOE_EINVAL, "moe_chroma_resample: size %d x %d must be positive", w, h);
    if (scale < 1 || scale > 16) return fail(MOE_EINVAL, "moe_chroma_resample: scale %d (1 to 16)", scale);
    if ((long long)h * scale > 0x7fffffffll || (long long)w * scale > 0x7fffffffll) return fail(MOE_EINVAL, "moe_chroma_resample: size %d x %d times %d does not fit an int", w, h, scale);
    if (taps != 1 && taps != 2 && taps != 4) return fail(MOE_EINVAL, "moe_chroma_resample: %d taps (1, 2 or 4)", taps);
    if (int rc = poly_aligned_check("moe_chroma_resample", src, src_depth, dst, dst_depth)) return rc;
    ChromaTab t[2] = {};
    const int16_t* const coef[2] = {cx, cy};
    const int8_t* const off[2] = {ox, oy};
    for (int a = 0; a < 2; ++a)
        for (int p = 0; p < scale; ++p) {
            if (int rc = poly_row_check("moe_chroma_resample", axis_name(a), "phase", p, coef[a] + p * taps, taps)) return rc;
            if (off[a][p] < -2 || off[a][p] > 1) return fail(MOE_EINVAL, "moe_chroma_resample: %s offset %d of phase %d (-2 to 1)", axis_name(a), (int)off[a][p], p);
            std::copy(coef[a] + p * taps, coef[a] + (p + 1) * taps, t[a].coef[p]);
            t[a].off[p] = off[a][p];
        }
    HIP_TRY(hipSetDevice(device));
    launch_chroma_resample(src, src_depth, h, w, dst, dst_depth, scale, taps, t[0], t[1], (hipStream_t)stream);
    return launched("resize_kernel_codes");
}

// The guided form of the same planes (chroma_guided.hip): what the kernel's 32-bit row sums and its exact division rest on is checked here.
int moe_chroma_guided(const void* src_c, const void* src_y, int src_depth, int h, int w, void* dst_c, const void* dst_y, int dst_depth, int scale, int loc,
                      const uint8_t* cx, const int8_t* ox, const uint8_t* cy, const int8_t* oy, const uint8_t* range64, int device, void* stream)
{
    if (!src_c || !src_y || !dst_c || !dst_y || !cx || !ox || !cy || !oy || !range64) return fail(MOE_EINVAL, "moe_chroma_guided: NULL argument");
    if (int rc = poly_depths_check("moe_chroma_guided", src_depth, dst_depth)) return rc;
    if (h < 1 || w < 1) return fail(MOE_EINVAL, "moe_chroma_guided: size %d x %d must be positive", w, h);
    if (scale < 2 || scale > 16) return fail(MOE_EINVAL, "moe_chroma_guided: scale %d (2 to 16)", scale);
    if (2ll * h * scale > 0x7fffffffll || 2ll * w * scale > 0x7fffffffll)
        return fail(MOE_EINVAL, "moe_chroma_guided: the luma plane of %d x %d chroma samples times %d does not fit an int", w, h, scale);
    if (loc != MOE_CHROMA_CENTER && loc != MOE_CHROMA_LEFT) return fail(MOE_EINVAL, "moe_chroma_guided: loc %d (MOE_CHROMA_CENTER or MOE_CHROMA_LEFT)", loc);
    if (int rc = poly_aligned_check("moe_chroma_guided", src_c, src_depth, dst_c, dst_depth)) return rc;
    if (src_depth > 8 && ((uintptr_t)src_y & 1)) return fail(MOE_EINVAL, "moe_chroma_guided: src_y is not 2-byte aligned (depth %d: uint16 samples)", src_depth);
    if (dst_depth > 8 && ((uintptr_t)dst_y & 1)) return fail(MOE_EINVAL, "moe_chroma_guided: dst_y is not 2-byte aligned (depth %d: uint16 samples)", dst_depth);
    const uint8_t* const coef[2] = {cx, cy};
    const int8_t* const off[2] = {ox, oy};
    for (int a = 0; a < 2; ++a)
        for (int p = 0; p < scale; ++p) {
            const uint8_t* c = coef[a] + p * 4;
            if (c[0] + c[1] + c[2] + c[3] != 256)
                return fail(MOE_EINVAL, "moe_chroma_guided: %s coefficients of phase %d sum to %d (must be 256)", axis_name(a), p, c[0] + c[1] + c[2] + c[3]);
            if (off[a][p] < -2 || off[a][p] > 1) return fail(MOE_EINVAL, "moe_chroma_guided: %s offset %d of phase %d (-2 to 1)", axis_name(a), (int)off[a][p], p);
        }
    for (int d = 0; d < 64; ++d)
        if (!range64[d]) return fail(MOE_EINVAL, "moe_chroma_guided: range weight %d is zero (the denominator must not vanish)", d);
    const long long es = dst_depth == 8 ? 1 : 2, samples = (long long)h * scale * w * scale;
    const uintptr_t y0 = (uintptr_t)dst_y, y1 = y0 + (uintptr_t)(4 * samples * es), c0 = (uintptr_t)dst_c, c1 = c0 + (uintptr_t)(2 * samples * es);
    if (c0 < y1 && y0 < c1) return fail(MOE_EINVAL, "moe_chroma_guided: dst_c overlaps dst_y (the kernel reads the luma plane while it writes the chroma planes)");
    HIP_TRY(hipSetDevice(device));
    launch_chroma_guided(src_c, src_y, src_depth, h, w, dst_c, dst_y, dst_depth, scale, loc == MOE_CHROMA_LEFT, cx, ox, cy, oy, range64, (hipStream_t)stream);
    return launched("resize_kernel_guided");
}

// RGB frames from a planar 4:2:0 frame (planes_rgb.hip): the x2 chroma tables as moe_chroma_resample takes them, and the matrix constants whose magnitudes the
// kernel's int64 sums and its 32-bit clamp rest on.
int moe_planes_to_rgb(const void* src, int depth, int H, int W, void* dst, int bits, int matrix, int order, int taps,
                      const int16_t* cx, const int8_t* ox, const int16_t* cy, const int8_t* oy, const int32_t* coef, int device, void* stream)
{
    if (!src || !dst || !cx || !ox || !cy || !oy || !coef) return fail(MOE_EINVAL, "moe_planes_to_rgb: NULL argument");
    if (!plane_depth(depth)) return fail(MOE_EINVAL, "moe_planes_to_rgb: depth %d (8, 10, 12 or 16)", depth);
    const int flags = bits & ~0xff, low = bits & 0xff;
    if (flags & ~(MOE_Q_ROUND | MOE_Q_ORDERED | MOE_Q_UNIT)) return fail(MOE_EINVAL, "moe_planes_to_rgb: bits 0x%x carries unknown flags (MOE_Q_ROUND, MOE_Q_ORDERED)", bits);
    if (flags & MOE_Q_UNIT) return fail(MOE_EINVAL, "moe_planes_to_rgb: MOE_Q_UNIT does not apply (the samples are quantised in integers; 8 bits always take the unit scale)");
    if ((flags & MOE_Q_ROUND) && (flags & MOE_Q_ORDERED)) return fail(MOE_EINVAL, "moe_planes_to_rgb: MOE_Q_ROUND and MOE_Q_ORDERED are both set (one mode at most)");
    if (low != 8 && low != 16) return fail(MOE_EINVAL, "moe_planes_to_rgb: bits %d (8 or 16)", low);
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(MOE_EINVAL, "moe_planes_to_rgb: size %d x %d (an even width and height of 2 at least)", W, H);
    if (3ll * H * W > 0x7fffffffll) return fail(MOE_EINVAL, "moe_planes_to_rgb: the %d x %d x 3 samples do not fit an int", W, H);
    if (matrix != MOE_YUV_BT709 && matrix != MOE_YUV_BT601 && matrix != MOE_YUV_BT2020NC) return fail(MOE_EINVAL, "moe_planes_to_rgb: matrix %d (MOE_YUV_BT709, _BT601 or _BT2020NC)", matrix);
    if (order != MOE_ORDER_BGR && order != MOE_ORDER_RGB) return fail(MOE_EINVAL, "moe_planes_to_rgb: order %d (MOE_ORDER_BGR or MOE_ORDER_RGB)", order);
    if (taps != 1 && taps != 2 && taps != 4) return fail(MOE_EINVAL, "moe_planes_to_rgb: %d taps (1, 2 or 4)", taps);
    if (int rc = poly_aligned_check("moe_planes_to_rgb", src, depth, dst, low)) return rc;
    ChromaTab t[2] = {};
    const int16_t* const rows[2] = {cx, cy};
    const int8_t* const off[2] = {ox, oy};
    for (int a = 0; a < 2; ++a)
        for (int p = 0; p < 2; ++p) {
            if (int rc = poly_row_check("moe_planes_to_rgb", axis_name(a), "phase", p, rows[a] + p * taps, taps)) return rc;
            if (off[a][p] < -2 || off[a][p] > 1) return fail(MOE_EINVAL, "moe_planes_to_rgb: %s offset %d of phase %d (-2 to 1)", axis_name(a), (int)off[a][p], p);
            std::copy(rows[a] + p * taps, rows[a] + (p + 1) * taps, t[a].coef[p]);
            t[a].off[p] = off[a][p];
        }
    // |y|, |u|, |v| < 2^16 and constants of 2^30 at most: three products and the rounding term stay below 2^49, and the sum shifted by RGB_FRAC fits an int
    static const char* const names[5] = {"cY", "cRV", "cGU", "cGV", "cBU"};
    for (int i = 0; i < 5; ++i)
        if (coef[i] > (1 << 30) || coef[i] < (i ? -(1 << 30) : 1))
            return fail(MOE_EINVAL, "moe_planes_to_rgb: matrix constant %s = %d (%s, with %d fractional bits)", names[i], (int)coef[i], i ? "a magnitude of 2^30 at most" : "1 to 2^30", RGB_FRAC);
    const long long px = (long long)H * W;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(px + px / 2) * (depth == 8 ? 1 : 2), d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(3 * px) * (low == 8 ? 1 : 2);
    if (d0 < s1 && s0 < d1) return fail(MOE_EINVAL, "moe_planes_to_rgb: dst overlaps src (a workgroup reads chroma samples that belong to its neighbours' pixels)");
    PlanesRgb k = {};
    std::copy(coef, coef + 5, k.coef);
    k.yoff = 16 << (depth - 8); k.coff = 128 << (depth - 8); k.cmax = (1 << depth) - 1; k.top = (1 << low) - 1;
    k.rgb = order == MOE_ORDER_RGB; k.ordered = (flags & MOE_Q_ORDERED) != 0;
    HIP_TRY(hipSetDevice(device));
    launch_planes_rgb(src, depth, H, W, dst, low, taps, t[0], t[1], k, (hipStream_t)stream);
    return launched("to_output_rgb420_kernel");
}

// ---- fitted sizes (fit.hip) ------------------------------------------------------------------------------
struct moe_fit {
    int planes, ds, dd, h, w, oh, ow, th, device;
    int channels;       // 0: `planes` planes (moe_fit_create); 1 .. 4: one interleaved image of as many channels (moe_fit_create_px)
    size_t lds;
    void* tab;          // one device block: ox[ow], oy[oh], then the coefficient rows of x and of y
    FitAxis ax, ay;
};

// The largest source window (samples along the axis) of any tile of `tile` output indices: off[last] + taps - off[first]; off is non-decreasing.
// C > 1: the axis holds m pixels of C interleaved elements and a tile is `tile` ELEMENTS; its window is that of the pixels its elements belong to, in elements.
static long long fit_window(const int32_t* off, long long m, int taps, int tile, int C = 1)
{
    long long worst = 0;
    for (long long e0 = 0; e0 < m * C; e0 += tile) {
        const long long e1 = std::min<long long>(e0 + tile, m * C) - 1;
        worst = std::max(worst, ((long long)off[e1 / C] + taps - off[e0 / C]) * C);
    }
    return worst;
}

// Both creators (`who`): channels = 0 -- `planes` planes, a tile FIT_TW samples wide -- or the channels of one interleaved image, whose tile is FIT_TW ELEMENTS wide.
static int fit_create(const char* who, int planes, int channels, int src_depth, int64_t h, int64_t w, int dst_depth, int64_t oh, int64_t ow, int taps_x, const int16_t* cx,
                      const int32_t* ox, int taps_y, const int16_t* cy, const int32_t* oy, int device, moe_fit** out)
{
    if (!cx || !ox || !cy || !oy || !out) return fail(MOE_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    if (int rc = poly_depths_check(who, src_depth, dst_depth)) return rc;
    if (planes < 1 || planes > 4) return fail(MOE_EINVAL, "%s: %d planes (1 to 4)", who, planes);
    if (h < 1 || w < 1 || oh < 1 || ow < 1) return fail(MOE_EINVAL, "%s: size %lld x %lld -> %lld x %lld must be positive", who, (long long)w, (long long)h, (long long)ow, (long long)oh);
    if (h > 0x7fffffffll || w > 0x7fffffffll || oh > 0x7fffffffll || ow > 0x7fffffffll)
        return fail(MOE_EINVAL, "%s: size %lld x %lld -> %lld x %lld does not fit an int", who, (long long)w, (long long)h, (long long)ow, (long long)oh);
    const int C = channels ? channels : 1;
    if (w * C > 0x7fffffffll || ow * C > 0x7fffffffll)
        return fail(MOE_EINVAL, "%s: a row of %lld -> %lld pixels of %d channels does not fit an int", who, (long long)w, (long long)ow, C);
    if (taps_x < 1 || taps_x > FIT_TAPS || taps_y < 1 || taps_y > FIT_TAPS) return fail(MOE_EINVAL, "%s: %d x %d taps (1 to %d)", who, taps_x, taps_y, FIT_TAPS);
    const int16_t* const coef[2] = {cx, cy};
    const int32_t* const off[2] = {ox, oy};
    const long long n[2] = {w, h}, m[2] = {ow, oh};
    const int taps[2] = {taps_x, taps_y};
    for (int a = 0; a < 2; ++a)
        for (long long o = 0; o < m[a]; ++o) {
            if (int rc = poly_row_check(who, axis_name(a), "output", o, coef[a] + o * taps[a], taps[a])) return rc;
            const long long first = off[a][o];
            if (first + taps[a] - 1 < 0 || first > n[a] - 1)
                return fail(MOE_EINVAL, "%s: %s offset %lld of output %lld: its %d taps do not reach the %lld samples", who, axis_name(a), first, o, taps[a], n[a]);
            if (o && first < off[a][o - 1])
                return fail(MOE_EINVAL, "%s: %s offset %lld of output %lld is below its predecessor's %d (offsets must not decrease)", who, axis_name(a), first, o, (int)off[a][o - 1]);
        }
    // the tile: FIT_TW outputs wide and th high, the largest th whose window (the row pass's int32 sums and the source samples) fits the budget
    const long long es = src_depth == 8 ? 1 : 2, sw = fit_window(ox, ow, taps_x, FIT_TW, C);
    int th = 0;
    long long lds = 0;
    for (int t : {32, 16, 8}) {
        const long long sh = fit_window(oy, oh, taps_y, t);
        lds = sh * FIT_TW * 4 + ((sh * sw * es + 15) & ~15ll);
        if (lds <= (long long)FIT_LDS_BUDGET) { th = t; break; }
    }
    if (!th) return fail(MOE_EINVAL, "%s: the source window of a %d x 8 tile takes %lld bytes of LDS (%lld at most): the offsets step too far", who, FIT_TW, lds, (long long)FIT_LDS_BUDGET);
    std::unique_ptr<moe_fit> f(new moe_fit{});
    f->planes = planes; f->channels = channels; f->ds = src_depth; f->dd = dst_depth; f->h = (int)h; f->w = (int)w; f->oh = (int)oh; f->ow = (int)ow; f->th = th; f->device = device;
    f->lds = (size_t)lds;
    // the upload: offsets, then (16-byte aligned) the coefficient rows padded to FIT_TAPS with zeros
    const size_t n_off = (((size_t)(ow + oh) * 4) + 15) & ~(size_t)15, n_cx = (size_t)ow * FIT_TAPS * 2, n_cy = (size_t)oh * FIT_TAPS * 2;
    std::vector<unsigned char> host(n_off + n_cx + n_cy, 0);
    memcpy(host.data(), ox, (size_t)ow * 4);
    memcpy(host.data() + (size_t)ow * 4, oy, (size_t)oh * 4);
    for (int a = 0; a < 2; ++a) {
        int16_t* rows = (int16_t*)(host.data() + n_off + (a ? n_cx : 0));
        for (long long o = 0; o < m[a]; ++o) memcpy(rows + o * FIT_TAPS, coef[a] + o * taps[a], (size_t)taps[a] * 2);
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(&f->tab, host.size()));
    const hipError_t e = hipMemcpy(f->tab, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(f->tab);
        return fail(MOE_EHIP, "%s: the tables' upload failed: %s", who, hipGetErrorString(e));
    }
    const unsigned char* d = (const unsigned char*)f->tab;
    f->ax = FitAxis{(const int*)d, (const short*)(d + n_off), taps_x};
    f->ay = FitAxis{(const int*)(d + (size_t)ow * 4), (const short*)(d + n_off + n_cx), taps_y};
    *out = f.release();
    return MOE_OK;
}

int moe_fit_create(int planes, int src_depth, int64_t h, int64_t w, int dst_depth, int64_t oh, int64_t ow, int taps_x, const int16_t* cx, const int32_t* ox,
                   int taps_y, const int16_t* cy, const int32_t* oy, int device, moe_fit** out)
{
    return fit_create("moe_fit_create", planes, 0, src_depth, h, w, dst_depth, oh, ow, taps_x, cx, ox, taps_y, cy, oy, device, out);
}

int moe_fit_create_px(int channels, int src_depth, int64_t h, int64_t w, int dst_depth, int64_t oh, int64_t ow, int taps_x, const int16_t* cx, const int32_t* ox,
                      int taps_y, const int16_t* cy, const int32_t* oy, int device, moe_fit** out)
{
    if (out) *out = nullptr;
    if (channels < 1 || channels > 4) return fail(MOE_EINVAL, "moe_fit_create_px: %d channels (1 to 4)", channels);
    return fit_create("moe_fit_create_px", 1, channels, src_depth, h, w, dst_depth, oh, ow, taps_x, cx, ox, taps_y, cy, oy, device, out);
}

int moe_fit_run(const moe_fit* f, const void* src, void* dst, void* stream)
{
    if (!f || !src || !dst) return fail(MOE_EINVAL, "moe_fit_run: NULL argument");
    if (int rc = poly_aligned_check("moe_fit_run", src, f->ds, dst, f->dd)) return rc;
    HIP_TRY(hipSetDevice(f->device));
    if (f->channels) {
        launch_fit_px(src, f->ds, f->h, f->w, dst, f->dd, f->oh, f->ow, f->channels, f->th, f->lds, f->ax, f->ay, (hipStream_t)stream);
        return launched("resize_kernel_fit_px");
    }
    launch_fit(src, f->ds, f->h, f->w, dst, f->dd, f->oh, f->ow, f->planes, f->th, f->lds, f->ax, f->ay, (hipStream_t)stream);
    return launched("resize_kernel_fit");
}

int moe_fit_info(const moe_fit* f, int64_t info[4])
{
    if (!f || !info) return fail(MOE_EINVAL, "moe_fit_info: NULL argument");
    info[0] = FIT_TW; info[1] = f->th; info[2] = (int64_t)f->lds; info[3] = f->channels ? f->channels : f->planes;
    return MOE_OK;
}

void moe_fit_destroy(moe_fit* f)
{
    if (!f) return;
    if (f->tab) {
        (void)hipSetDevice(f->device);
        (void)hipFree(f->tab);
    }
    delete f;
}

}  // extern "C"
