// lut3d_api.cpp -- the entry points of the 3D LUT colour step: moe_lut3d_create / _run / _info / _destroy (lut3d.hip; the definition: moephoto_amd/lut3d.py).  What they
// check of the caller's table, vertices and arguments is the contract the kernel relies on: the kernel checks nothing.
#include <cmath>
#include <vector>
#include "net.h"

using namespace moe;

extern "C" {

int moe_lut3d_create(int d, const float* table_host, const float* vertices_host, int device, moe_lut3d** out)
{
    if (!table_host || !vertices_host || !out) return fail(MOE_EINVAL, "moe_lut3d_create: NULL argument");
    *out = nullptr;
    if (d < LUT3D_MIN || d > LUT3D_MAX) return fail(MOE_EINVAL, "moe_lut3d_create: d = %d (%d to %d)", d, LUT3D_MIN, LUT3D_MAX);
    const size_t n = (size_t)d * d * d;
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < d; ++i) {
            const float v = vertices_host[c * d + i];
            if (!std::isfinite(v)) return fail(MOE_EINVAL, "moe_lut3d_create: vertex %d of channel %d is not finite", i, c);
            if (i && v < vertices_host[c * d + i - 1]) return fail(MOE_EINVAL, "moe_lut3d_create: vertex %d of channel %d decreases (%g after %g)", i, c, (double)v, (double)vertices_host[c * d + i - 1]);
        }
    for (size_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(table_host[i])) return fail(MOE_EINVAL, "moe_lut3d_create: table value %lld of channel %d is not finite", (long long)(i % n), (int)(i / n));
    // one 16-byte entry per lattice point, red fastest -- the table's own order: a corner is one load
    std::vector<float> host(4 * n + 3 * (size_t)d);
    for (size_t i = 0; i < n; ++i) {
        host[4 * i] = table_host[i]; host[4 * i + 1] = table_host[n + i]; host[4 * i + 2] = table_host[2 * n + i]; host[4 * i + 3] = 0.f;
    }
    for (int i = 0; i < 3 * d; ++i) host[4 * n + i] = vertices_host[i];
    HIP_TRY(hipSetDevice(device));
    moe_lut3d* h = new moe_lut3d{d, device, nullptr, 16 * n};
    if (hipMalloc(&h->dev, host.size() * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return fail(MOE_ENOMEM, "moe_lut3d_create: the table of %zu bytes does not fit the device", host.size() * sizeof(float));
    }
    const hipError_t e = hipMemcpy(h->dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(h->dev);
        delete h;
        return fail(MOE_EHIP, "moe_lut3d_create: upload: %s", hipGetErrorString(e));
    }
    *out = h;
    return MOE_OK;
}

int moe_lut3d_run(const moe_lut3d* h, const void* src, int src_bits, int H, int W, void* dst, int bits, int order, float strength, void* stream)
{
    if (!h || !src || !dst) return fail(MOE_EINVAL, "moe_lut3d_run: NULL argument");
    if (src_bits != 8 && src_bits != 16) return fail(MOE_EINVAL, "moe_lut3d_run: src_bits %d (8 or 16)", src_bits);
    const int flags = bits & ~0xff, low = bits & 0xff;
    if (bits < 0 || (flags & ~(MOE_Q_ROUND | MOE_Q_ORDERED | MOE_Q_UNIT))) return fail(MOE_EINVAL, "moe_lut3d_run: bits 0x%x carries unknown flags (MOE_Q_ROUND, MOE_Q_ORDERED, MOE_Q_UNIT)", bits);
    if ((flags & MOE_Q_ROUND) && (flags & MOE_Q_ORDERED)) return fail(MOE_EINVAL, "moe_lut3d_run: MOE_Q_ROUND and MOE_Q_ORDERED are both set (one mode at most)");
    if ((flags & MOE_Q_UNIT) && !(flags & (MOE_Q_ROUND | MOE_Q_ORDERED))) return fail(MOE_EINVAL, "moe_lut3d_run: MOE_Q_UNIT without MOE_Q_ROUND or MOE_Q_ORDERED (the truncating quantiser has no unit scale)");
    if (low != 8 && low != 16) return fail(MOE_EINVAL, "moe_lut3d_run: bits %d (8 or 16)", low);
    if (H < 1 || W < 1) return fail(MOE_EINVAL, "moe_lut3d_run: size %d x %d must be positive", W, H);
    if (3ll * H * W > 0x7fffffffll) return fail(MOE_EINVAL, "moe_lut3d_run: the %d x %d x 3 samples do not fit an int", W, H);
    if (order != MOE_ORDER_BGR && order != MOE_ORDER_RGB) return fail(MOE_EINVAL, "moe_lut3d_run: order %d (MOE_ORDER_BGR or MOE_ORDER_RGB)", order);
    if (!std::isfinite(strength)) return fail(MOE_EINVAL, "moe_lut3d_run: strength is not finite");
    if (src_bits == 16 && ((uintptr_t)src & 1)) return fail(MOE_EINVAL, "moe_lut3d_run: src is not 2-byte aligned (uint16 samples)");
    if (low == 16 && ((uintptr_t)dst & 1)) return fail(MOE_EINVAL, "moe_lut3d_run: dst is not 2-byte aligned (uint16 samples)");
    const long long samples = 3ll * H * W;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)samples * (src_bits / 8), d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)samples * (low / 8);
    if (d0 < s1 && s0 < d1) return fail(MOE_EINVAL, "moe_lut3d_run: dst overlaps src");
    Lut3dArgs k = {};
    k.table = (const float4*)h->dev;
    k.vert = (const float*)((const char*)h->dev + h->table_bytes);
    k.d = h->d;
    k.strength = strength; k.rest = 1.f - strength; k.blend = strength != 1.f;
    k.rgb = order == MOE_ORDER_RGB;
    const float top = (float)((1 << low) - 1);
    const QuantDither dq = {(flags & MOE_Q_UNIT) ? top : top + 1.f, top, (flags & MOE_Q_ORDERED) != 0};
    HIP_TRY(hipSetDevice(h->device));
    launch_lut3d(src, src_bits, H, W, dst, low, k, top + 1.f, (flags & (MOE_Q_ROUND | MOE_Q_ORDERED)) ? &dq : nullptr, (hipStream_t)stream);
    return launched("to_output_lut3d_kernel");
}

int moe_lut3d_info(const moe_lut3d* h, int64_t info[4])
{
    if (!h || !info) return fail(MOE_EINVAL, "moe_lut3d_info: NULL argument");
    info[0] = h->d; info[1] = (int64_t)h->table_bytes; info[2] = 3 * LUT3D_MAX * (int64_t)sizeof(float); info[3] = 8;
    return MOE_OK;
}

void moe_lut3d_destroy(moe_lut3d* h)
{
    if (!h) return;
    if (h->dev) {
        (void)hipSetDevice(h->device);
        (void)hipFree(h->dev);
    }
    delete h;
}

}  // extern "C"
