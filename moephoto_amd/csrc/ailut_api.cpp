// ailut_api.cpp -- the entry points of the AiLUT generator net: moe_ailut_create / _num_params / _param_info / _set_param / _finalize / _run / _stage / _guards /
// _destroy, moe_ailut_thumbnail and moe_lut3d_read (ailut.hip; the definition: moephoto_amd/ailut.py).  What they check of the caller's arguments is the contract the
// kernels rely on: the kernels check nothing.
#include <cmath>
#include <string>
#include <vector>
#include "net.h"

using namespace moe;

namespace {
constexpr size_t GUARD = 64;                 // floats between any two of the handle's device buffers, before the first and behind the last
constexpr unsigned char GUARD_BYTE = 0xA5;
constexpr const char* KEY_H0 = "lut_generator.weights_generator", * KEY_BANK = "lut_generator.basis_luts_bank", * KEY_G = "adaint.intervals_generator";
}  // namespace

struct moe_ailut {
    int d = 0, ranks = 0, device = -1;
    bool finalized = false;
    std::vector<Param> params;               // the reference's state-dict entries, in its order
    std::vector<size_t> at;                  // params[i]'s offset in dev, in floats
    std::vector<std::pair<size_t, size_t>> guards;      // (offset, floats) of every guard band
    void* dev = nullptr;                     // one allocation: guard, parameter, guard, .., the workspace's buffers likewise
    size_t floats = 0;
    AilutNet net = {};
};

static Param make_param(const std::string& name, std::vector<int64_t> shape)
{
    Param p;
    p.name = name;
    p.shape = std::move(shape);
    return p;
}

static int find_param(const moe_ailut* g, const char* name)
{
    for (size_t i = 0; i < g->params.size(); ++i)
        if (g->params[i].name == name) return (int)i;
    return -1;
}

static void release(moe_ailut* g)          // runs queued earlier on any stream may still read the block: the device is synchronised before it is freed
{
    if (g->dev) {
        (void)hipSetDevice(g->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(g->dev);
        g->dev = nullptr;
    }
    g->finalized = false;
}

extern "C" {

int moe_ailut_create(int d, int ranks, moe_ailut** out)
{
    if (!out) return fail(MOE_EINVAL, "moe_ailut_create: NULL argument");
    *out = nullptr;
    if (d < LUT3D_MIN || d > LUT3D_MAX) return fail(MOE_EINVAL, "moe_ailut_create: d = %d (%d to %d)", d, LUT3D_MIN, LUT3D_MAX);
    if (ranks < AILUT_MIN_RANKS || ranks > AILUT_MAX_RANKS) return fail(MOE_EINVAL, "moe_ailut_create: ranks = %d (%d to %d)", ranks, AILUT_MIN_RANKS, AILUT_MAX_RANKS);
    moe_ailut* g = new moe_ailut;
    g->d = d;
    g->ranks = ranks;
    for (int i = 0; i < 5; ++i) {
        const std::string b = "backbone." + std::to_string(i);
        g->params.push_back(make_param(b + ".0.weight", {AILUT_CH[i + 1], AILUT_CH[i], 3, 3}));
        g->params.push_back(make_param(b + ".0.bias", {AILUT_CH[i + 1]}));
        if (i < 4) {
            g->params.push_back(make_param(b + ".2.weight", {AILUT_CH[i + 1]}));
            g->params.push_back(make_param(b + ".2.bias", {AILUT_CH[i + 1]}));
        }
    }
    g->params.push_back(make_param(std::string(KEY_H0) + ".weight", {ranks, AILUT_FEATS}));
    g->params.push_back(make_param(std::string(KEY_H0) + ".bias", {ranks}));
    g->params.push_back(make_param(std::string(KEY_BANK) + ".weight", {3ll * d * d * d, ranks}));
    g->params.push_back(make_param(std::string(KEY_G) + ".weight", {3ll * (d - 1), AILUT_FEATS}));
    g->params.push_back(make_param(std::string(KEY_G) + ".bias", {3ll * (d - 1)}));
    *out = g;
    return MOE_OK;
}

int moe_ailut_num_params(const moe_ailut* g)
{
    if (!g) return fail(MOE_EINVAL, "moe_ailut_num_params: NULL argument");
    return (int)g->params.size();
}

int moe_ailut_param_info(const moe_ailut* g, int index, const char** name, int64_t shape[4], int* ndim)
{
    if (!g || !name || !shape || !ndim) return fail(MOE_EINVAL, "moe_ailut_param_info: NULL argument");
    if (index < 0 || index >= (int)g->params.size()) return fail(MOE_EINVAL, "moe_ailut_param_info: index %d (0 to %d)", index, (int)g->params.size() - 1);
    const Param& p = g->params[index];
    *name = p.name.c_str();
    *ndim = (int)p.shape.size();
    for (size_t i = 0; i < p.shape.size(); ++i) shape[i] = p.shape[i];
    return MOE_OK;
}

int moe_ailut_set_param(moe_ailut* g, const char* name, const float* data, const int64_t* shape, int ndim)
{
    if (!g || !name || !data || !shape) return fail(MOE_EINVAL, "moe_ailut_set_param: NULL argument");
    const int i = find_param(g, name);
    if (i < 0) return fail(MOE_EINVAL, "moe_ailut_set_param: unknown parameter '%s'", name);
    Param& p = g->params[i];
    bool same = ndim == (int)p.shape.size();
    for (int k = 0; same && k < ndim; ++k) same = shape[k] == p.shape[k];
    if (!same) return fail(MOE_EINVAL, "moe_ailut_set_param: '%s' has another shape (%d dims) than this generator's (d = %d, ranks = %d)", name, ndim, g->d, g->ranks);
    const int64_t n = p.numel();
    for (int64_t k = 0; k < n; ++k)
        if (!std::isfinite(data[k])) return fail(MOE_EINVAL, "moe_ailut_set_param: value %lld of '%s' is not finite", (long long)k, name);
    p.data.assign(data, data + n);
    p.set = true;
    g->finalized = false;          // (the device copy is stale: finalize again)
    return MOE_OK;
}

int moe_ailut_finalize(moe_ailut* g, int device)
{
    if (!g) return fail(MOE_EINVAL, "moe_ailut_finalize: NULL argument");
    if (device < 0) return fail(MOE_EINVAL, "moe_ailut_finalize: device %d", device);
    for (const Param& p : g->params)
        if (!p.set) return fail(MOE_ESTATE, "moe_ailut_finalize: parameter '%s' is not set", p.name.c_str());
    release(g);
    // the layout: guard, buffer, guard, buffer, .., guard; every buffer a multiple of 4 floats, so 16-byte aligned (doubles included)
    size_t at = 0;
    g->at.clear();
    g->guards.clear();
    auto guard = [&]() { g->guards.push_back({at, GUARD}); at += GUARD; };
    auto take = [&](size_t n) { const size_t o = at; at += (n + 3) / 4 * 4; guard(); return o; };
    guard();
    for (const Param& p : g->params) g->at.push_back(take((size_t)p.numel()));
    const size_t thumb = take(3 * (size_t)AILUT_SIZE * AILUT_SIZE);
    size_t act[5], stat[4];
    for (int i = 0; i < 5; ++i) {
        const int side = AILUT_SIZE >> (i + 1);
        act[i] = take((size_t)AILUT_CH[i + 1] * side * side);
    }
    for (int i = 0; i < 4; ++i) stat[i] = take((size_t)AILUT_CH[i + 1] * AILUT_STAT_GROUPS[i] * 2 * 2);          // doubles: two floats each
    const size_t lin = take((size_t)AILUT_MAX_RANKS + 3 * (LUT3D_MAX - 1));
    std::vector<float> host(at, 0.f);
    for (size_t i = 0; i < g->params.size(); ++i) std::copy(g->params[i].data.begin(), g->params[i].data.end(), host.begin() + g->at[i]);
    for (const auto& b : g->guards) memset(host.data() + b.first, GUARD_BYTE, b.second * sizeof(float));
    HIP_TRY(hipSetDevice(device));
    if (hipMalloc(&g->dev, at * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        g->dev = nullptr;
        return fail(MOE_ENOMEM, "moe_ailut_finalize: the generator's %zu bytes do not fit the device", at * sizeof(float));
    }
    g->device = device;
    g->floats = at;
    const hipError_t e = hipMemcpy(g->dev, host.data(), at * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        release(g);
        return fail(MOE_EHIP, "moe_ailut_finalize: upload: %s", hipGetErrorString(e));
    }
    float* const base = (float*)g->dev;
    AilutNet& n = g->net;
    size_t k = 0;
    for (int i = 0; i < 5; ++i) {
        n.w[i] = base + g->at[k++];
        n.b[i] = base + g->at[k++];
        if (i < 4) {
            n.gamma[i] = base + g->at[k++];
            n.beta[i] = base + g->at[k++];
        }
    }
    n.h0_w = base + g->at[k++]; n.h0_b = base + g->at[k++]; n.bank = base + g->at[k++]; n.g_w = base + g->at[k++]; n.g_b = base + g->at[k++];
    n.thumb = base + thumb;
    for (int i = 0; i < 5; ++i) n.act[i] = base + act[i];
    for (int i = 0; i < 4; ++i) n.stat[i] = (double*)(base + stat[i]);
    n.lin = base + lin;
    n.d = g->d;
    n.ranks = g->ranks;
    g->finalized = true;
    return MOE_OK;
}

// what moe_ailut_run and moe_ailut_stage refuse alike, before any device call
static int check_run(const char* who, const moe_ailut* g, const void* src, int src_bits, int H, int W, int order, const moe_lut3d* lut)
{
    if (!g || !src || !lut) return fail(MOE_EINVAL, "%s: NULL argument", who);
    if (src_bits != 8 && src_bits != 16) return fail(MOE_EINVAL, "%s: src_bits %d (8 or 16)", who, src_bits);
    if (H < 1 || W < 1) return fail(MOE_EINVAL, "%s: size %d x %d must be positive", who, W, H);
    if (3ll * H * W > 0x7fffffffll) return fail(MOE_EINVAL, "%s: the %d x %d x 3 samples do not fit an int", who, W, H);
    if (order != MOE_ORDER_BGR && order != MOE_ORDER_RGB) return fail(MOE_EINVAL, "%s: order %d (MOE_ORDER_BGR or MOE_ORDER_RGB)", who, order);
    if (src_bits == 16 && ((uintptr_t)src & 1)) return fail(MOE_EINVAL, "%s: src is not 2-byte aligned (uint16 samples)", who);
    if (lut->d != g->d) return fail(MOE_EINVAL, "%s: the table handle has d = %d, the generator writes d = %d", who, lut->d, g->d);
    if (!g->finalized) return fail(MOE_ESTATE, "%s: the generator is not finalized (moe_ailut_finalize)", who);
    if (lut->device != g->device) return fail(MOE_EINVAL, "%s: the table handle lives on device %d, the generator on device %d", who, lut->device, g->device);
    return MOE_OK;
}

static int run_stage(const moe_ailut* g, int stage, const void* src, int src_bits, int H, int W, int order, const moe_lut3d* lut, hipStream_t s)
{
    if (stage == 0) {
        launch_ailut_thumb(src, src_bits, H, W, order == MOE_ORDER_RGB, g->net.thumb, s);
        return launched("to_float_thumb_kernel");
    }
    return launched(launch_ailut_stage(g->net, stage, (float4*)lut->dev, (float*)((char*)lut->dev + lut->table_bytes), s));
}

int moe_ailut_run(const moe_ailut* g, const void* src, int src_bits, int H, int W, int order, const moe_lut3d* lut, void* stream)
{
    if (const int rc = check_run("moe_ailut_run", g, src, src_bits, H, W, order, lut)) return rc;
    HIP_TRY(hipSetDevice(g->device));
    for (int stage = 0; stage < AILUT_STAGES; ++stage)
        if (const int rc = run_stage(g, stage, src, src_bits, H, W, order, lut, (hipStream_t)stream)) return rc;
    return MOE_OK;
}

int moe_ailut_stage(const moe_ailut* g, int stage, const void* src, int src_bits, int H, int W, int order, const moe_lut3d* lut, void* stream)
{
    if (const int rc = check_run("moe_ailut_stage", g, src, src_bits, H, W, order, lut)) return rc;
    if (stage < 0 || stage >= AILUT_STAGES) return fail(MOE_EINVAL, "moe_ailut_stage: stage %d (0 to %d)", stage, AILUT_STAGES - 1);
    HIP_TRY(hipSetDevice(g->device));
    return run_stage(g, stage, src, src_bits, H, W, order, lut, (hipStream_t)stream);
}

int moe_ailut_thumbnail(const void* src, int src_bits, int H, int W, int order, float* dst, int device, void* stream)
{
    if (!src || !dst) return fail(MOE_EINVAL, "moe_ailut_thumbnail: NULL argument");
    if (src_bits != 8 && src_bits != 16) return fail(MOE_EINVAL, "moe_ailut_thumbnail: src_bits %d (8 or 16)", src_bits);
    if (H < 1 || W < 1) return fail(MOE_EINVAL, "moe_ailut_thumbnail: size %d x %d must be positive", W, H);
    if (3ll * H * W > 0x7fffffffll) return fail(MOE_EINVAL, "moe_ailut_thumbnail: the %d x %d x 3 samples do not fit an int", W, H);
    if (order != MOE_ORDER_BGR && order != MOE_ORDER_RGB) return fail(MOE_EINVAL, "moe_ailut_thumbnail: order %d (MOE_ORDER_BGR or MOE_ORDER_RGB)", order);
    if (src_bits == 16 && ((uintptr_t)src & 1)) return fail(MOE_EINVAL, "moe_ailut_thumbnail: src is not 2-byte aligned (uint16 samples)");
    if ((uintptr_t)dst & 3) return fail(MOE_EINVAL, "moe_ailut_thumbnail: dst is not 4-byte aligned (float planes)");
    if (device < 0) return fail(MOE_EINVAL, "moe_ailut_thumbnail: device %d", device);
    HIP_TRY(hipSetDevice(device));
    launch_ailut_thumb(src, src_bits, H, W, order == MOE_ORDER_RGB, dst, (hipStream_t)stream);
    return launched("to_float_thumb_kernel");
}

int moe_ailut_guards(const moe_ailut* g, int64_t* bad, void* stream)
{
    if (!g || !bad) return fail(MOE_EINVAL, "moe_ailut_guards: NULL argument");
    if (!g->finalized) return fail(MOE_ESTATE, "moe_ailut_guards: the generator is not finalized (moe_ailut_finalize)");
    HIP_TRY(hipSetDevice(g->device));
    std::vector<float> host(g->floats);
    HIP_TRY(hipMemcpyAsync(host.data(), g->dev, g->floats * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    int64_t n = 0;
    for (const auto& b : g->guards) {
        const unsigned char* const p = (const unsigned char*)(host.data() + b.first);
        for (size_t i = 0; i < b.second * sizeof(float); ++i) n += p[i] != GUARD_BYTE;
    }
    for (size_t i = 0; i < g->params.size(); ++i)          // the parameters themselves: nothing on the device writes them
        n += memcmp(host.data() + g->at[i], g->params[i].data.data(), g->params[i].data.size() * sizeof(float)) != 0;
    *bad = n;
    return MOE_OK;
}

void moe_ailut_destroy(moe_ailut* g)
{
    if (!g) return;
    release(g);
    delete g;
}

int moe_lut3d_read(const moe_lut3d* h, float* table_host, float* vertices_host, void* stream)
{
    if (!h || !table_host || !vertices_host) return fail(MOE_EINVAL, "moe_lut3d_read: NULL argument");
    const size_t n = (size_t)h->d * h->d * h->d;
    std::vector<float> host(4 * n + 3 * (size_t)h->d);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(host.data(), h->dev, host.size() * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (size_t i = 0; i < n; ++i) {
        table_host[i] = host[4 * i]; table_host[n + i] = host[4 * i + 1]; table_host[2 * n + i] = host[4 * i + 2];
    }
    for (int i = 0; i < 3 * h->d; ++i) vertices_host[i] = host[4 * n + i];
    return MOE_OK;
}

}  // extern "C"
