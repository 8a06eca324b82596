// plan_run.cpp -- the device-resident doCrop (tile gather -> net -> stitch: python/imageProcess.py:157-172): the plans' device tables, stitch, the
// moe_run_plan* runners, the planner's entry points, the inter-rank wire format and the image edges.
#include "net.h"

using namespace moe;

// =====================================================================================================
// plan device cache + stitch + run
// =====================================================================================================
static int plan_device_tables(const Plan& p, int device, int C, int64_t sC, int64_t sH, int64_t sW, int si, int scnt,
                              PlanDeviceCache** outp)
{
    if (scnt < 1) { scnt = 1; si = 0; }
    for (auto& up : p.dev) {
        PlanDeviceCache& d = *up;
        if (d.blob && d.device == device && d.C == C && d.sC == sC && d.sH == sH && d.sW == sW && d.shard_index == si && d.shard_count == scnt) {
            *outp = &d;
            return MOE_OK;
        }
    }
    if (p.dev.size() >= 16) {   // bounded: drop the oldest layout
        if (p.dev.front()->blob) (void)hipFree(p.dev.front()->blob);
        for (auto& e : p.dev.front()->strip_tabs) (void)hipFree(e.second);
        p.dev.erase(p.dev.begin());
    }
    p.dev.push_back(std::make_unique<PlanDeviceCache>());
    PlanDeviceCache& d = *p.dev.back();
    const size_t nt = p.tiles.size();
    std::vector<long long> xo, yo;
    int slot = 0;
    for (const auto& g : p.groups) {
        d.group_first.push_back(slot);
        int cnt = 0;
        for (int k : g.tiles) {
            if (k % scnt != si) continue;
            const TileRect& t = p.tiles[k];
            const long long plane = (long long)(g.th * p.sc) * (g.tw * p.sc);
            for (int c = 0; c < C; ++c) {
                xo.push_back((long long)c * sC + (long long)t.top * sH + (long long)t.left * sW);
                yo.push_back(p.tile_off[k] / p.C * C + (long long)c * plane);
            }
            ++slot; ++cnt;
        }
        d.group_count.push_back(cnt);
    }
    if (xo.empty()) { xo.push_back(0); yo.push_back(0); }
    d.y_mult8 = true;
    for (long long v : yo) d.y_mult8 = d.y_mult8 && (v % 8 == 0);
    // tile_off scaled to C planes (C may differ from the planning shape's channel count, e.g. alpha stripped)
    std::vector<long long> toff(nt);
    for (size_t k = 0; k < nt; ++k) toff[k] = p.tile_off[k] / p.C * C;
    std::vector<char> host;
    auto put = [&](const void* src, size_t bytes) { const size_t a = (host.size() + 255) & ~(size_t)255; host.resize(a + bytes); memcpy(host.data() + a, src, bytes); return a; };
    const size_t o_x = put(xo.data(), xo.size() * 8), o_y = put(yo.data(), yo.size() * 8), o_t = put(toff.data(), toff.size() * 8);
    const size_t o_rf = put(p.row_first.data(), p.row_first.size() * 4), o_rc = put(p.row_cnt.data(), p.row_cnt.size() * 4);
    const size_t o_cf = put(p.col_first.data(), p.col_first.size() * 4), o_cc = put(p.col_cnt.data(), p.col_cnt.size() * 4);
    const size_t o_rt = put(p.row_tab.data(), p.row_tab.size() * 4), o_ct = put(p.col_tab.data(), p.col_tab.size() * 4);
    const float zero = 0.f;
    const size_t o_rp = put(p.ramp.empty() ? &zero : p.ramp.data(), std::max<size_t>(4, p.ramp.size() * 4));
    HIP_TRY(hipMalloc(&d.blob, host.size()));
    HIP_TRY(hipMemcpy(d.blob, host.data(), host.size(), hipMemcpyHostToDevice));
    char* b = (char*)d.blob;
    d.x_off = (long long*)(b + o_x); d.y_off = (long long*)(b + o_y); d.tile_off = (long long*)(b + o_t);
    d.row_first = (int*)(b + o_rf); d.row_cnt = (int*)(b + o_rc); d.col_first = (int*)(b + o_cf); d.col_cnt = (int*)(b + o_cc);
    d.row_tab = (int*)(b + o_rt); d.col_tab = (int*)(b + o_ct); d.ramp = (float*)(b + o_rp);
    d.device = device; d.C = C; d.sC = sC; d.sH = sH; d.sW = sW; d.shard_index = si; d.shard_count = scnt;
    *outp = &d;
    return MOE_OK;
}

static void fill_stitch(const Plan& p, const PlanDeviceCache& d, StitchArgs& a, const float* tiles, const long long* tile_off, int C, void* out, int out_dtype)
{
    a.tiles = tiles; a.tile_off = tile_off;
    a.row_first = d.row_first; a.row_cnt = d.row_cnt; a.col_first = d.col_first; a.col_cnt = d.col_cnt;
    a.row_tab = d.row_tab; a.col_tab = d.col_tab; a.ramp = d.ramp;
    a.out = out; a.out_dtype = out_dtype; a.C = C; a.out_h = p.out_h; a.out_w = p.out_w; a.step_w = p.aw.step;
    a.y0 = 0; a.rows = p.out_h; a.row_lo = 0;
}

struct moe_plan { Plan p; };

extern "C" {

// ---- planner ------------------------------------------------------------------------------------------
int moe_plan_create(const int64_t shape[3], double ram, double ram_coef, int pad, int scale, int align, int cropsize, moe_plan** out)
{
    if (!shape || !out) return fail(MOE_EINVAL, "moe_plan_create: NULL argument");
    auto p = std::make_unique<moe_plan>();
    std::string err;
    int rc = build_plan(p->p, shape, ram, ram_coef, pad, scale, align, cropsize, err);
    if (rc) return fail(rc, "%s", err.c_str());
    *out = p.release();
    return MOE_OK;
}

void moe_plan_destroy(moe_plan* p)
{
    if (!p) return;
    for (auto& d : p->p.dev) { if (d->blob) (void)hipFree(d->blob); for (auto& e : d->strip_tabs) (void)hipFree(e.second); }
    for (auto& d : p->p.fdev) if (d->blob) (void)hipFree(d->blob);
    for (auto& c : p->p.custom_off) if (c.dev) (void)hipFree(c.dev);
    if (p->p.pool) (void)hipFree(p->p.pool);
    delete p;
}

int moe_plan_info(const moe_plan* p, int64_t info[12])
{
    if (!p || !info) return fail(MOE_EINVAL, "moe_plan_info: NULL argument");
    const Plan& q = p->p;
    const int64_t v[12] = {(int64_t)q.tiles.size(), q.ah.step, q.aw.step, q.out_h, q.out_w, q.pad_h_to, q.pad_w_to, q.pad_sc,
                           q.tile_h, q.tile_w, q.ah.clip, q.aw.clip};
    memcpy(info, v, sizeof v);
    return MOE_OK;
}

int moe_plan_rows(const moe_plan* p, int32_t* rows)
{
    if (!p || !rows) return fail(MOE_EINVAL, "moe_plan_rows: NULL argument");
    memcpy(rows, p->p.row_tab.data(), p->p.row_tab.size() * 4);
    return MOE_OK;
}

// Seam rows / columns of every tile for the wire format (misc_kernels.hip: wire_kernel): per tile 8 ints (ra0, ra1, rb0, rb1, ca0, ca1, cb0, cb1), tile-local.
// A tile's value is read at full precision inside its OWN blend band and wherever a LATER tile along the axis blends over it; the union of those bands,
// clipped to the tile, is covered with at most two ranges per axis (more than two are merged into the hull of the second and the rest: a superset is safe).
static void axis_seams(const std::vector<int>& tab, int i, int out[4])
{
    const int n = (int)tab.size() / 4;
    const int o = tab[i * 4 + 2], ext = tab[i * 4 + 3];
    std::vector<std::pair<int, int>> iv;
    for (int k = 0; k < n; ++k) {                      // (earlier tiles' bands lie before the tile; they are taken along for the clipped last tile: a superset is safe)
        const int a = std::max(tab[k * 4 + 0] - o, 0), b = std::min(tab[k * 4 + 1] - o, ext);
        if (b > a) iv.push_back({a, b});
    }
    std::sort(iv.begin(), iv.end());
    std::vector<std::pair<int, int>> m;
    for (auto& v : iv) {
        if (!m.empty() && v.first <= m.back().second) m.back().second = std::max(m.back().second, v.second);
        else m.push_back(v);
    }
    while (m.size() > 2) { m[1].second = m.back().second; m.pop_back(); }
    out[0] = out[1] = out[2] = out[3] = 0;
    if (m.size() >= 1) { out[0] = m[0].first; out[1] = m[0].second; out[2] = out[3] = m[0].second; }
    if (m.size() == 2) { out[2] = m[1].first; out[3] = m[1].second; }
}

int moe_plan_seams(const moe_plan* p, int32_t* seams)
{
    if (!p || !seams) return fail(MOE_EINVAL, "moe_plan_seams: NULL argument");
    const Plan& q = p->p;
    for (int i = 0; i < q.ah.step; ++i)
        for (int j = 0; j < q.aw.step; ++j) {
            int r[4], c[4];
            axis_seams(q.row_tab, i, r);
            axis_seams(q.col_tab, j, c);
            int32_t* o = seams + ((size_t)i * q.aw.step + j) * 8;
            for (int e = 0; e < 4; ++e) { o[e] = r[e]; o[4 + e] = c[e]; }
        }
    return MOE_OK;
}

static_assert(sizeof(moe_wire_rec) == sizeof(WireRec) && sizeof(WireRec) == 64, "moe_wire_rec layout");

int64_t moe_wire_words(const moe_wire_rec* rec)
{
    if (!rec) return -1;
    WireRec r;
    memcpy(&r, rec, sizeof r);
    return wire_rec_words(r);
}

static int wire_call(bool pack, float* tiles, void* wire, const moe_wire_rec* recs_dev, int n, int64_t max_elems, void* stream)
{
    if (n < 0 || (n > 0 && (!tiles || !wire || !recs_dev))) return fail(MOE_EINVAL, "moe_wire_%s: bad argument", pack ? "pack" : "unpack");
    launch_wire(pack, tiles, (unsigned*)wire, (const WireRec*)recs_dev, n, max_elems, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "wire kernel launch failed: %s", hipGetErrorString(e));
    return MOE_OK;
}

int moe_wire_pack(const float* tiles_dev, void* wire_dev, const moe_wire_rec* recs_dev, int n, int64_t max_elems, void* stream)
{
    return wire_call(true, (float*)tiles_dev, wire_dev, recs_dev, n, max_elems, stream);
}

int moe_wire_unpack(float* tiles_dev, const void* wire_dev, const moe_wire_rec* recs_dev, int n, int64_t max_elems, void* stream)
{
    return wire_call(false, tiles_dev, (void*)wire_dev, recs_dev, n, max_elems, stream);
}

int moe_plan_tiles(const moe_plan* p, int32_t* tiles)
{
    if (!p || !tiles) return fail(MOE_EINVAL, "moe_plan_tiles: NULL argument");
    for (size_t k = 0; k < p->p.tiles.size(); ++k) {
        const TileRect& t = p->p.tiles[k];
        const int32_t v[8] = {t.top, t.bottom, t.left, t.right, t.top_t, t.left_t, t.bsc, t.rsc};
        memcpy(tiles + k * 8, v, sizeof v);
    }
    return MOE_OK;
}

int moe_plan_ramp(const moe_plan* p, float* ramp)
{
    if (!p || !ramp) return fail(MOE_EINVAL, "moe_plan_ramp: NULL argument");
    memcpy(ramp, p->p.ramp.data(), p->p.ramp.size() * 4);
    return MOE_OK;
}

// ---- stitch / run ------------------------------------------------------------------------------------
int64_t moe_plan_pool_elems(const moe_plan* p, int C)
{
    if (!p || C < 1) return fail(MOE_EINVAL, "moe_plan_pool_elems: bad argument");
    return (int64_t)(p->p.pool_elems_per_plane_set / p->p.C * C);
}

int moe_plan_tile_offsets(const moe_plan* p, int C, int64_t* off)
{
    if (!p || !off || C < 1) return fail(MOE_EINVAL, "moe_plan_tile_offsets: bad argument");
    for (size_t k = 0; k < p->p.tiles.size(); ++k) off[k] = p->p.tile_off[k] / p->p.C * C;
    return MOE_OK;
}

int moe_stitch(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off, int C, void* out, int out_dtype, void* stream)
{
    if (!p || !tiles_dev || !out || C < 1) return fail(MOE_EINVAL, "moe_stitch: bad argument");
    HIP_TRY(hipSetDevice(device));
    PlanDeviceCache* d = nullptr;
    int rc = plan_device_tables(p->p, device, C, 0, 0, 0, 0, 1, &d);
    if (rc) return rc;
    long long* toff = nullptr;
    if (tile_off) {   // caller-defined pool layout (e.g. the receive buffer of dist.py): uploaded once per distinct table, then cached on the plan
        const size_t nt = p->p.tiles.size();
        for (auto& c : p->p.custom_off)
            if (c.device == device && c.host.size() == nt && std::equal(c.host.begin(), c.host.end(), tile_off)) { toff = c.dev; break; }
        if (!toff) {
            if (p->p.custom_off.size() >= 16) {
                HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
                (void)hipFree(p->p.custom_off.front().dev);
                p->p.custom_off.erase(p->p.custom_off.begin());
            }
            HIP_TRY(hipMalloc((void**)&toff, nt * 8));
            HIP_TRY(hipMemcpy(toff, tile_off, nt * 8, hipMemcpyHostToDevice));
            p->p.custom_off.push_back(CustomOffsets{device, std::vector<long long>(tile_off, tile_off + nt), toff});
        }
    }
    StitchArgs a{};
    fill_stitch(p->p, *d, a, tiles_dev, toff ? toff : d->tile_off, C, out, out_dtype);
    launch_stitch(a, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "stitch launch failed: %s", hipGetErrorString(e));
    return MOE_OK;
}

int moe_stitch_dev(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, void* out, int out_dtype, void* stream)
{
    if (!p || !tiles_dev || !tile_off_dev || !out || C < 1) return fail(MOE_EINVAL, "moe_stitch_dev: bad argument");
    HIP_TRY(hipSetDevice(device));
    PlanDeviceCache* d = nullptr;
    int rc = plan_device_tables(p->p, device, C, 0, 0, 0, 0, 1, &d);
    if (rc) return rc;
    StitchArgs a{};
    fill_stitch(p->p, *d, a, tiles_dev, (const long long*)tile_off_dev, C, out, out_dtype);
    launch_stitch(a, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "stitch launch failed: %s", hipGetErrorString(e));
    return MOE_OK;
}

int moe_stitch_band(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, void* out, int out_dtype,
                    int row0, int row1, int strip, void* stream)
{
    if (!p || !tiles_dev || !tile_off_dev || !out || C < 1) return fail(MOE_EINVAL, "moe_stitch_band: bad argument");
    const Plan& q = p->p;
    const int nrow = q.ah.step;
    if (row0 < 0 || row1 <= row0 || row1 > nrow) return fail(MOE_EINVAL, "moe_stitch_band: tile rows [%d, %d) of %d", row0, row1, nrow);
    HIP_TRY(hipSetDevice(device));
    PlanDeviceCache* d = nullptr;
    int rc = plan_device_tables(q, device, C, 0, 0, 0, 0, 1, &d);
    if (rc) return rc;
    StitchArgs a{};
    fill_stitch(q, *d, a, tiles_dev, (const long long*)tile_off_dev, C, out, out_dtype);
    a.row_lo = row0;
    a.y0 = q.row_tab[row0 * 4 + 1];                                  // S(row0): first un-blended row of the band's first tile row (0 for row 0)
    a.rows = (row1 < nrow ? q.row_tab[row1 * 4 + 1] : q.out_h) - a.y0;
    if (strip && row1 < nrow) {
        // the band ends with the blend band of tile row row1, rows [first, solid): its tiles are present as STRIPS of exactly those pad_sc rows (C planes of
        // pad_sc x width each): a row table in which that tile row starts at `first` and is pad_sc high addresses them
        int* tab = nullptr;
        for (auto& e : d->strip_tabs) if (e.first == row1) tab = e.second;
        if (!tab) {
            std::vector<int> rt(q.row_tab);
            rt[row1 * 4 + 2] = rt[row1 * 4 + 0];
            rt[row1 * 4 + 3] = rt[row1 * 4 + 1] - rt[row1 * 4 + 0];
            HIP_TRY(hipMalloc((void**)&tab, rt.size() * 4));
            HIP_TRY(hipMemcpy(tab, rt.data(), rt.size() * 4, hipMemcpyHostToDevice));
            d->strip_tabs.push_back({row1, tab});
        }
        a.row_tab = tab;
    }
    launch_stitch(a, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "stitch launch failed: %s", hipGetErrorString(e));
    return MOE_OK;
}

int moe_blend_tile(const void* r, int64_t r_sC, int64_t r_sH, void* canvas, int64_t c_sC, int64_t c_sH, int dtype, int C,
                   int top_sc, int left_sc, int bsc, int rsc, int topT, int leftT, int pad_sc, const void* ramp, void* stream)
{
    if (!r || !canvas || C < 1) return fail(MOE_EINVAL, "moe_blend_tile: NULL argument");
    if (dtype != MOE_F32 && dtype != MOE_F16) return fail(MOE_EINVAL, "moe_blend_tile: dtype must be MOE_F32 or MOE_F16");
    const int rh = bsc - top_sc, rw = rsc - left_sc;
    if (rh < 1 || rw < 1 || top_sc < 0 || left_sc < 0 || pad_sc < 0) return fail(MOE_EINVAL, "moe_blend_tile: empty or negative window (%d..%d, %d..%d)", top_sc, bsc, left_sc, rsc);
    // blend(r, x, lt, pad, dim, ..), python/imageProcess.py:120-131: lt < 0 counts from the end; lt < 1: nothing is blended and the whole extent is assigned
    auto band = [&](int lt, int l, int& first, int& solid) {
        if (lt < 0) lt += l;
        if (lt < 1) { first = solid = 0; return true; }
        first = lt - pad_sc; solid = lt;
        return first >= 0 && lt <= l;
    };
    BlendTileArgs a{};
    if (!band(topT, rh, a.r0, a.lt_h) || !band(leftT, rw, a.c0, a.lt_w))
        return fail(MOE_EINVAL, "moe_blend_tile: blend band outside the window (topT %d, leftT %d, pad_sc %d, window %d x %d)", topT, leftT, pad_sc, rh, rw);
    if ((a.lt_h > a.r0 || a.lt_w > a.c0) && !ramp) return fail(MOE_EINVAL, "moe_blend_tile: ramp is NULL");
    a.r = r; a.canvas = canvas; a.ramp = ramp; a.r_sC = r_sC; a.r_sH = r_sH; a.c_sC = c_sC; a.c_sH = c_sH;
    a.C = C; a.rh = rh; a.rw = rw; a.top_sc = top_sc; a.left_sc = left_sc;
    launch_blend_tile(a, dtype == MOE_F16, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "blend launch failed: %s", hipGetErrorString(e));
    return MOE_OK;
}

int moe_run_plan_ex(moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                    void* out, int out_dtype, int max_tiles, float* pool, int shard_index, int shard_count, int do_stitch, void* stream)
{
    if (!n || !pl || !img || (do_stitch && !out)) return fail(MOE_EINVAL, "moe_run_plan: NULL argument");
    if (!n->finalized) return fail(MOE_ESTATE, "moe_run_plan: net is not finalized");
    const Plan& p = pl->p;
    if (p.sc != n->scale) return fail(MOE_EINVAL, "moe_run_plan: plan scale %d != net scale %d", p.sc, n->scale);
    if (shard_count < 1) { shard_count = 1; shard_index = 0; }
    if (shard_index < 0 || shard_index >= shard_count) return fail(MOE_EINVAL, "moe_run_plan: shard %d of %d", shard_index, shard_count);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(n->device));
    const int C = p.C;
    PlanDeviceCache* d = nullptr;
    int rc = plan_device_tables(p, n->device, C, sC, sH, sW, shard_index, shard_count, &d);
    if (rc) return rc;
    if (!pool) {
        const size_t pool_need = p.pool_elems_per_plane_set;
        if (pool_need > p.pool_elems) {
            if (p.pool) { HIP_TRY(hipStreamSynchronize(s)); HIP_TRY(hipFree(p.pool)); p.pool = nullptr; p.pool_elems = 0; }
            if (hipMalloc((void**)&p.pool, pool_need * 4) != hipSuccess) { (void)hipGetLastError(); return fail(MOE_ENOMEM, "tile pool of %zu bytes does not fit", pool_need * 4); }
            p.pool_elems = pool_need;
        }
        pool = p.pool;
    }
    if (max_tiles <= 0) {
        max_tiles = n->opt.tiles_per_batch > 0 ? n->opt.tiles_per_batch : 32;     // (tiles of 256^2 pixels per launch set: 28.97 / 28.59 / 28.42 / 28.28 / 28.33 ms per 1080p x4 frame with 4 / 8 / 12 / 16 / 24 in round 3: fewer pipeline
                                                                                   // fills per pixel; round 4's kernels, 16 / 20 / 28: 24.32 / 24.20 / 24.09 -- the 28 full tiles of a 1080p frame as ONE launch set; a tile's bits do not depend on it)
    }
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const auto& g = p.groups[gi];
        const int nt = d->group_count[gi];
        if (nt < 1) continue;
        // bigger batches for small tiles: keep roughly max_tiles * 256^2 pixels per launch
        const long long px = (long long)g.th * g.tw;
        const int per = (int)std::max<long long>(1, std::min<long long>(nt, (long long)max_tiles * 65536 / std::max<long long>(px, 1)));
        for (int t0 = 0; t0 < nt; t0 += per) {
            const int cnt = std::min(per, nt - t0);
            const long long slot = (long long)(d->group_first[gi] + t0) * C;
            rc = forward_dev(*n, FwdIO{img, img_dtype, 0, sH, sW, d->x_off + slot, pool, MOE_F32, d->y_off + slot}, cnt * C, g.th, g.tw, s, d->y_mult8, own_ctx(*n, &n->set));
            if (rc) return rc;
        }
    }
    if (do_stitch) {
        StitchArgs a{};
        fill_stitch(p, *d, a, pool, d->tile_off, C, out, out_dtype);
        launch_stitch(a, s);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(MOE_EHIP, "stitch launch failed: %s", hipGetErrorString(e));
    }
    return MOE_OK;
}

int moe_run_plan_tiles(moe_net* n, const moe_plan* pl, const void* imgs, int img_dtype, int64_t frame_stride,
                       int64_t sC, int64_t sH, int64_t sW, int n_frames, float* dst, const int64_t* tile_dst,
                       int max_tiles, void* stream)
{
    if (!n || !pl || !imgs || !dst || !tile_dst || n_frames < 1) return fail(MOE_EINVAL, "moe_run_plan_tiles: bad argument");
    if (!n->finalized) return fail(MOE_ESTATE, "moe_run_plan_tiles: net is not finalized");
    const Plan& p = pl->p;
    if (p.sc != n->scale) return fail(MOE_EINVAL, "moe_run_plan_tiles: plan scale %d != net scale %d", p.sc, n->scale);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(n->device));
    const int C = p.C;
    const long long nt = (long long)p.tiles.size();
    FramesDeviceCache* d = nullptr;
    for (auto& up : p.fdev) {
        FramesDeviceCache& c = *up;
        if (c.blob && c.device == n->device && c.C == C && c.sC == sC && c.sH == sH && c.sW == sW && c.frame_stride == frame_stride &&
            c.n_frames == n_frames && c.tile_dst.size() == (size_t)(nt * n_frames) &&
            std::equal(c.tile_dst.begin(), c.tile_dst.end(), tile_dst)) { d = &c; break; }
    }
    if (!d) {
        if (p.fdev.size() >= 8) {
            HIP_TRY(hipStreamSynchronize(s));
            if (p.fdev.front()->blob) (void)hipFree(p.fdev.front()->blob);
            p.fdev.erase(p.fdev.begin());
        }
        p.fdev.push_back(std::make_unique<FramesDeviceCache>());
        d = p.fdev.back().get();
        std::vector<long long> xo, yo;
        int slot = 0;
        for (const auto& g : p.groups) {      // same-shaped tiles of ALL frames share launches
            d->group_first.push_back(slot);
            int cnt = 0;
            const long long plane = (long long)(g.th * p.sc) * (g.tw * p.sc);
            for (int f = 0; f < n_frames; ++f)
                for (int k : g.tiles) {
                    const long long at = tile_dst[(long long)f * nt + k];
                    if (at < 0) continue;                                  // not computed by this call
                    const TileRect& t = p.tiles[k];
                    for (int c = 0; c < C; ++c) {
                        xo.push_back((long long)f * frame_stride + (long long)c * sC + (long long)t.top * sH + (long long)t.left * sW);
                        yo.push_back(at + (long long)c * plane);
                    }
                    ++slot; ++cnt;
                }
            d->group_count.push_back(cnt);
        }
        if (xo.empty()) { xo.push_back(0); yo.push_back(0); }
        d->y_mult8 = true;
        for (long long v : yo) d->y_mult8 = d->y_mult8 && (v % 8 == 0);
        HIP_TRY(hipMalloc(&d->blob, xo.size() * 16));
        d->x_off = (long long*)d->blob; d->y_off = d->x_off + xo.size();
        HIP_TRY(hipMemcpy(d->x_off, xo.data(), xo.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->y_off, yo.data(), yo.size() * 8, hipMemcpyHostToDevice));
        d->device = n->device; d->C = C; d->sC = sC; d->sH = sH; d->sW = sW; d->frame_stride = frame_stride;
        d->n_frames = n_frames; d->tile_dst.assign(tile_dst, tile_dst + nt * n_frames);
    }
    if (max_tiles <= 0) {
        max_tiles = n->opt.tiles_per_batch > 0 ? n->opt.tiles_per_batch : 32;     // (as moe_run_plan_ex)
    }
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const auto& g = p.groups[gi];
        const int ntl = d->group_count[gi];
        if (ntl < 1) continue;
        const long long px = (long long)g.th * g.tw;
        const int per = (int)std::max<long long>(1, std::min<long long>(ntl, (long long)max_tiles * 65536 / std::max<long long>(px, 1)));
        for (int t0 = 0; t0 < ntl; t0 += per) {
            const int cnt = std::min(per, ntl - t0);
            const long long slot = (long long)(d->group_first[gi] + t0) * C;
            int rc = forward_dev(*n, FwdIO{imgs, img_dtype, 0, sH, sW, d->x_off + slot, dst, MOE_F32, d->y_off + slot}, cnt * C, g.th, g.tw, s, d->y_mult8, own_ctx(*n, &n->set));
            if (rc) return rc;
        }
    }
    return MOE_OK;
}

int moe_run_plan_frames(moe_net* n, const moe_plan* pl, const void* imgs, int img_dtype, int64_t frame_stride,
                        int64_t sC, int64_t sH, int64_t sW, int n_frames, float* pools, int64_t pool_stride,
                        int owner_index, int owner_count, int max_tiles, void* stream)
{
    if (!n || !pl || !imgs || !pools || n_frames < 1) return fail(MOE_EINVAL, "moe_run_plan_frames: bad argument");
    const Plan& p = pl->p;
    if (owner_count < 1) { owner_count = 1; owner_index = 0; }
    if (owner_index < 0 || owner_index >= owner_count) return fail(MOE_EINVAL, "moe_run_plan_frames: owner %d of %d", owner_index, owner_count);
    if (pool_stride < (int64_t)p.pool_elems_per_plane_set) return fail(MOE_EINVAL, "moe_run_plan_frames: pool stride smaller than one frame's pool");
    const long long nt = (long long)p.tiles.size();
    std::vector<int64_t> at((size_t)(nt * n_frames));
    for (int f = 0; f < n_frames; ++f)
        for (long long k = 0; k < nt; ++k)
            at[(size_t)(f * nt + k)] = ((f * nt + k) % owner_count == owner_index) ? (int64_t)f * pool_stride + p.tile_off[(size_t)k] : -1;
    return moe_run_plan_tiles(n, pl, imgs, img_dtype, frame_stride, sC, sH, sW, n_frames, pools, at.data(), max_tiles, stream);
}

int moe_run_plan(moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                 void* out, int out_dtype, int max_tiles, void* stream)
{
    return moe_run_plan_ex(n, pl, img, img_dtype, sC, sH, sW, out, out_dtype, max_tiles, nullptr, 0, 1, 1, stream);
}

// ---- self-ensemble (python/imageProcess.py:563-572, runSR.py:26) ------------------------------------------
// symmetry s = 0..6 in the order of the reference's `trans` list as (transpose first, flip width, flip height); -1 = the identity
struct Sym { int t, fh, fv; };
static Sym sym_of(int s)
{
    static const Sym tab[7] = {{1, 0, 0}, {0, 1, 0}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {0, 0, 1}, {1, 1, 1}};
    return s < 0 ? Sym{0, 0, 0} : tab[s];
}

static int sym_launched(const char* who)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "%s launch failed: %s", who, hipGetErrorString(e));
    return MOE_OK;
}

// dst (C, Hp, Wp) = padImage(trans_s(src)); src = (C, H, W) with element strides
static int sym_pad(const void* src, bool f16, int C, int H, int W, int64_t sC, int64_t sH, int64_t sW, int s, void* dst, int Hp, int Wp, hipStream_t st)
{
    const Sym y = sym_of(s);
    SymArgs a{};
    a.src = src; a.dst = dst; a.sC = sC; a.sH = sH; a.sW = sW; a.C = C; a.Hd = Hp; a.Wd = Wp;
    a.nR = y.t ? W : H; a.nC = y.t ? H : W; a.flipR = y.fv; a.flipC = y.fh;
    launch_sym(a, f16, false, y.t != 0, st);
    return sym_launched("moe_sym_pad");
}

// acc (C, H, W) += transInv_s(t); t = (C, Ht, Wt) contiguous, the canvas of the transformed image
static int sym_fold(void* acc, const void* t, bool f16, int C, int H, int W, int s, int final_div, hipStream_t st)
{
    const Sym y = sym_of(s);
    const int Wt = y.t ? H : W;
    SymArgs a{};
    a.src = t; a.dst = acc; a.sC = (long long)H * W; a.sH = Wt; a.sW = 1; a.C = C; a.Hd = H; a.Wd = W;
    a.nR = H; a.nC = W;
    a.flipR = y.t ? y.fh : y.fv; a.flipC = y.t ? y.fv : y.fh;       // (transposed, acc's rows run along t's columns: the flip of t's width reverses them)
    a.div = final_div > 1; a.inv = 1.0f / (float)(final_div > 1 ? final_div : 1);
    launch_sym(a, f16, true, y.t != 0, st);
    return sym_launched("moe_sym_fold");
}

static bool sym_dtype(int dtype) { return dtype == MOE_F32 || dtype == MOE_F16; }

int moe_sym_pad(const void* src, int dtype, int C, int H, int W, int64_t sC, int64_t sH, int64_t sW, int sym, void* dst, int Hp, int Wp, int device, void* stream)
{
    if (!src || !dst) return fail(MOE_EINVAL, "moe_sym_pad: NULL argument");
    if (!sym_dtype(dtype)) return fail(MOE_EINVAL, "moe_sym_pad: dtype must be MOE_F32 or MOE_F16");
    if (sym < 0 || sym > 6) return fail(MOE_EINVAL, "moe_sym_pad: sym %d is not one of the seven symmetries 0..6", sym);
    if (C < 1 || H < 1 || W < 1) return fail(MOE_EINVAL, "moe_sym_pad: size %d x %d x %d must be positive", C, H, W);
    const Sym y = sym_of(sym);
    const int Ht = y.t ? W : H, Wt = y.t ? H : W;
    if (Hp < Ht || Wp < Wt) return fail(MOE_EINVAL, "moe_sym_pad: padded size %d x %d is smaller than the transformed image %d x %d", Hp, Wp, Ht, Wt);
    HIP_TRY(hipSetDevice(device));
    return sym_pad(src, dtype == MOE_F16, C, H, W, sC, sH, sW, sym, dst, Hp, Wp, (hipStream_t)stream);
}

int moe_sym_fold(void* acc, const void* t, int dtype, int C, int H, int W, int sym, int final_div, int device, void* stream)
{
    if (!acc || !t) return fail(MOE_EINVAL, "moe_sym_fold: NULL argument");
    if (!sym_dtype(dtype)) return fail(MOE_EINVAL, "moe_sym_fold: dtype must be MOE_F32 or MOE_F16");
    if (sym < 0 || sym > 6) return fail(MOE_EINVAL, "moe_sym_fold: sym %d is not one of the seven symmetries 0..6", sym);
    if (C < 1 || H < 1 || W < 1) return fail(MOE_EINVAL, "moe_sym_fold: size %d x %d x %d must be positive", C, H, W);
    if (final_div < 0) return fail(MOE_EINVAL, "moe_sym_fold: final_div %d is negative (0 or 1: no division)", final_div);
    HIP_TRY(hipSetDevice(device));
    return sym_fold(acc, t, dtype == MOE_F16, C, H, W, sym, final_div, (hipStream_t)stream);
}

}  // extern "C"

void moe::free_ens_scratch(moe_net& n)
{
    if (n.ens_pad) (void)hipFree(n.ens_pad);
    if (n.ens_canvas) (void)hipFree(n.ens_canvas);
    n.ens_pad = n.ens_canvas = nullptr;
    n.ens_pad_bytes = n.ens_canvas_bytes = 0;
}

// grow-only, like the workspace: work enqueued on `s` may still read the old block
static int ens_grow(void*& buf, size_t& have, size_t need, hipStream_t s, const char* what)
{
    if (need <= have) return MOE_OK;
    if (buf) { HIP_TRY(hipStreamSynchronize(s)); HIP_TRY(hipFree(buf)); buf = nullptr; have = 0; }
    if (hipMalloc(&buf, need) != hipSuccess) { (void)hipGetLastError(); buf = nullptr; return fail(MOE_ENOMEM, "moe_run_plan_ens: %s of %zu bytes does not fit", what, need); }
    have = need;
    return MOE_OK;
}

static int run_plan_ens(moe_net* n, const moe_plan* pl, const moe_plan* pl_t, int n_sym, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                        void* out, int out_dtype, int max_tiles, hipStream_t s)
{
    const Plan& p = pl->p;
    const bool f16_in = img_dtype == MOE_F16, f16_out = out_dtype == MOE_F16;
    const size_t es_in = f16_in ? 2 : 4, es_out = f16_out ? 2 : 4;
    auto padded = [](const Plan& q, int& hp, int& wp) { hp = std::max(q.H, q.pad_h_to); wp = std::max(q.W, q.pad_w_to); };
    int hp, wp, hpt = 0, wpt = 0;
    padded(p, hp, wp);
    size_t pad_need = (size_t)p.C * hp * wp * es_in, canvas_need = 0;
    if (n_sym > 0) {
        canvas_need = (size_t)p.C * p.out_h * p.out_w * es_out;
        padded(pl_t->p, hpt, wpt);
        pad_need = std::max(pad_need, (size_t)p.C * hpt * wpt * es_in);
    }
    int rc = ens_grow(n->ens_pad, n->ens_pad_bytes, pad_need, s, "the padded image");
    if (!rc && canvas_need) rc = ens_grow(n->ens_canvas, n->ens_canvas_bytes, canvas_need, s, "a symmetry's canvas");
    if (rc) return rc;
    // v = doCrop(x)
    rc = sym_pad(img, f16_in, p.C, p.H, p.W, sC, sH, sW, -1, n->ens_pad, hp, wp, s);
    if (!rc) rc = moe_run_plan(n, pl, n->ens_pad, img_dtype, (int64_t)hp * wp, wp, 1, out, out_dtype, max_tiles, s);
    // v = v + transInv[i](doCrop(trans[i](x))), the closing / (n + 1) inside the last fold
    for (int i = 0; i < n_sym && !rc; ++i) {
        const bool t = sym_of(i).t != 0;
        const int h = t ? hpt : hp, w = t ? wpt : wp;
        rc = sym_pad(img, f16_in, p.C, p.H, p.W, sC, sH, sW, i, n->ens_pad, h, w, s);
        if (!rc) rc = moe_run_plan(n, t ? pl_t : pl, n->ens_pad, img_dtype, (int64_t)h * w, w, 1, n->ens_canvas, out_dtype, max_tiles, s);
        if (!rc) rc = sym_fold(out, n->ens_canvas, f16_out, p.C, p.out_h, p.out_w, i, i == n_sym - 1 ? n_sym + 1 : 0, s);
    }
    return rc;
}

extern "C" {

int moe_run_plan_ens(moe_net* n, const moe_plan* pl, const moe_plan* pl_t, int n_sym, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                     void* out, int out_dtype, int max_tiles, void* stream)
{
    if (!n || !pl || !img || !out) return fail(MOE_EINVAL, "moe_run_plan_ens: NULL argument");
    if (n_sym < 0 || n_sym > 7) return fail(MOE_EINVAL, "moe_run_plan_ens: n_sym %d is not in 0..7", n_sym);
    if (!sym_dtype(img_dtype) || !sym_dtype(out_dtype)) return fail(MOE_EINVAL, "moe_run_plan_ens: dtype must be MOE_F32 or MOE_F16");
    const Plan& p = pl->p;
    if (n_sym > 0) {       // (symmetry 0 is the transpose: every ensemble needs the transposed shape's plan)
        if (!pl_t) return fail(MOE_EINVAL, "moe_run_plan_ens: plan_t is NULL (n_sym %d needs the plan of the transposed shape)", n_sym);
        const Plan& q = pl_t->p;
        if (q.C != p.C || q.H != p.W || q.W != p.H || q.sc != p.sc)
            return fail(MOE_EINVAL, "moe_run_plan_ens: plan_t is for %d x %d x %d (scale %d), not the transpose of %d x %d x %d (scale %d)", q.C, q.H, q.W, q.sc, p.C, p.H, p.W, p.sc);
        if (q.out_h != p.out_w || q.out_w != p.out_h)
            return fail(MOE_EINVAL, "moe_run_plan_ens: the two plans disagree on the output shape (%d x %d against %d x %d transposed)", p.out_h, p.out_w, q.out_h, q.out_w);
    }
    if (!n->finalized) return fail(MOE_ESTATE, "moe_run_plan_ens: net is not finalized");
    int prev = -1;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(n->device));
    const int rc = run_plan_ens(n, pl, pl_t, n_sym, img, img_dtype, sC, sH, sW, out, out_dtype, max_tiles, (hipStream_t)stream);
    if (prev >= 0 && prev != n->device) (void)hipSetDevice(prev);      // (the scratch is allocated on the net's device; the caller's current device is as it was)
    return rc;
}

// ---- image edges ---------------------------------------------------------------------------------------
int moe_to_float(const void* src, int src_dtype, int bits, int H, int W, int C, void* dst, int dst_dtype, int device, void* stream)
{
    if (!src || !dst || H < 1 || W < 1 || C < 1) return fail(MOE_EINVAL, "moe_to_float: bad argument");
    if ((src_dtype != MOE_U8 && src_dtype != MOE_U16) || (dst_dtype != MOE_F32 && dst_dtype != MOE_F16)) return fail(MOE_EINVAL, "moe_to_float: bad dtype");
    HIP_TRY(hipSetDevice(device));
    if (src_dtype == MOE_U8) launch_to_float(src, src_dtype, 255.f, true, H, W, C, dst, dst_dtype, (hipStream_t)stream);
    else launch_to_float(src, src_dtype, 1.f / (float)(1 << bits), false, H, W, C, dst, dst_dtype, (hipStream_t)stream);
    return MOE_OK;
}

int moe_resize(const void* src, void* dst, int dtype, int C, int H, int W, int h, int w, int mode, int device, void* stream)
{
    if (!src || !dst || C < 1 || H < 1 || W < 1 || h < 1 || w < 1) return fail(MOE_EINVAL, "moe_resize: bad argument");
    if (dtype != MOE_F32 && dtype != MOE_F16) return fail(MOE_EINVAL, "moe_resize: dtype must be MOE_F32 or MOE_F16");
    if (mode < MOE_RESIZE_NEAREST || mode > MOE_RESIZE_BICUBIC) return fail(MOE_EINVAL, "moe_resize: unknown mode %d", mode);
    HIP_TRY(hipSetDevice(device));
    launch_resize(src, dst, dtype, C, H, W, h, w, mode, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "resize launch failed: %s", hipGetErrorString(e));
    return MOE_OK;
}

int moe_to_output(const void* src, int src_dtype, int H, int W, int C, int bits, void* dst, int dst_dtype, int device, void* stream)
{
    if (!src || !dst || H < 1 || W < 1 || C < 1 || bits < 1 || bits > 16) return fail(MOE_EINVAL, "moe_to_output: bad argument");
    if ((dst_dtype != MOE_U8 && dst_dtype != MOE_U16) || (src_dtype != MOE_F32 && src_dtype != MOE_F16)) return fail(MOE_EINVAL, "moe_to_output: bad dtype");
    if (dst_dtype == MOE_U8 && bits > 8) return fail(MOE_EINVAL, "moe_to_output: %d bits do not fit MOE_U8", bits);
    HIP_TRY(hipSetDevice(device));
    launch_to_output(src, src_dtype, H, W, C, (float)(1 << bits), dst, dst_dtype, (hipStream_t)stream);
    return MOE_OK;
}

}  // extern "C"
