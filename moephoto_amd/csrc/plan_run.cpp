// plan_run.cpp -- the device-resident doCrop (tile gather -> net -> stitch: python/imageProcess.py:157-172).  A plan handle owns the planner's result and, beside it,
// its device state: TILE TABLES (which planes of which image go where: built by tile_table from an input layout and a (frame, tile) -> destination table, one bounded
// cache), the stitch tables of a (device, C) and the internal tile pool.  Every moe_run_plan* runner is a destination table + run_sets, the one loop that cuts a
// table's groups into launch sets; every stitch is stitch().  Also here: the planner's entry points, the inter-rank wire format, the self-ensemble and the image edges
// between floats and samples (the integer resamplers of planar codes, moe_chroma_resample and moe_fit_*, are polyphase.cpp's).
#include "net.h"

using namespace moe;

// =====================================================================================================
// the plan handle's device state
// =====================================================================================================
// Which planes go where, for one call's worth of work: per plan group the (frame, tile) pairs the destination table names, in (frame, raster) order, C planes each.
struct TileTable {
    int device = -1, n_frames = 0;                         // the key: the input layout and the destination table the device tables were built from
    int64_t sC = 0, sH = 0, sW = 0, frame_stride = 0;
    std::vector<int64_t> tile_dst;
    bool y_mult8 = false;                                  // every y_off entry is a multiple of 8 elements (16-byte aligned output planes)
    std::vector<int> group_first, group_count;             // per plan group: first slot / number of its pairs
    void* dev = nullptr;                                   // one allocation: [slot][C] each, the plane's offset in the images / in the destination
    const long long *x_off = nullptr, *y_off = nullptr;
};

struct StitchTables {      // what the stitch kernel reads of a plan besides the tiles: a function of (device, C) alone, uploaded once
    int device = -1, C = 0;
    void* dev = nullptr;
    long long* tile_off = nullptr;     // the plan's own pool layout for C planes, raster order
    int *row_first = nullptr, *row_cnt = nullptr, *col_first = nullptr, *col_cnt = nullptr, *row_tab = nullptr, *col_tab = nullptr;
    float* ramp = nullptr;
    std::vector<std::pair<int, int*>> strip_tabs;   // moe_stitch_band: row tables in which one tile row is present as the strip of its blend band
};

struct UploadedOffsets { int device; std::vector<int64_t> host; void* dev; };   // a caller's pool layout passed to moe_stitch from the host

// moe_run_plan_subset's offset tables.  Its mask is new with every frame, and the cache of tile tables would answer that with a stream synchronise, a hipFree, a hipMalloc
// and a blocking copy per call once its 16 entries are taken.  The ring is one device block and one pinned host block of kSlots tables each, sized once for the plan's
// largest table (every tile, C planes, x and y offsets) on first use; a call fills the next slot's host half, sends it with hipMemcpyAsync on the caller's stream in
// front of its launch sets and records the slot's event behind them.  A slot is taken again kSlots calls later and only once that event has passed: both halves are then
// free, whatever stream the next call runs on.  A caller that is fewer than kSlots calls ahead of the device -- the frame stream: ring depth x steps x images -- finds
// the event passed; only one that is further ahead waits for that one event.  Nothing is allocated or freed after the first call, no stream is synchronised.
struct TableRing {
    static constexpr int kSlots = 32;
    int device = -1;
    size_t slot_bytes = 0;
    char *host = nullptr, *dev = nullptr;
    hipEvent_t done[kSlots] = {};
    bool used[kSlots] = {};
    int next = 0;
};

struct PlanDevice {
    static constexpr size_t kCached = 16;      // tile tables / uploaded layouts kept; the oldest goes first
    std::vector<TileTable> tables;
    std::vector<StitchTables> stitch;          // (a handful: one per device and channel count the plan is stitched with)
    std::vector<UploadedOffsets> uploaded;
    std::vector<TableRing> rings;              // (one per device the plan's subsets ran on)
    DevBuf pool;                               // per-tile fp32 results when the caller passes no pool
    ~PlanDevice()
    {
        for (auto& t : tables) (void)hipFree(t.dev);
        for (auto& t : stitch) { (void)hipFree(t.dev); for (auto& e : t.strip_tabs) (void)hipFree(e.second); }
        for (auto& u : uploaded) (void)hipFree(u.dev);
        for (auto& r : rings) {
            for (hipEvent_t e : r.done) if (e) (void)hipEventDestroy(e);
            (void)hipHostFree(r.host);
            (void)hipFree(r.dev);
        }
        pool.release();
    }
    // Room for one more entry of `tables` or `uploaded`.  The dropped entry's block may still be read by kernels in flight: the runners and the stitch enqueue on the
    // caller's stream, which is synchronised here, and hipFree itself waits for every other stream of the device -- nothing reads the block once it has returned.
    template <typename V> static int make_room(V& v, hipStream_t s)
    {
        if (v.size() < kCached) return MOE_OK;
        HIP_TRY(hipStreamSynchronize(s));
        (void)hipFree(v.front().dev);
        v.erase(v.begin());
        return MOE_OK;
    }
};

static int upload(const void* host, size_t bytes, void** dev)
{
    HIP_TRY(hipMalloc(dev, bytes));
    const hipError_t e = hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(*dev); *dev = nullptr; }
    HIP_TRY(e);
    return MOE_OK;
}

struct moe_plan { Plan p; mutable PlanDevice dev; };      // (the ABI's runners and stitches take the plan as const: the device state is a cache beside it)

// The rows of a tile table: per plan group the (frame, tile) pairs tile_dst names with their planes' offsets in the images (x) and in the destination (y), and what
// run_sets reads of the table besides them (the groups' slots, y_mult8).  At least one row, so that no table is empty.
static void table_rows(const Plan& p, int64_t frame_stride, int64_t sC, int64_t sH, int64_t sW, int n_frames, const int64_t* tile_dst, TileTable& d,
                       std::vector<long long>& off, std::vector<long long>& yo)
{
    int slot = 0;
    for (const auto& g : p.groups) {     // same-shaped tiles of ALL frames share launches
        d.group_first.push_back(slot);
        const long long plane = (long long)(g.th * p.sc) * (g.tw * p.sc);
        for (int f = 0; f < n_frames; ++f)
            for (int k : g.tiles) {
                const long long at = tile_dst[(size_t)f * p.tiles.size() + k];
                if (at < 0) continue;                                  // not computed by this call
                const TileRect& t = p.tiles[k];
                for (int c = 0; c < p.C; ++c) {
                    off.push_back((long long)f * frame_stride + (long long)c * sC + (long long)t.top * sH + (long long)t.left * sW);
                    yo.push_back(at + (long long)c * plane);
                }
                ++slot;
            }
        d.group_count.push_back(slot - d.group_first.back());
    }
    if (off.empty()) { off.push_back(0); yo.push_back(0); }
    d.y_mult8 = true;
    for (long long v : yo) d.y_mult8 = d.y_mult8 && (v % 8 == 0);
}

// the tile table of (input layout, destination table): tile_dst[f * n_tiles + k] is where frame f's tile k goes, -1 = not computed by this call
static int tile_table(const moe_plan& pl, int device, int64_t frame_stride, int64_t sC, int64_t sH, int64_t sW, int n_frames, const int64_t* tile_dst,
                      hipStream_t s, const TileTable** out)
{
    const Plan& p = pl.p;
    const size_t n = p.tiles.size() * (size_t)n_frames;      // (entries of tile_dst; equal n_frames: equal sizes)
    for (const TileTable& c : pl.dev.tables)
        if (c.device == device && c.sC == sC && c.sH == sH && c.sW == sW && c.frame_stride == frame_stride && c.n_frames == n_frames &&
            std::equal(c.tile_dst.begin(), c.tile_dst.end(), tile_dst)) { *out = &c; return MOE_OK; }
    int rc = PlanDevice::make_room(pl.dev.tables, s);
    if (rc) return rc;
    TileTable d;
    std::vector<long long> off, yo;      // x_off, then y_off behind it
    table_rows(p, frame_stride, sC, sH, sW, n_frames, tile_dst, d, off, yo);
    off.insert(off.end(), yo.begin(), yo.end());
    rc = upload(off.data(), off.size() * 8, &d.dev);
    if (rc) return rc;
    d.x_off = (const long long*)d.dev; d.y_off = d.x_off + yo.size();
    d.device = device; d.sC = sC; d.sH = sH; d.sW = sW; d.frame_stride = frame_stride; d.n_frames = n_frames;
    d.tile_dst.assign(tile_dst, tile_dst + n);
    pl.dev.tables.push_back(std::move(d));
    *out = &pl.dev.tables.back();
    return MOE_OK;
}

// The launch sets of one table: every group's planes through the net, `max_tiles` tiles' worth of 256^2 pixels at a time, from the image(s) into dst.
static int run_sets(moe_net& n, const Plan& p, const TileTable& d, const void* img, int img_dtype, int64_t sH, int64_t sW, float* dst, int max_tiles, hipStream_t s)
{
    if (max_tiles <= 0) {
        max_tiles = n.opt.tiles_per_batch > 0 ? n.opt.tiles_per_batch : 32;      // (tiles of 256^2 pixels per launch set: 28.97 / 28.59 / 28.42 / 28.28 / 28.33 ms per 1080p x4 frame with 4 / 8 / 12 / 16 / 24 in round 3: fewer pipeline
                                                                                   // fills per pixel; round 4's kernels, 16 / 20 / 28: 24.32 / 24.20 / 24.09 -- the 28 full tiles of a 1080p frame as ONE launch set; a tile's bits do not depend on it)
    }
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const auto& g = p.groups[gi];
        const int nt = d.group_count[gi];
        if (nt < 1) continue;
        // bigger batches for small tiles: keep roughly max_tiles * 256^2 pixels per launch
        const long long px = (long long)g.th * g.tw;
        const int per = (int)std::max<long long>(1, std::min<long long>(nt, (long long)max_tiles * 65536 / std::max<long long>(px, 1)));
        for (int t0 = 0; t0 < nt; t0 += per) {
            const int cnt = std::min(per, nt - t0);
            const long long slot = (long long)(d.group_first[gi] + t0) * p.C;
            int rc = forward_dev(n, FwdIO{img, img_dtype, 0, sH, sW, d.x_off + slot, dst, MOE_F32, d.y_off + slot}, cnt * p.C, g.th, g.tw, s, d.y_mult8, own_ctx(n, &n.set));
            if (rc) return rc;
        }
    }
    return MOE_OK;
}

static int stitch_tables(const moe_plan& pl, int device, int C, StitchTables** out)
{
    for (StitchTables& c : pl.dev.stitch)
        if (c.device == device && c.C == C) { *out = &c; return MOE_OK; }
    const Plan& p = pl.p;
    // tile_off scaled to C planes (C may differ from the planning shape's channel count, e.g. alpha stripped)
    std::vector<long long> toff(p.tiles.size());
    for (size_t k = 0; k < toff.size(); ++k) toff[k] = p.tile_off[k] / p.C * C;
    std::vector<char> host;
    auto put = [&](const void* src, size_t bytes) { const size_t a = (host.size() + 255) & ~(size_t)255; host.resize(a + bytes); memcpy(host.data() + a, src, bytes); return a; };
    const size_t o_t = put(toff.data(), toff.size() * 8);
    const size_t o_rf = put(p.row_first.data(), p.row_first.size() * 4), o_rc = put(p.row_cnt.data(), p.row_cnt.size() * 4);
    const size_t o_cf = put(p.col_first.data(), p.col_first.size() * 4), o_cc = put(p.col_cnt.data(), p.col_cnt.size() * 4);
    const size_t o_rt = put(p.row_tab.data(), p.row_tab.size() * 4), o_ct = put(p.col_tab.data(), p.col_tab.size() * 4);
    const float zero = 0.f;
    const size_t o_rp = put(p.ramp.empty() ? &zero : p.ramp.data(), std::max<size_t>(4, p.ramp.size() * 4));
    StitchTables d;
    int rc = upload(host.data(), host.size(), &d.dev);
    if (rc) return rc;
    char* b = (char*)d.dev;
    d.device = device; d.C = C; d.tile_off = (long long*)(b + o_t);
    d.row_first = (int*)(b + o_rf); d.row_cnt = (int*)(b + o_rc); d.col_first = (int*)(b + o_cf); d.col_cnt = (int*)(b + o_cc);
    d.row_tab = (int*)(b + o_rt); d.col_tab = (int*)(b + o_ct); d.ramp = (float*)(b + o_rp);
    pl.dev.stitch.push_back(std::move(d));
    *out = &pl.dev.stitch.back();
    return MOE_OK;
}

// The stitch of C planes from `tiles` into `out`.  tile_off: where each tile lies in `tiles` -- NULL = the plan's own pool layout, else a table on the device or
// (off_on_host: uploaded once per distinct table, then kept on the plan -- e.g. a receive buffer's layout) on the host.  band: NULL = the whole canvas, else
// {row0, row1, strip}: the rows of tile rows [row0, row1) only, strip != 0 with tile row row1 present as the strips of its blend band.
// edge: NULL = `out` is the canvas (C, rows, out_w) of out_dtype; else `out` is the quantised interleaved image (out_h, out_w, C) of out_dtype MOE_U8 / MOE_U16
// (moe_stitch_out: the whole canvas only); with mix the DN step's blend and alpha ride in the fold too (moe_stitch_mix: canvas or samples, mix->quant says which);
// with yuv `out` is the planar Y'CbCr 4:2:0 frame (moe_stitch_yuv: three planes, the whole canvas); with planes_depth `out` is C planes of samples at that depth
// (moe_stitch_planes: the whole canvas).
// With luma the C planes are Y' (and alpha) and `out` receives the C + 2 colour planes of a luma-only step's merge
// (moe_stitch_luma: canvas or samples, luma->quant says which).
// dq: the rounding / ordered-dither quantiser of the sample forms (MOE_Q_*: quant_flags below), NULL = today's; yuv_dither: the same request for the Y'CbCr edge (0, 1 = round, 2 = ordered).
struct OutEdge { int canvas_dtype; float quant; const StitchMix* mix = nullptr; const YuvEdge* yuv = nullptr; int planes_depth = 0; const StitchLuma* luma = nullptr;
                 const QuantDither* dq = nullptr; int yuv_dither = 0; };

// The MOE_Q_* flags OR-ed into a `bits` / `depth` argument, checked before any device call.  low: the argument's low byte, validated by the caller exactly as before; an
// argument with any other high bit (or a negative one) is handed on whole, so that the caller's own check refuses it as the unknown bits / depth it always was.
// dither: 0 = none, 1 = MOE_Q_ROUND, 2 = MOE_Q_ORDERED.  unit_ok: the edge has a unit scale (the three *yuv* calls quantise in integers: they have none).
struct QuantReq {
    int low = 0, dither = 0; bool unit = false; QuantDither d{};
    const QuantDither* dq() { return dither ? &d : nullptr; }
    void fill() { const float top = (float)((1 << low) - 1); d = QuantDither{unit ? top : top + 1.f, top, dither == 2}; }      // (after the caller has validated low)
};
static int quant_flags(const char* who, int arg, bool unit_ok, QuantReq* q)
{
    const int known = MOE_Q_ROUND | MOE_Q_ORDERED | MOE_Q_UNIT, flags = arg & ~0xff;
    *q = QuantReq{};
    q->low = arg;
    if (arg < 0 || (flags & ~known)) return MOE_OK;
    q->low = arg & 0xff;
    if ((flags & MOE_Q_ROUND) && (flags & MOE_Q_ORDERED)) return fail(MOE_EINVAL, "%s: MOE_Q_ROUND and MOE_Q_ORDERED are both set (one mode at most)", who);
    if ((flags & MOE_Q_UNIT) && !(flags & (MOE_Q_ROUND | MOE_Q_ORDERED))) return fail(MOE_EINVAL, "%s: MOE_Q_UNIT without MOE_Q_ROUND or MOE_Q_ORDERED (the truncating quantiser has no unit scale)", who);
    if ((flags & MOE_Q_UNIT) && !unit_ok) return fail(MOE_EINVAL, "%s: MOE_Q_UNIT does not apply to the Y'CbCr edge (its samples are quantised in integers)", who);
    if (flags && q->low == 0) return fail(MOE_EINVAL, "%s: MOE_Q_* flags beside bits = 0 (the canvas form quantises nothing)", who);
    q->dither = flags & MOE_Q_ROUND ? 1 : flags & MOE_Q_ORDERED ? 2 : 0;
    q->unit = (flags & MOE_Q_UNIT) != 0;
    return MOE_OK;
}
static int stitch(const moe_plan& pl, int device, const float* tiles, const int64_t* tile_off, bool off_on_host, int C, void* out, int out_dtype, const int* band, hipStream_t s,
                  const OutEdge* edge = nullptr)
{
    const Plan& p = pl.p;
    HIP_TRY(hipSetDevice(device));
    StitchTables* d = nullptr;
    int rc = stitch_tables(pl, device, C, &d);
    if (rc) return rc;
    const long long* toff = tile_off ? (const long long*)tile_off : d->tile_off;
    if (tile_off && off_on_host) {
        const size_t nt = p.tiles.size();
        toff = nullptr;
        for (auto& c : pl.dev.uploaded)
            if (c.device == device && std::equal(c.host.begin(), c.host.end(), tile_off)) { toff = (const long long*)c.dev; break; }
        if (!toff) {
            void* up = nullptr;
            rc = PlanDevice::make_room(pl.dev.uploaded, s);
            if (!rc) rc = upload(tile_off, nt * 8, &up);
            if (rc) return rc;
            pl.dev.uploaded.push_back(UploadedOffsets{device, std::vector<int64_t>(tile_off, tile_off + nt), up});
            toff = (const long long*)up;
        }
    }
    StitchArgs a{};
    a.tiles = tiles; a.tile_off = toff;
    a.row_first = d->row_first; a.row_cnt = d->row_cnt; a.col_first = d->col_first; a.col_cnt = d->col_cnt;
    a.row_tab = d->row_tab; a.col_tab = d->col_tab; a.ramp = d->ramp;
    a.out = out; a.out_dtype = out_dtype; a.C = C; a.out_h = p.out_h; a.out_w = p.out_w; a.step_w = p.aw.step;
    a.y0 = 0; a.rows = p.out_h; a.row_lo = 0;
    if (band) {
        const int row0 = band[0], row1 = band[1], nrow = p.ah.step;
        a.row_lo = row0;
        a.y0 = p.row_tab[row0 * 4 + 1];                                  // S(row0): first un-blended row of the band's first tile row (0 for row 0)
        a.rows = (row1 < nrow ? p.row_tab[row1 * 4 + 1] : p.out_h) - a.y0;
        if (band[2] && row1 < nrow) {
            // the band ends with the blend band of tile row row1, rows [first, solid): its tiles are present as STRIPS of exactly those pad_sc rows (C planes of
            // pad_sc x width each): a row table in which that tile row starts at `first` and is pad_sc high addresses them
            int* tab = nullptr;
            for (auto& e : d->strip_tabs) if (e.first == row1) tab = e.second;
            if (!tab) {
                std::vector<int> rt(p.row_tab);
                rt[row1 * 4 + 2] = rt[row1 * 4 + 0];
                rt[row1 * 4 + 3] = rt[row1 * 4 + 1] - rt[row1 * 4 + 0];
                rc = upload(rt.data(), rt.size() * 4, (void**)&tab);
                if (rc) return rc;
                d->strip_tabs.push_back({row1, tab});
            }
            a.row_tab = tab;
        }
    }
    if (edge && edge->yuv) {
        launch_stitch_yuv(a, *edge->yuv, s, edge->yuv_dither);
        return launched("stitch_yuv");
    }
    if (edge && edge->planes_depth) {
        launch_stitch_planes(a, edge->canvas_dtype, edge->planes_depth, s, edge->dq);
        return launched("stitch_planes");
    }
    if (edge && edge->luma) {
        if (!launch_stitch_luma(a, *edge->luma, edge->canvas_dtype, s, edge->dq)) return fail(MOE_EINVAL, "moe_stitch_luma: %d pool planes (1 or 2 are supported)", C);
        return launched("stitch_luma");
    }
    if (edge && edge->mix) {
        if (!launch_stitch_mix(a, *edge->mix, edge->canvas_dtype, s, edge->dq)) return fail(MOE_EINVAL, "moe_stitch_mix: %d planes (1 to 4 are supported)", C + (edge->mix->alpha ? 1 : 0));
        return launched("stitch_mix");
    }
    if (edge) {
        if (!launch_stitch_out(a, edge->canvas_dtype, edge->quant, s, edge->dq)) return fail(MOE_EINVAL, "moe_stitch_out: %d planes (1 to 4 are supported)", C);
        return launched("stitch_out");
    }
    launch_stitch(a, s);
    return launched("stitch");
}

// What moe_stitch_out and moe_run_plan_out check of their output edge before any device call; planes: the C the kernel is asked for.
static int out_edge_args(const char* who, int planes, int canvas_dtype, int bits, const void* dst, int dst_dtype)
{
    if (!dst) return fail(MOE_EINVAL, "%s: NULL argument", who);
    if (planes < 1 || planes > 4) return fail(MOE_EINVAL, "%s: %d planes (1 to 4 are supported)", who, planes);
    if (canvas_dtype != MOE_F32 && canvas_dtype != MOE_F16) return fail(MOE_EINVAL, "%s: canvas dtype must be MOE_F32 or MOE_F16", who);
    if (bits != 8 && bits != 16) return fail(MOE_EINVAL, "%s: %d bits (8 or 16)", who, bits);
    if (dst_dtype != MOE_U8 && dst_dtype != MOE_U16) return fail(MOE_EINVAL, "%s: dst dtype must be MOE_U8 or MOE_U16", who);
    if (dst_dtype == MOE_U8 && bits > 8) return fail(MOE_EINVAL, "%s: %d bits do not fit MOE_U8", who, bits);
    return MOE_OK;
}

// What moe_stitch_planes and moe_run_plan_planes check of their edge before any device call, and the edge itself.  planes: the C the kernel is asked for.
static int plane_edge_args(const char* who, int planes, int canvas_dtype, int depth, const void* dst, OutEdge* edge)
{
    if (!dst) return fail(MOE_EINVAL, "%s: NULL argument", who);
    if (planes < 1 || planes > 4) return fail(MOE_EINVAL, "%s: %d planes (1 to 4 are supported)", who, planes);
    if (canvas_dtype != MOE_F32 && canvas_dtype != MOE_F16) return fail(MOE_EINVAL, "%s: canvas dtype must be MOE_F32 or MOE_F16", who);
    if (!plane_depth(depth)) return fail(MOE_EINVAL, "%s: depth %d (8, 10, 12 or 16)", who, depth);
    if (depth > 8 && ((uintptr_t)dst & 1)) return fail(MOE_EINVAL, "%s: dst is not 2-byte aligned (depth %d: uint16 samples)", who, depth);
    *edge = OutEdge{canvas_dtype, (float)(1 << depth)};
    edge->planes_depth = depth;
    return MOE_OK;
}

// What moe_stitch_yuv, moe_run_plan_yuv and moe_to_yuv check of their edge before any device call, and the edge itself.  planes: the plan's C (moe_to_yuv: 3).
// The coefficient tables are moephoto_amd/pixfmt.py's, per matrix the Y, Cb and Cr rows over (R, G, B).
static int yuv_edge_args(const char* who, int planes, int dtype, int depth, int matrix, int order, const void* dst, YuvEdge* y)
{
    static const int tab[3][3][3] = {{{3483, 11718, 1183}, {-1877, -6315, 8192}, {8192, -7441, -751}},        // MOE_YUV_BT709
                                     {{4899, 9617, 1868}, {-2765, -5427, 8192}, {8192, -6860, -1332}},        // MOE_YUV_BT601
                                     {{4304, 11108, 972}, {-2288, -5904, 8192}, {8192, -7533, -659}}};        // MOE_YUV_BT2020NC
    if (!dst) return fail(MOE_EINVAL, "%s: NULL argument", who);
    if (planes != 3) return fail(MOE_EINVAL, "%s: the plan has %d planes (C must be 3)", who, planes);
    if (dtype != MOE_F32 && dtype != MOE_F16) return fail(MOE_EINVAL, "%s: canvas dtype must be MOE_F32 or MOE_F16", who);
    if (depth != 8 && depth != 10 && depth != 12 && depth != 16) return fail(MOE_EINVAL, "%s: depth %d (8, 10, 12 or 16)", who, depth);
    if (matrix < MOE_YUV_BT709 || matrix > MOE_YUV_BT2020NC) return fail(MOE_EINVAL, "%s: unknown matrix %d", who, matrix);
    if (order != MOE_ORDER_BGR && order != MOE_ORDER_RGB) return fail(MOE_EINVAL, "%s: unknown order %d", who, order);
    for (int p = 0; p < 3; ++p) {
        const int colour = order == MOE_ORDER_BGR ? 2 - p : p;
        y->ky[p] = tab[matrix][0][colour]; y->ku[p] = tab[matrix][1][colour]; y->kv[p] = tab[matrix][2][colour];
    }
    y->mul_y = 219u << (depth - 6); y->base_y = 16u << (depth - 8);
    y->mul_c = 224 << (depth - 8); y->base_c = 128 << (depth - 8);
    y->depth = depth; y->f16 = dtype == MOE_F16;
    return MOE_OK;
}

// What moe_stitch_mix and moe_run_plan_filter check of their edge before any device call, and the edge itself.  planes: the net's; inp: the image the blend reads.
static int mix_edge_args(const char* who, const Plan& p, int planes, const void* inp, int inp_dtype, int64_t sC, int64_t sH, int64_t sW, const void* alpha, int64_t aH, int64_t aW,
                         double strength, int bits, const void* dst, int dst_dtype, StitchMix* m)
{
    if (!inp || !dst) return fail(MOE_EINVAL, "%s: NULL argument", who);
    if (p.sc != 1) return fail(MOE_EINVAL, "%s: plan scale %d (the blend with the input needs a plan of scale 1)", who, p.sc);
    if (bits != 0 && bits != 8 && bits != 16) return fail(MOE_EINVAL, "%s: %d bits (0 = the canvas, 8 or 16)", who, bits);
    if (inp_dtype != MOE_F32 && inp_dtype != MOE_F16) return fail(MOE_EINVAL, "%s: canvas dtype (the input's) must be MOE_F32 or MOE_F16", who);
    if (bits == 0 && dst_dtype != inp_dtype) return fail(MOE_EINVAL, "%s: dst dtype must be the input's for the canvas form (bits = 0)", who);
    if (bits != 0 && dst_dtype != MOE_U8 && dst_dtype != MOE_U16) return fail(MOE_EINVAL, "%s: dst dtype must be MOE_U8 or MOE_U16 for %d bits", who, bits);
    if (bits > 8 && dst_dtype == MOE_U8) return fail(MOE_EINVAL, "%s: %d bits do not fit MOE_U8", who, bits);
    if (planes < 1 || planes + (alpha ? 1 : 0) > 4) return fail(MOE_EINVAL, "%s: %d planes%s (1 to 4 in all are supported)", who, planes, alpha ? " + alpha" : "");
    if (!std::isfinite(strength)) return fail(MOE_EINVAL, "%s: strength must be finite", who);
    // strengthOp (python/imageProcess.py:562): x itself for s == 1, else s * x + (1 - s) * inp with the two Python floats handed to the device as fp32
    *m = StitchMix{inp, sC, sH, sW, alpha, aH, aW, (float)strength, (float)(1.0 - strength), strength != 1.0, bits ? (float)(1 << bits) : 0.f, 0, 0, 0, 0};
    return MOE_OK;
}

// The constants of a luma-only step (moephoto_amd/luma.py: lumaCoefficients): each computed in double, in the definition's order, and rounded once to fp32.
static LumaCoef luma_coef(int matrix)
{
    static const double K[3][2] = {{0.2126, 0.0722}, {0.299, 0.114}, {0.2627, 0.0593}};      // (Kr, Kb) of MOE_YUV_BT709, MOE_YUV_BT601, MOE_YUV_BT2020NC (pixfmt.LUMA)
    const double kr = K[matrix][0], kb = K[matrix][1], kg = 1 - kr - kb;
    const double eb = 2 * (1 - kb), er = 2 * (1 - kr);
    return LumaCoef{(float)kr, (float)kg, (float)kb, (float)(1 / eb), (float)(1 / er), (float)eb, (float)er, (float)(kr * er / kg), (float)(kb * eb / kg)};
}

// What moe_luma_merge, moe_stitch_luma and moe_run_plan_luma check of their edge before any device call, and the edge itself.  planes: the colour planes written
// (3, or 4 with alpha); T = dtype: the canvas dtype.  bits: 0 = the canvas, 8 or 16 = the samples.
static int luma_edge_args(const char* who, int planes, int dtype, const void* c, int matrix, int order, int bits, const void* dst, int dst_dtype, StitchLuma* m)
{
    if (!c || !dst) return fail(MOE_EINVAL, "%s: NULL argument", who);
    if (planes != 3 && planes != 4) return fail(MOE_EINVAL, "%s: %d colour planes (3, or 4 with alpha)", who, planes);
    if (dtype != MOE_F32 && dtype != MOE_F16) return fail(MOE_EINVAL, "%s: canvas dtype must be MOE_F32 or MOE_F16", who);
    if (matrix < MOE_YUV_BT709 || matrix > MOE_YUV_BT2020NC) return fail(MOE_EINVAL, "%s: unknown matrix %d", who, matrix);
    if (order != MOE_ORDER_BGR && order != MOE_ORDER_RGB) return fail(MOE_EINVAL, "%s: unknown order %d", who, order);
    if (bits != 0 && bits != 8 && bits != 16) return fail(MOE_EINVAL, "%s: %d bits (0 = the canvas, 8 or 16)", who, bits);
    if (bits == 0 && dst_dtype != dtype) return fail(MOE_EINVAL, "%s: dst dtype must be the canvas dtype for the canvas form (bits = 0)", who);
    if (bits != 0 && dst_dtype != MOE_U8 && dst_dtype != MOE_U16) return fail(MOE_EINVAL, "%s: dst dtype must be MOE_U8 or MOE_U16 for %d bits", who, bits);
    if (bits > 8 && dst_dtype == MOE_U8) return fail(MOE_EINVAL, "%s: %d bits do not fit MOE_U8", who, bits);
    if ((uintptr_t)c & 3) return fail(MOE_EINVAL, "%s: c is not 4-byte aligned (fp32 planes)", who);
    const uintptr_t es = dst_dtype == MOE_F32 ? 4 : dst_dtype == MOE_U8 ? 1 : 2;
    if ((uintptr_t)dst & (es - 1)) return fail(MOE_EINVAL, "%s: dst is not aligned to its %d-byte elements", who, (int)es);
    *m = StitchLuma{(const float*)c, luma_coef(matrix), order == MOE_ORDER_RGB ? 0 : 2, bits ? (float)(1 << bits) : 0.f};
    return MOE_OK;
}

// moe_run_plan_ex, and moe_run_plan_out / moe_run_plan_filter = the same with the final fold writing the quantised image / the DN step's result (edge)
static int run_plan(const char* who, moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                    void* out, int out_dtype, int max_tiles, float* pool, int shard_index, int shard_count, int do_stitch, void* stream, const OutEdge* edge)
{
    if (!n || !pl || !img || (do_stitch && !out)) return fail(MOE_EINVAL, "%s: NULL argument", who);
    if (!n->finalized) return fail(MOE_ESTATE, "%s: net is not finalized", who);
    const Plan& p = pl->p;
    if (p.sc != n->scale) return fail(MOE_EINVAL, "%s: plan scale %d != net scale %d", who, p.sc, n->scale);
    if (shard_count < 1) { shard_count = 1; shard_index = 0; }
    if (shard_index < 0 || shard_index >= shard_count) return fail(MOE_EINVAL, "%s: shard %d of %d", who, shard_index, shard_count);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(n->device));
    std::vector<int64_t> at(p.tile_off.begin(), p.tile_off.end());      // this shard's tiles into the plan's own pool layout
    for (size_t k = 0; k < at.size(); ++k) if ((int)(k % shard_count) != shard_index) at[k] = -1;
    const TileTable* d = nullptr;
    int rc = tile_table(*pl, n->device, 0, sC, sH, sW, 1, at.data(), s, &d);
    if (rc) return rc;
    if (!pool) {
        rc = pl->dev.pool.grow(p.pool_elems_per_plane_set * 4, s, "tile pool of %zu bytes does not fit", p.pool_elems_per_plane_set * 4);
        if (rc) return rc;
        pool = (float*)pl->dev.pool.p;
    }
    rc = run_sets(*n, p, *d, img, img_dtype, sH, sW, pool, max_tiles, s);
    if (rc || !do_stitch) return rc;
    return stitch(*pl, n->device, pool, nullptr, false, p.C, out, out_dtype, nullptr, s, edge);
}

// The next slot of the plan's table ring on `device` (TableRing above), free to be written: created on first use, then only waited for when the caller is a whole ring
// ahead of the device.
static int ring_slot(const moe_plan& pl, int device, TableRing** ring, int* slot)
{
    TableRing* r = nullptr;
    for (TableRing& c : pl.dev.rings) if (c.device == device) r = &c;
    if (!r) {
        TableRing t;
        t.device = device;
        t.slot_bytes = (std::max<size_t>(1, pl.p.tiles.size() * (size_t)pl.p.C) * 16 + 255) & ~(size_t)255;      // x and y offsets of every plane of every tile
        HIP_TRY(hipMalloc((void**)&t.dev, t.slot_bytes * TableRing::kSlots));
        hipError_t e = hipHostMalloc((void**)&t.host, t.slot_bytes * TableRing::kSlots, hipHostMallocDefault);
        for (int i = 0; i < TableRing::kSlots && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&t.done[i], hipEventDisableTiming);
        if (e != hipSuccess) {
            for (hipEvent_t ev : t.done) if (ev) (void)hipEventDestroy(ev);
            if (t.host) (void)hipHostFree(t.host);
            (void)hipFree(t.dev);
        }
        HIP_TRY(e);
        pl.dev.rings.push_back(t);
        r = &pl.dev.rings.back();
    }
    const int i = r->next;
    if (r->used[i]) {
        const hipError_t e = hipEventQuery(r->done[i]);
        if (e == hipErrorNotReady) HIP_TRY(hipEventSynchronize(r->done[i]));
        else HIP_TRY(e);
    }
    r->next = (i + 1) % TableRing::kSlots;
    *ring = r; *slot = i;
    return MOE_OK;
}

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
    delete p;      // (~PlanDevice frees the device state)
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
    return launched("wire kernel");
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
    return stitch(*p, device, tiles_dev, tile_off, true, C, out, out_dtype, nullptr, (hipStream_t)stream);
}

int moe_stitch_dev(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, void* out, int out_dtype, void* stream)
{
    if (!p || !tiles_dev || !tile_off_dev || !out || C < 1) return fail(MOE_EINVAL, "moe_stitch_dev: bad argument");
    return stitch(*p, device, tiles_dev, tile_off_dev, false, C, out, out_dtype, nullptr, (hipStream_t)stream);
}

int moe_stitch_band(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, void* out, int out_dtype,
                    int row0, int row1, int strip, void* stream)
{
    if (!p || !tiles_dev || !tile_off_dev || !out || C < 1) return fail(MOE_EINVAL, "moe_stitch_band: bad argument");
    const int nrow = p->p.ah.step;
    if (row0 < 0 || row1 <= row0 || row1 > nrow) return fail(MOE_EINVAL, "moe_stitch_band: tile rows [%d, %d) of %d", row0, row1, nrow);
    const int band[3] = {row0, row1, strip};
    return stitch(*p, device, tiles_dev, tile_off_dev, false, C, out, out_dtype, band, (hipStream_t)stream);
}

int moe_stitch_out(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, int canvas_dtype, int bits, void* dst, int dst_dtype, void* stream)
{
    if (!p || !tiles_dev || C < 1) return fail(MOE_EINVAL, "moe_stitch_out: bad argument");
    QuantReq q;
    if (int rc = quant_flags("moe_stitch_out", bits, true, &q)) return rc;
    bits = q.low;
    const int rc = out_edge_args("moe_stitch_out", C, canvas_dtype, bits, dst, dst_dtype);
    if (rc) return rc;
    q.fill();
    OutEdge edge{canvas_dtype, (float)(1 << bits)};
    edge.dq = q.dq();
    return stitch(*p, device, tiles_dev, tile_off_dev, false, C, dst, dst_dtype, nullptr, (hipStream_t)stream, &edge);
}

int moe_stitch_planes(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, int canvas_dtype, int depth, void* dst, void* stream)
{
    if (!p || !tiles_dev) return fail(MOE_EINVAL, "moe_stitch_planes: NULL argument");
    OutEdge edge{};
    QuantReq q;
    if (int rc = quant_flags("moe_stitch_planes", depth, true, &q)) return rc;
    depth = q.low;
    const int rc = plane_edge_args("moe_stitch_planes", C, canvas_dtype, depth, dst, &edge);
    if (rc) return rc;
    q.fill();
    edge.dq = q.dq();
    return stitch(*p, device, tiles_dev, tile_off_dev, false, C, dst, depth == 8 ? MOE_U8 : MOE_U16, nullptr, (hipStream_t)stream, &edge);
}

int moe_stitch_mix(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int C, const void* inp, int inp_dtype, int64_t sC, int64_t sH, int64_t sW,
                   const void* alpha, int64_t aH, int64_t aW, double strength, int bits, void* dst, int dst_dtype, void* stream)
{
    if (!p || !tiles_dev) return fail(MOE_EINVAL, "moe_stitch_mix: NULL argument");
    StitchMix m{};
    QuantReq q;
    if (int rc = quant_flags("moe_stitch_mix", bits, true, &q)) return rc;
    bits = q.low;
    const int rc = mix_edge_args("moe_stitch_mix", p->p, C, inp, inp_dtype, sC, sH, sW, alpha, aH, aW, strength, bits, dst, dst_dtype, &m);
    if (rc) return rc;
    q.fill();
    OutEdge edge{inp_dtype, m.quant, &m};
    edge.dq = q.dq();
    return stitch(*p, device, tiles_dev, tile_off_dev, false, C, dst, dst_dtype, nullptr, (hipStream_t)stream, &edge);
}

int moe_stitch_yuv(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int canvas_dtype, int depth, int matrix, int order, void* dst, void* stream)
{
    if (!p || !tiles_dev) return fail(MOE_EINVAL, "moe_stitch_yuv: NULL argument");
    YuvEdge y{};
    QuantReq q;
    if (int rc = quant_flags("moe_stitch_yuv", depth, false, &q)) return rc;
    depth = q.low;
    const int rc = yuv_edge_args("moe_stitch_yuv", p->p.C, canvas_dtype, depth, matrix, order, dst, &y);
    if (rc) return rc;
    OutEdge edge{canvas_dtype, 0.f};
    edge.yuv = &y;
    edge.yuv_dither = q.dither;
    return stitch(*p, device, tiles_dev, tile_off_dev, false, 3, dst, depth == 8 ? MOE_U8 : MOE_U16, nullptr, (hipStream_t)stream, &edge);
}

int moe_stitch_luma(const moe_plan* p, int device, const float* tiles_dev, const int64_t* tile_off_dev, int P, int canvas_dtype, const void* c, int matrix, int order,
                    int bits, void* dst, int dst_dtype, void* stream)
{
    if (!p || !tiles_dev) return fail(MOE_EINVAL, "moe_stitch_luma: NULL argument");
    if (P != 1 && P != 2) return fail(MOE_EINVAL, "moe_stitch_luma: %d pool planes (1: Y', or 2: Y' and alpha)", P);
    StitchLuma m{};
    QuantReq q;
    if (int rc = quant_flags("moe_stitch_luma", bits, true, &q)) return rc;
    bits = q.low;
    const int rc = luma_edge_args("moe_stitch_luma", P + 2, canvas_dtype, c, matrix, order, bits, dst, dst_dtype, &m);
    if (rc) return rc;
    q.fill();
    if ((uintptr_t)tiles_dev & 3) return fail(MOE_EINVAL, "moe_stitch_luma: tiles_dev is not 4-byte aligned (fp32 pool)");
    OutEdge edge{canvas_dtype, m.quant};
    edge.luma = &m;
    edge.dq = q.dq();
    return stitch(*p, device, tiles_dev, tile_off_dev, false, P, dst, dst_dtype, nullptr, (hipStream_t)stream, &edge);
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
    return launched("blend");
}

int moe_run_plan_ex(moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                    void* out, int out_dtype, int max_tiles, float* pool, int shard_index, int shard_count, int do_stitch, void* stream)
{
    return run_plan("moe_run_plan", n, pl, img, img_dtype, sC, sH, sW, out, out_dtype, max_tiles, pool, shard_index, shard_count, do_stitch, stream, nullptr);
}

int moe_run_plan_out(moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                     int canvas_dtype, int bits, void* dst, int dst_dtype, int max_tiles, void* stream)
{
    if (!n || !pl || !img) return fail(MOE_EINVAL, "moe_run_plan_out: NULL argument");
    QuantReq q;
    if (int rc = quant_flags("moe_run_plan_out", bits, true, &q)) return rc;
    bits = q.low;
    const int rc = out_edge_args("moe_run_plan_out", pl->p.C, canvas_dtype, bits, dst, dst_dtype);
    if (rc) return rc;
    q.fill();
    OutEdge edge{canvas_dtype, (float)(1 << bits)};
    edge.dq = q.dq();
    return run_plan("moe_run_plan_out", n, pl, img, img_dtype, sC, sH, sW, dst, dst_dtype, max_tiles, nullptr, 0, 1, 1, stream, &edge);
}

int moe_run_plan_planes(moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                        int canvas_dtype, int depth, void* dst, int max_tiles, void* stream)
{
    if (!n || !pl || !img) return fail(MOE_EINVAL, "moe_run_plan_planes: NULL argument");
    OutEdge edge{};
    QuantReq q;
    if (int rc = quant_flags("moe_run_plan_planes", depth, true, &q)) return rc;
    depth = q.low;
    const int rc = plane_edge_args("moe_run_plan_planes", pl->p.C, canvas_dtype, depth, dst, &edge);
    if (rc) return rc;
    q.fill();
    edge.dq = q.dq();
    return run_plan("moe_run_plan_planes", n, pl, img, img_dtype, sC, sH, sW, dst, depth == 8 ? MOE_U8 : MOE_U16, max_tiles, nullptr, 0, 1, 1, stream, &edge);
}

int moe_run_plan_yuv(moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW,
                     int canvas_dtype, int depth, int matrix, int order, void* dst, int max_tiles, void* stream)
{
    if (!n || !pl || !img) return fail(MOE_EINVAL, "moe_run_plan_yuv: NULL argument");
    YuvEdge y{};
    QuantReq q;
    if (int rc = quant_flags("moe_run_plan_yuv", depth, false, &q)) return rc;
    depth = q.low;
    const int rc = yuv_edge_args("moe_run_plan_yuv", pl->p.C, canvas_dtype, depth, matrix, order, dst, &y);
    if (rc) return rc;
    OutEdge edge{canvas_dtype, 0.f};
    edge.yuv = &y;
    edge.yuv_dither = q.dither;
    return run_plan("moe_run_plan_yuv", n, pl, img, img_dtype, sC, sH, sW, dst, depth == 8 ? MOE_U8 : MOE_U16, max_tiles, nullptr, 0, 1, 1, stream, &edge);
}

int moe_run_plan_filter(moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW, const void* alpha, int64_t aH, int64_t aW,
                        double strength, int bits, void* dst, int dst_dtype, int max_tiles, void* stream)
{
    if (!n || !pl || !img) return fail(MOE_EINVAL, "moe_run_plan_filter: NULL argument");
    StitchMix m{};
    QuantReq q;
    if (int rc = quant_flags("moe_run_plan_filter", bits, true, &q)) return rc;
    bits = q.low;
    const int rc = mix_edge_args("moe_run_plan_filter", pl->p, pl->p.C, img, img_dtype, sC, sH, sW, alpha, aH, aW, strength, bits, dst, dst_dtype, &m);
    if (rc) return rc;
    q.fill();
    OutEdge edge{img_dtype, m.quant, &m};
    edge.dq = q.dq();
    return run_plan("moe_run_plan_filter", n, pl, img, img_dtype, sC, sH, sW, dst, dst_dtype, max_tiles, nullptr, 0, 1, 1, stream, &edge);
}

int moe_run_plan_luma(moe_net* n, const moe_plan* pl, const void* img_y, int dtype, int64_t sC, int64_t sH, int64_t sW, const void* c, int matrix, int order,
                      int bits, void* dst, int dst_dtype, int max_tiles, void* stream)
{
    if (!n || !pl || !img_y) return fail(MOE_EINVAL, "moe_run_plan_luma: NULL argument");
    if (pl->p.C != 1 && pl->p.C != 2) return fail(MOE_EINVAL, "moe_run_plan_luma: the plan has %d planes (1: Y', or 2: Y' and alpha)", pl->p.C);
    StitchLuma m{};
    QuantReq q;
    if (int rc = quant_flags("moe_run_plan_luma", bits, true, &q)) return rc;
    bits = q.low;
    const int rc = luma_edge_args("moe_run_plan_luma", pl->p.C + 2, dtype, c, matrix, order, bits, dst, dst_dtype, &m);
    if (rc) return rc;
    q.fill();
    if ((uintptr_t)img_y & (dtype == MOE_F16 ? 1 : 3)) return fail(MOE_EINVAL, "moe_run_plan_luma: img_y is not aligned to its %d-byte elements", dtype == MOE_F16 ? 2 : 4);
    OutEdge edge{dtype, m.quant};
    edge.luma = &m;
    edge.dq = q.dq();
    return run_plan("moe_run_plan_luma", n, pl, img_y, dtype, sC, sH, sW, dst, dst_dtype, max_tiles, nullptr, 0, 1, 1, stream, &edge);
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
    const TileTable* d = nullptr;
    int rc = tile_table(*pl, n->device, frame_stride, sC, sH, sW, n_frames, tile_dst, s, &d);
    if (rc) return rc;
    return run_sets(*n, p, *d, imgs, img_dtype, sH, sW, dst, max_tiles, s);
}

int moe_run_plan_subset(moe_net* n, const moe_plan* pl, const void* img, int img_dtype, int64_t sC, int64_t sH, int64_t sW, const uint8_t* run,
                        float* pool, int max_tiles, void* stream)
{
    if (!n || !pl || !img || !run || !pool) return fail(MOE_EINVAL, "moe_run_plan_subset: NULL argument");
    if (!n->finalized) return fail(MOE_ESTATE, "moe_run_plan_subset: net is not finalized");
    const Plan& p = pl->p;
    if (p.sc != n->scale) return fail(MOE_EINVAL, "moe_run_plan_subset: plan scale %d != net scale %d", p.sc, n->scale);
    std::vector<int64_t> at(p.tile_off.begin(), p.tile_off.end());      // the masked tiles into the plan's own pool layout
    bool any = false;
    for (size_t k = 0; k < at.size(); ++k) {
        if (run[k]) any = true;
        else at[k] = -1;
    }
    if (!any) return MOE_OK;                                            // (nothing to compute: no device call)
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(n->device));
    TileTable d;
    std::vector<long long> off, yo;
    table_rows(p, 0, sC, sH, sW, 1, at.data(), d, off, yo);
    TableRing* ring = nullptr;
    int slot = 0;
    int rc = ring_slot(*pl, n->device, &ring, &slot);
    if (rc) return rc;
    const size_t rows = off.size(), at_slot = ring->slot_bytes * (size_t)slot;
    memcpy(ring->host + at_slot, off.data(), rows * 8);
    memcpy(ring->host + at_slot + rows * 8, yo.data(), rows * 8);
    HIP_TRY(hipMemcpyAsync(ring->dev + at_slot, ring->host + at_slot, rows * 16, hipMemcpyHostToDevice, s));
    ring->used[slot] = true;                                            // (from here on the slot's halves are in use until its event has passed)
    d.x_off = (const long long*)(ring->dev + at_slot); d.y_off = d.x_off + rows;
    rc = run_sets(*n, p, d, img, img_dtype, sH, sW, pool, max_tiles, s);
    const hipError_t e = hipEventRecord(ring->done[slot], s);
    if (rc) return rc;
    HIP_TRY(e);
    return MOE_OK;
}

int moe_changed_blocks(const void* cur, void* prev, int n, int rows, int64_t row_bytes, int block_rows, int block_bytes, uint8_t* map, int device, void* stream)
{
    if (!cur || !prev || !map) return fail(MOE_EINVAL, "moe_changed_blocks: NULL argument");
    if (n < 1 || rows < 1 || row_bytes < 1) return fail(MOE_EINVAL, "moe_changed_blocks: %d matrices of %d rows x %lld bytes (each must be 1 at least)", n, rows, (long long)row_bytes);
    if (block_rows < 1 || block_bytes < 1) return fail(MOE_EINVAL, "moe_changed_blocks: blocks of %d rows x %d bytes (each must be 1 at least)", block_rows, block_bytes);
    if (cur == prev) return fail(MOE_EINVAL, "moe_changed_blocks: cur and prev are the same buffer");
    if (row_bytes > INT64_MAX / n / rows) return fail(MOE_EINVAL, "moe_changed_blocks: %d matrices of %d rows x %lld bytes do not fit 63 bits", n, rows, (long long)row_bytes);
    const uint64_t bytes = (uint64_t)n * (uint64_t)rows * (uint64_t)row_bytes, a = (uint64_t)(uintptr_t)cur, b = (uint64_t)(uintptr_t)prev;
    if ((a < b ? b - a : a - b) < bytes) return fail(MOE_EINVAL, "moe_changed_blocks: cur and prev overlap (%llu bytes each)", (unsigned long long)bytes);
    const int64_t nrow = ((int64_t)rows - 1) / block_rows + 1, ncol = (row_bytes - 1) / block_bytes + 1;
    const int64_t cells = ncol > INT32_MAX / nrow ? (int64_t)INT32_MAX + 1 : nrow * ncol;
    if (cells > INT32_MAX) return fail(MOE_EINVAL, "moe_changed_blocks: a map of %lld cells (2^31 - 1 at most)", (long long)cells);
    HIP_TRY(hipSetDevice(device));
    launch_changed_blocks(cur, prev, n, rows, row_bytes, block_rows, block_bytes, map, (hipStream_t)stream);
    return launched("changed_blocks");
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

// dst (C, Hp, Wp) = padImage(trans_s(src)); src = (C, H, W) with element strides
static int sym_pad(const void* src, bool f16, int C, int H, int W, int64_t sC, int64_t sH, int64_t sW, int s, void* dst, int Hp, int Wp, hipStream_t st)
{
    const Sym y = sym_of(s);
    SymArgs a{};
    a.src = src; a.dst = dst; a.sC = sC; a.sH = sH; a.sW = sW; a.C = C; a.Hd = Hp; a.Wd = Wp;
    a.nR = y.t ? W : H; a.nC = y.t ? H : W; a.flipR = y.fv; a.flipC = y.fh;
    launch_sym(a, f16, false, y.t != 0, st);
    return launched("moe_sym_pad");
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
    return launched("moe_sym_fold");
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
    const char* fits = "moe_run_plan_ens: %s of %zu bytes does not fit";
    int rc = n->ens_pad.grow(pad_need, s, fits, "the padded image", pad_need);
    if (!rc && canvas_need) rc = n->ens_canvas.grow(canvas_need, s, fits, "a symmetry's canvas", canvas_need);
    if (rc) return rc;
    // v = doCrop(x)
    rc = sym_pad(img, f16_in, p.C, p.H, p.W, sC, sH, sW, -1, n->ens_pad.p, hp, wp, s);
    if (!rc) rc = moe_run_plan(n, pl, n->ens_pad.p, img_dtype, (int64_t)hp * wp, wp, 1, out, out_dtype, max_tiles, s);
    // v = v + transInv[i](doCrop(trans[i](x))), the closing / (n + 1) inside the last fold
    for (int i = 0; i < n_sym && !rc; ++i) {
        const bool t = sym_of(i).t != 0;
        const int h = t ? hpt : hp, w = t ? wpt : wp;
        rc = sym_pad(img, f16_in, p.C, p.H, p.W, sC, sH, sW, i, n->ens_pad.p, h, w, s);
        if (!rc) rc = moe_run_plan(n, t ? pl_t : pl, n->ens_pad.p, img_dtype, (int64_t)h * w, w, 1, n->ens_canvas.p, out_dtype, max_tiles, s);
        if (!rc) rc = sym_fold(out, n->ens_canvas.p, f16_out, p.C, p.out_h, p.out_w, i, i == n_sym - 1 ? n_sym + 1 : 0, s);
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

int moe_planes_to_float(const void* src, int depth, int H, int W, void* dst_y, void* dst_c, int dst_dtype, int device, void* stream)
{
    if (!src || !dst_y || !dst_c) return fail(MOE_EINVAL, "moe_planes_to_float: NULL argument");
    if (!plane_depth(depth)) return fail(MOE_EINVAL, "moe_planes_to_float: depth %d (8, 10, 12 or 16)", depth);
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(MOE_EINVAL, "moe_planes_to_float: size %d x %d (a 4:2:0 frame has an even width and height, 2 at least)", W, H);
    if (dst_dtype != MOE_F32 && dst_dtype != MOE_F16) return fail(MOE_EINVAL, "moe_planes_to_float: dst dtype must be MOE_F32 or MOE_F16");
    if (depth > 8 && ((uintptr_t)src & 1)) return fail(MOE_EINVAL, "moe_planes_to_float: src is not 2-byte aligned (depth %d: uint16 samples)", depth);
    const uintptr_t es = dst_dtype == MOE_F16 ? 2 : 4;
    if (((uintptr_t)dst_y | (uintptr_t)dst_c) & (es - 1)) return fail(MOE_EINVAL, "moe_planes_to_float: dst_y / dst_c are not aligned to their %d-byte elements", (int)es);
    HIP_TRY(hipSetDevice(device));
    launch_to_float_planes(src, depth, H, W, dst_y, dst_c, dst_dtype, (hipStream_t)stream);
    return launched("to_float_planes");
}

int moe_luma_split(const void* img, int dtype, int C, int64_t sC, int64_t sH, int64_t sW, int H, int W, int matrix, int order, void* dst_y, void* dst_c, int device, void* stream)
{
    if (!img || !dst_y || !dst_c) return fail(MOE_EINVAL, "moe_luma_split: NULL argument");
    if (C != 3 && C != 4) return fail(MOE_EINVAL, "moe_luma_split: %d planes (3, or 4 with alpha)", C);
    if (dtype != MOE_F32 && dtype != MOE_F16) return fail(MOE_EINVAL, "moe_luma_split: dtype must be MOE_F32 or MOE_F16");
    if (H < 1 || W < 1) return fail(MOE_EINVAL, "moe_luma_split: size %d x %d must be positive", W, H);
    if (matrix < MOE_YUV_BT709 || matrix > MOE_YUV_BT2020NC) return fail(MOE_EINVAL, "moe_luma_split: unknown matrix %d", matrix);
    if (order != MOE_ORDER_BGR && order != MOE_ORDER_RGB) return fail(MOE_EINVAL, "moe_luma_split: unknown order %d", order);
    const uintptr_t es = dtype == MOE_F16 ? 2 : 4;
    if (((uintptr_t)img | (uintptr_t)dst_y) & (es - 1)) return fail(MOE_EINVAL, "moe_luma_split: img / dst_y are not aligned to their %d-byte elements", (int)es);
    if ((uintptr_t)dst_c & 3) return fail(MOE_EINVAL, "moe_luma_split: dst_c is not 4-byte aligned (fp32 planes)");
    HIP_TRY(hipSetDevice(device));
    launch_luma_split(img, dtype, C, sC, sH, sW, H, W, luma_coef(matrix), order == MOE_ORDER_RGB ? 0 : 2, dst_y, (float*)dst_c, (hipStream_t)stream);
    return launched("to_float_luma");
}

int moe_luma_merge(const void* y, int dtype, const void* c, int C, int H, int W, int matrix, int order, int bits, void* dst, int dst_dtype, int device, void* stream)
{
    if (!y) return fail(MOE_EINVAL, "moe_luma_merge: NULL argument");
    if (H < 1 || W < 1) return fail(MOE_EINVAL, "moe_luma_merge: size %d x %d must be positive", W, H);
    StitchLuma m{};
    QuantReq q;
    if (int rc = quant_flags("moe_luma_merge", bits, true, &q)) return rc;
    bits = q.low;
    const int rc = luma_edge_args("moe_luma_merge", C, dtype, c, matrix, order, bits, dst, dst_dtype, &m);
    if (rc) return rc;
    q.fill();
    if ((uintptr_t)y & (dtype == MOE_F16 ? 1 : 3)) return fail(MOE_EINVAL, "moe_luma_merge: y is not aligned to its %d-byte elements", dtype == MOE_F16 ? 2 : 4);
    HIP_TRY(hipSetDevice(device));
    launch_luma_merge(y, dtype, m.c, C, H, W, m.k, m.rp, m.quant, dst, dst_dtype, (hipStream_t)stream, q.dq());
    return launched("to_output_luma");
}

int moe_resize(const void* src, void* dst, int dtype, int C, int H, int W, int h, int w, int mode, int device, void* stream)
{
    if (!src || !dst || C < 1 || H < 1 || W < 1 || h < 1 || w < 1) return fail(MOE_EINVAL, "moe_resize: bad argument");
    if (dtype != MOE_F32 && dtype != MOE_F16) return fail(MOE_EINVAL, "moe_resize: dtype must be MOE_F32 or MOE_F16");
    if (mode < MOE_RESIZE_NEAREST || mode > MOE_RESIZE_BICUBIC) return fail(MOE_EINVAL, "moe_resize: unknown mode %d", mode);
    HIP_TRY(hipSetDevice(device));
    launch_resize(src, dst, dtype, C, H, W, h, w, mode, (hipStream_t)stream);
    return launched("resize");
}

int moe_to_output(const void* src, int src_dtype, int H, int W, int C, int bits, void* dst, int dst_dtype, int device, void* stream)
{
    QuantReq q;
    if (int rc = quant_flags("moe_to_output", bits, true, &q)) return rc;
    bits = q.low;
    if (!src || !dst || H < 1 || W < 1 || C < 1 || bits < 1 || bits > 16) return fail(MOE_EINVAL, "moe_to_output: bad argument");
    if ((dst_dtype != MOE_U8 && dst_dtype != MOE_U16) || (src_dtype != MOE_F32 && src_dtype != MOE_F16)) return fail(MOE_EINVAL, "moe_to_output: bad dtype");
    if (dst_dtype == MOE_U8 && bits > 8) return fail(MOE_EINVAL, "moe_to_output: %d bits do not fit MOE_U8", bits);
    HIP_TRY(hipSetDevice(device));
    q.fill();
    launch_to_output(src, src_dtype, H, W, C, (float)(1 << bits), dst, dst_dtype, (hipStream_t)stream, q.dq());
    return MOE_OK;
}

int moe_to_yuv(const void* src, int src_dtype, int H, int W, int depth, int matrix, int order, void* dst, int device, void* stream)
{
    if (!src) return fail(MOE_EINVAL, "moe_to_yuv: NULL argument");
    if (H < 1 || W < 1) return fail(MOE_EINVAL, "moe_to_yuv: size %d x %d must be positive", H, W);
    YuvEdge y{};
    QuantReq q;
    if (int rc = quant_flags("moe_to_yuv", depth, false, &q)) return rc;
    depth = q.low;
    const int rc = yuv_edge_args("moe_to_yuv", 3, src_dtype, depth, matrix, order, dst, &y);
    if (rc) return rc;
    y.f16 = 0;      // (the planes are the canvas: their values are converted as they are)
    HIP_TRY(hipSetDevice(device));
    launch_to_output_yuv(src, src_dtype, H, W, y, dst, (hipStream_t)stream, q.dither);
    return launched("to_output_yuv");
}

}  // extern "C"
