// capi.hip — the raster part of the C ABI declared in include/splatraster.h: buffer layouts, the per-view / window / raw
// raster pipeline (argument validation and stage sequencing), the sort and timing entry points, error strings and polling,
// and the raster debug hooks.  Every other stage defines its splatraster_* / splatknn_* entry points in an extern "C" block
// at the end of its own .hip (densify.hip, matching.hip, ...).  No torch types; everything is raw device pointers.
#include <assert.h>
#include <string.h>

#include <mutex>
#include <unordered_map>
#include <string>
#include <vector>

#include "common.h"

namespace sr {

static thread_local std::string g_last_error;
static int g_deterministic = 0;   // splatraster_debug_set_deterministic
// the knobs behind a frame's launch plan (their setters at the end of this file): frame_plan() alone reads them
static int g_split_max_waves = SPLIT_MAX_WAVES;   // quadrant-waves up to which a narrow launch is split
static int g_fwd_team = -1;         // -1: automatic (the split launches' condition), 0: never, 1: every narrow launch that has a launch order, 2: and a team for each of its first TEAM_MAX lists
static int g_payload_compact = -1;  // -1 default (on), 0 off (payload_kernel, the full stream)
static int g_dead_marks = 1;        // the backward skips the entries the forward marked dead (0: it walks them)
static int g_bin_mode = -1;         // front end: -1 auto, 0 radix always, 1 binned whenever the shape allows

void set_hip_error(hipError_t e, const char* what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
}

void set_error_text(const char* text) { g_last_error = text; }

// ---- stage timing ---------------------------------------------------------------------
struct StageRec { int stage; hipEvent_t a, b; };
static uint32_t g_timing_mask = 0;  // bit s: stage s is bracketed by an event pair
static std::mutex g_timing_mu;
static std::vector<StageRec> g_recs;
static std::vector<hipEvent_t> g_pool;

static hipEvent_t get_event()
{
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

struct StageTimer {
    hipStream_t stream;
    StageRec rec{};
    bool on;
    StageTimer(int stage, hipStream_t s) : stream(s), on((g_timing_mask >> stage) & 1u)
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(g_timing_mu);
        rec.stage = stage; rec.a = get_event(); rec.b = get_event();
        if (!rec.a || !rec.b) { on = false; return; }
        (void)hipEventRecord(rec.a, stream);
    }
    ~StageTimer()
    {
        if (!on) return;
        (void)hipEventRecord(rec.b, stream);
        std::lock_guard<std::mutex> lk(g_timing_mu);
        g_recs.push_back(rec);
    }
};

// ---- host landing slot of the early instance count ---------------------------------------
// One pinned, device-mapped buffer + one event per host thread (and device): preprocess_kernel writes its per-(view, block)
// sums straight into it (round 5: a 4-us copy operation used to sit between preprocess and the next kernel of every frame), the
// event is recorded behind preprocess, the depth sort and scan are enqueued behind it, and the host waits on the EVENT only —
// the GPU keeps working while the caller sizes and allocates the binning buffer.
struct HostSlot {
    uint32_t* p = nullptr;    // host address
    uint32_t* dp = nullptr;   // the same memory as the device addresses it
    size_t cap = 0;  // elements
    hipEvent_t ev = nullptr;
    int device = -1;
};
static thread_local HostSlot t_slot;

static int host_slot(size_t n, HostSlot** out)
{
    HostSlot& s = t_slot;
    int dev = 0;
    SR_HIP_CHECK(hipGetDevice(&dev));
    if (s.cap < n) {
        if (s.p) (void)hipHostFree(s.p);
        s.p = nullptr;
        s.dp = nullptr;
        s.cap = 0;
        const size_t cap = n < 4096 ? 4096 : n + n / 2;
        SR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&s.p), sizeof(uint32_t) * cap, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent));
        SR_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&s.dp), s.p, 0));
        s.cap = cap;
    }
    if (!s.ev || s.device != dev) {
        if (s.ev) (void)hipEventDestroy(s.ev);
        s.ev = nullptr;
        SR_HIP_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
        s.device = dev;
    }
    *out = &s;
    return SPLATRASTER_OK;
}

#ifndef SR_TILE_KEYS16
#define SR_TILE_KEYS16 1   // 0: 32-bit keys through the tile sort whatever their width (A/B baseline)
#endif
static inline int tile_bits(int tiles)
{
    int b = 1;
    while ((1 << b) < tiles) ++b;
    return b;
}

// tiles per row / column of a view: the buffer layouts below take W, H before any plan exists
struct TileGrid { int gx, gy; };
static inline TileGrid tile_grid(int32_t W, int32_t H) { return TileGrid{(W + TILE - 1) / TILE, (H + TILE - 1) / TILE}; }

// Both walks below note the offsets splatraster_get_*_layout publishes (and the two the binned front end's room check needs) on
// their way past: `c.o` in front of a take is where that section starts.
struct GeomLayout {
    GeomView v;
    uint32_t *keys_alt, *vals_alt;   // the depth sort's ping-pong twins
    void* scan_tmp;
    size_t rec0, tiles_touched, depth_order, offsets, rgb, clamped, sort_keys, total, bytes;
};
// n = V * P rows (V views of a window; V = 1 for the plain call)
static GeomLayout geom_layout(void* base, int32_t P, int32_t V)
{
    const size_t p1 = (size_t)(P > 0 ? P : 1), nv = (size_t)(V > 0 ? V : 1);
    const size_t n = p1 * nv;
    GeomLayout L;
    Carver c{base};
    L.rec0 = c.o;           L.v.rec = c.take<float4>(2 * n);
    L.tiles_touched = c.o;  L.v.tiles_touched = c.take<uint32_t>(n);
    L.depth_order = c.o;    L.v.depth_order = c.take<uint32_t>(n);
    L.offsets = c.o;        L.v.offsets = c.take<uint32_t>(n);
    L.rgb = c.o;            L.v.rgb = c.take<float>(3 * p1);       // SH colours: single-view calls only
    L.clamped = c.o;        L.v.clamped = c.take<uint8_t>(3 * p1);
    L.sort_keys = c.o;      L.v.sort_keys = c.take<uint32_t>(n);
    L.keys_alt = c.take<uint32_t>(n);
    L.vals_alt = c.take<uint32_t>(n);
    L.v.sort_tmp = reinterpret_cast<uint32_t*>(c.take<char>(sort_tmp_bytes((int64_t)n)));
    L.scan_tmp = c.take<char>(scan_tmp_bytes((int64_t)n));
    L.total = c.o;          L.v.total = c.take<uint32_t>(4);
    L.v.block_tiles = c.take<uint32_t>((size_t)preprocess_blocks((int32_t)p1) * nv);
    L.v.span_owner = c.take<uint32_t>((size_t)SPAN_OWNER_CAP);
    L.bytes = c.o;
    return L;
}
GeomView geom_view(void* base, int32_t P, int32_t V) { return geom_layout(base, P, V).v; }

struct BinLayout { BinView v; size_t point_list, tile_list, ranges, bytes; };
static BinLayout bin_layout(void* base, int32_t P, int32_t V, int64_t R, int32_t W, int32_t H, int32_t C)
{
    const size_t n = (size_t)(R > 0 ? R : 1), p1 = (size_t)(P > 0 ? P : 1), nv = (size_t)(V > 0 ? V : 1);
    const TileGrid tg = tile_grid(W, H);
    const size_t tiles = (size_t)tg.gx * (size_t)tg.gy * nv, tiles1 = tiles > 0 ? tiles : 1;
    BinLayout L;
    Carver c{base};
    L.point_list = c.o;  L.v.point_list = c.take<uint32_t>(n);
    L.tile_list = c.o;   L.v.tile_list = c.take<uint32_t>(n);
    L.v.keys_tmp = c.take<uint32_t>(n);
    L.v.vals_tmp = c.take<uint32_t>(n);
    L.ranges = c.o;      L.v.ranges = c.take<uint32_t>(2 * tiles1);
    L.v.sort_tmp = c.take<char>(sort_tmp_bytes((int64_t)n));
    L.v.irec = c.take<float4>(2 * n);
    L.v.ipack = c.take<uint32_t>(n);
    // padded feature table only when the rows are not already 16-byte aligned (shared by the views)
    L.v.featp = c.take<float>((C % 4) ? p1 * padded_channels(C) : 4);
    // (the shared colour rows and the per-(view, Gaussian) rows are ONE section: GaccLayout, common.h)
    L.v.gacc = c.take<float>(gacc_total_floats(C, p1, nv));
    L.v.pose_acc = c.take<float>(POSE_ACC_FLOATS);      // (directly behind gacc: the backward zeroes both with one fill)
    // (the deterministic debug mode's 64-bit accumulator is NOT part of this buffer: it is a stream-ordered
    //  allocation made by the backward only while that mode is on)
    // mid-list checkpoints of the forward for split launches (small frames, narrow layouts): the maximum is reserved
    // whenever the shape qualifies, whatever the run-time knob says
    const bool ck = C <= 4 && 4 * (size_t)tiles <= (size_t)SPLIT_MAX_WAVES;
    L.v.ckpt = c.take<float>(ck ? nv * (size_t)SPLIT_PARTS_MAX * (size_t)(C + 2) * (size_t)W * (size_t)H : 4);
    L.v.tile_order = c.take<uint32_t>(tiles1);
    L.v.nparts = c.take<uint32_t>(tiles1);
    L.bytes = c.o;
    return L;
}
BinView bin_view(void* base, int32_t P, int32_t V, int64_t R, int32_t W, int32_t H, int32_t C)
{
    return bin_layout(base, P, V, R, W, H, C).v;
}

// final_T, n_contrib (where they always were), then what the compact payload adds: the plane n_contrib_c and the table cranges.
// (The table belongs to the instance stream, but the binning buffer's size is pinned section by section
//  — tests/test_accumulator_layout_sizes.py — while this buffer travels with it from the forward to the backward anyway.)
struct ImgLayout { ImgView v; size_t n_contrib, bytes; };   // n_contrib: the offset splatraster_get_*_image_layout publishes
static ImgLayout img_layout(void* base, int32_t W, int32_t H, int32_t V)
{
    const size_t nv = (size_t)(V > 0 ? V : 1);
    const size_t plane = (size_t)W * H * nv;
    const TileGrid tg = tile_grid(W, H);
    ImgLayout L;
    Carver c{base};
    L.v.final_T = c.take<float>(plane);
    L.n_contrib = c.o;
    L.v.n_contrib = c.take<uint32_t>(plane);
    L.v.n_contrib_c = c.take<uint32_t>(plane);
    L.v.cranges = c.take<uint32_t>(2 * (size_t)tg.gx * (size_t)tg.gy * nv);
    L.bytes = c.o;
    return L;
}
ImgView img_view(void* base, int32_t W, int32_t H, int32_t V) { return img_layout(base, W, H, V).v; }

// The compositing kernels index feature / accumulator rows with 24-bit x 24-bit multiplies (one
// full-rate instruction instead of a 64-bit multiply-add pair per address): Gaussian ids must fit 24
// bits and a row's float offset 32 bits.  16.7 M Gaussians per scene — SplatLoc maps hold < 1 M.
// The accumulator's two tables (GaccLayout, common.h) are addressed as mul24(row, stride) + base + column modulo 2^32: right
// whenever the element's index itself — at most the accumulator's size — fits 32 bits.
static int check_row_index_range(int32_t P, int32_t V, int32_t C)
{
    const uint64_t n = (uint64_t)P * (uint64_t)V;   // rows of the window
    if (n > (1ull << 24) || n * (uint64_t)padded_channels(C) >= (1ull << 32)) return SPLATRASTER_ERR_UNSUPPORTED;
    if ((uint64_t)gacc_total_floats(C, (size_t)P, (size_t)V) >= (1ull << 32)) return SPLATRASTER_ERR_UNSUPPORTED;
    return SPLATRASTER_OK;
}

static int check_settings(const splatraster_settings* s)
{
    if (!s) return SPLATRASTER_ERR_BAD_ARG;
    if (s->image_width <= 0 || s->image_height <= 0 || s->channels <= 0) return SPLATRASTER_ERR_BAD_ARG;
    if (s->bg_channels < 0) return SPLATRASTER_ERR_BAD_ARG;
    return SPLATRASTER_OK;
}

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_abi_version(void) { return SPLATRASTER_ABI_VERSION; }

const char* splatraster_error_string(int status)
{
    switch (status) {
        case SPLATRASTER_OK: return "ok";
        case SPLATRASTER_ERR_BAD_ARG: return "bad argument";
        case SPLATRASTER_ERR_HIP: return "HIP runtime error";
        case SPLATRASTER_ERR_UNSUPPORTED: return "unsupported configuration";
        case SPLATRASTER_ERR_OVERFLOW: return "tile instance count overflow";
        case SPLATRASTER_WARN_LOOKBACK_STALL: return "look-back stall (results late, never wrong)";
        default: return "unknown status";
    }
}

const char* splatraster_last_hip_error(void) { return g_last_error.c_str(); }

size_t splatraster_geometry_bytes(int32_t P) { return geom_layout(nullptr, P, 1).bytes; }
size_t splatraster_binning_bytes(int32_t P, int64_t R, int32_t width, int32_t height, int32_t channels)
{
    return bin_layout(nullptr, P, 1, R, width, height, channels).bytes;
}
size_t splatraster_image_bytes(int32_t width, int32_t height) { return img_layout(nullptr, width, height, 1).bytes; }

size_t splatraster_window_geometry_bytes(int32_t P, int32_t n_views) { return geom_layout(nullptr, P, n_views).bytes; }
size_t splatraster_window_binning_bytes(int32_t P, int32_t n_views, int64_t R_total, int32_t width, int32_t height,
                                        int32_t channels)
{
    return bin_layout(nullptr, P, n_views, R_total, width, height, channels).bytes;
}
size_t splatraster_window_image_bytes(int32_t width, int32_t height, int32_t n_views)
{
    return img_layout(nullptr, width, height, n_views).bytes;
}

int splatraster_get_geometry_layout(int32_t P, splatraster_geometry_layout* out)
{
    return splatraster_get_window_geometry_layout(P, 1, out);
}
int splatraster_get_window_geometry_layout(int32_t P, int32_t n_views, splatraster_geometry_layout* out)
{
    if (!out || n_views < 1 || n_views > MAX_VIEWS) return SPLATRASTER_ERR_BAD_ARG;
    const GeomLayout L = geom_layout(nullptr, P, n_views);
    out->rec0 = L.rec0; out->rec1 = L.rec0 + 16; out->tiles_touched = L.tiles_touched;
    out->depth_order = L.depth_order; out->offsets = L.offsets; out->rgb = L.rgb;
    out->clamped = L.clamped; out->total = L.bytes;
    return SPLATRASTER_OK;
}
int splatraster_get_binning_layout(int32_t P, int64_t R, int32_t width, int32_t height, int32_t channels,
                                   splatraster_binning_layout* out)
{
    return splatraster_get_window_binning_layout(P, 1, R, width, height, channels, out);
}
int splatraster_get_window_binning_layout(int32_t P, int32_t n_views, int64_t R_total, int32_t width, int32_t height,
                                          int32_t channels, splatraster_binning_layout* out)
{
    if (!out || n_views < 1 || n_views > MAX_VIEWS) return SPLATRASTER_ERR_BAD_ARG;
    const BinLayout L = bin_layout(nullptr, P, n_views, R_total, width, height, channels);
    out->point_list = L.point_list; out->tile_list = L.tile_list; out->ranges = L.ranges; out->total = L.bytes;
    return SPLATRASTER_OK;
}
int splatraster_get_image_layout(int32_t width, int32_t height, splatraster_image_layout* out)
{
    return splatraster_get_window_image_layout(width, height, 1, out);
}
int splatraster_get_window_image_layout(int32_t width, int32_t height, int32_t n_views, splatraster_image_layout* out)
{
    if (!out || n_views < 1 || n_views > MAX_VIEWS) return SPLATRASTER_ERR_BAD_ARG;
    const ImgLayout L = img_layout(nullptr, width, height, n_views);
    out->final_T = 0; out->n_contrib = L.n_contrib; out->total = L.bytes;
    return SPLATRASTER_OK;
}

}  // extern "C"

namespace sr {

static int check_window(const splatraster_settings* s, int32_t V, const splatraster_window_view* views)
{
    int st = check_settings(s);
    if (st) return st;
    if (V < 1 || V > MAX_VIEWS || !views) return SPLATRASTER_ERR_BAD_ARG;
    return SPLATRASTER_OK;
}

static WinCams make_cams(int32_t V, const splatraster_window_view* views)
{
    WinCams c{};
    for (int v = 0; v < V; ++v) {
        c.view[v] = views[v].viewmatrix;
        c.proj[v] = views[v].projmatrix;
        c.campos[v] = views[v].campos;
        c.tanfovx[v] = views[v].tanfovx;
        c.tanfovy[v] = views[v].tanfovy;
        c.radii[v] = views[v].radii;
    }
    return c;
}

// The binned front end (binsort.hip) keeps its (tile, chunk) table and the state of its scan (BinScratch, common.h) where the
// radix front end keeps the depth-sort buffers (sort_keys ... scan_tmp): the geometry buffer's size does not depend on the path.

// What a stage WROTE at a buffer: the next stage is a separate public call and must follow that, not re-derive it from the
// process-wide debug switches as they stand by then (a switch flipped between two calls would otherwise make the render read a
// (tile, chunk) table that was never built, or the backward walk a stream or segment records nobody wrote).  The geometry stage
// records its front end under the geometry buffer, the render stage {front end, stream, segment records} under the binning
// buffer.  Host-side, keyed by the buffer's address; an address without a record (never seen, or dropped when the map was
// trimmed) falls back to the switches.
struct Written { bool binned, compact, split; };
static std::mutex g_written_mu;
static std::unordered_map<const void*, Written> g_written;
static void written_record(const void* at, const Written& w)
{
    std::lock_guard<std::mutex> lk(g_written_mu);
    if (g_written.size() > (1u << 15)) g_written.clear();   // (both kinds of buffer: twice the entries either kind used to be given)
    g_written[at] = w;
}
static bool written_find(const void* at, Written* w)
{
    std::lock_guard<std::mutex> lk(g_written_mu);
    auto it = g_written.find(at);
    if (it != g_written.end()) *w = it->second;
    return it != g_written.end();
}

// The launch plan of a frame (common.h).  `geometry`: follow the front end its geometry stage recorded (null: the geometry stage
// itself, which decides); `binning`: follow what its render stage recorded (the backwards).  R: the instances `binning` is laid
// out for (0 where no stream is decided).
static FramePlan frame_plan(int32_t W, int32_t H, int C, int32_t P, int32_t V, int64_t R, const void* geometry, const void* binning)
{
    FramePlan p{};
    const TileGrid tg = tile_grid(W, H);
    p.W = W; p.H = H; p.gx = tg.gx; p.gy = tg.gy; p.tiles = tg.gx * tg.gy; p.gtiles = (int64_t)p.tiles * V;
    p.P = P; p.V = V; p.C = C;
    p.order = SR_TILE_ORDER && 4 * p.gtiles <= TILE_ORDER_MAX_WAVES;
    p.team_every = g_fwd_team == 2 ? 1 : 0;
    Written w{};
    const bool rendered = binning && written_find(binning, &w);   // (then no forward follows: no team)
    if (!rendered && !(geometry && written_find(geometry, &w))) {
        // binned front end (binsort.hip): where the shape allows and its table fits the depth-sort scratch of the geometry buffer
        const GeomLayout L = geom_layout(nullptr, P, V);
        w.binned = g_bin_mode != 0 && P > 0 && p.tiles > 0 && p.tiles <= BIN_MAX_TILES && p.gx <= 255 && p.gy <= 255 &&
                   bin_table_entries(P, V, p.tiles) < ((size_t)1 << 31) && bin_scratch_layout(nullptr, P, V, p.tiles).bytes <= L.total - L.sort_keys &&
                   (g_bin_mode == 1 || p.gtiles <= BIN_AUTO_MAX_TILES);
    }
    p.binned = w.binned;
    p.split = rendered ? w.split : C <= 4 && 4 * p.gtiles <= g_split_max_waves;
    p.team = !rendered && (g_fwd_team < 0 ? p.split : (g_fwd_team != 0 && C <= 4));
    // compact payload (binning.hip payload_tile_kernel): behind the radix front end, for launches of one wave per quadrant over
    // whole lists — the binned front end writes its own payload, a team or a split launch walks full list positions
    p.compact = rendered ? w.compact : g_payload_compact != 0 && R > 0 && !p.binned && !p.split && !p.team;
    assert(!p.compact || (!p.binned && !p.split && !p.team && R > 0));
    p.dead_marks = g_dead_marks != 0;   // (read by the backward alone: an unmarked stream and an ignored mark are both walked in full)
    return p;
}

// The (BinView, ImgView) pair a compositing launch sees.  Compact stream: the kernels (unchanged) walk [cranges) of irec / ipack
// and count in its positions — the forward fills both planes (n_contrib, n_contrib_c), the backward receives n_contrib_c for
// n_contrib: its `idx < last` test and the bound list0 + wave_last then hold in compact positions.  Full stream: no n_contrib_c.
struct CompositeViews { BinView b; ImgView im; };
static CompositeViews composite_views(const FramePlan& p, BinView b, ImgView im, bool backward)
{
    if (!p.compact) im.n_contrib_c = nullptr;
    else {
        b.ranges = im.cranges;
        if (backward) im.n_contrib = im.n_contrib_c;
    }
    return CompositeViews{b, im};
}

static BinScratch bin_scratch(const FramePlan& p, void* geometry)
{
    if (!p.binned) return BinScratch{};
    return bin_scratch_layout(geom_view(geometry, p.P, p.V).sort_keys, p.P, p.V, p.tiles);
}

// Stage 1 of the forward over a window of V views (V = 1: the plain call): one preprocess, ONE depth sort of the
// V * P rows, one scan; the per-view instance counts are read back under the sort.
static int window_geometry(const splatraster_settings* s, int32_t V, const splatraster_window_view* views, int32_t P,
                           const float* means3D, const float* shs, const float* opacities, const float* scales,
                           const float* rotations, const float* cov3D_precomp, void* geometry, int64_t* num_rendered,
                           hipStream_t stream, const RawFwd* raw = nullptr,
                           bool bounded = false /*no count comes back (num_rendered is NULL) and the host waits for nothing: binned front end only*/)
{
    int st = check_window(s, V, views);
    if (st) return st;
    if (P < 0 || (!num_rendered && !bounded)) return SPLATRASTER_ERR_BAD_ARG;
    if (!bounded)
        for (int v = 0; v < V; ++v) num_rendered[v] = 0;
    if (P == 0) return bounded ? SPLATRASTER_ERR_UNSUPPORTED : SPLATRASTER_OK;
    if (raw) {      // the raw tensors stand in for opacities / scales / rotations (which are this call's OUTPUTS: raw->scales ...)
        if (shs || cov3D_precomp || !raw->scaling || !raw->rotation || !raw->opacity || !raw->f_dc || !raw->scales || !raw->rotations ||
            !raw->opacities || !raw->colors || raw->E != s->channels - 3 || (raw->E > 0 && !raw->extra))
            return SPLATRASTER_ERR_BAD_ARG;
        opacities = raw->opacities; scales = raw->scales; rotations = raw->rotations;
    }
    if (!means3D || !opacities || !geometry) return SPLATRASTER_ERR_BAD_ARG;
    for (int v = 0; v < V; ++v)
        if (!views[v].viewmatrix || !views[v].projmatrix || !views[v].radii) return SPLATRASTER_ERR_BAD_ARG;
    const bool have_sr = scales && rotations;
    if (have_sr == (cov3D_precomp != nullptr)) return SPLATRASTER_ERR_BAD_ARG;
    if ((scales == nullptr) != (rotations == nullptr)) return SPLATRASTER_ERR_BAD_ARG;
    if (shs) {
        if (V != 1) return SPLATRASTER_ERR_UNSUPPORTED;   // view-dependent colours: one table per view
        if (s->channels != 3 || !views[0].campos) return SPLATRASTER_ERR_BAD_ARG;
        if (s->sh_degree < 0 || s->sh_degree > 3) return SPLATRASTER_ERR_UNSUPPORTED;
        if (s->sh_coeffs < (s->sh_degree + 1) * (s->sh_degree + 1)) return SPLATRASTER_ERR_BAD_ARG;
    }
    if ((int64_t)P * V >= ((int64_t)1 << 31)) return SPLATRASTER_ERR_OVERFLOW;
    st = check_row_index_range(P, V, s->channels);   // (the depth-order words keep the row in 24 bits)
    if (st) return st;
    st = lookback_error_init();
    if (st) return st;
    const int32_t n = P * V;
    const GeomLayout L = geom_layout(geometry, P, V);
    GeomView g = L.v;
    const WinCams cams = make_cams(V, views);
    const FramePlan plan = frame_plan(s->image_width, s->image_height, s->channels, P, V, 0, nullptr, nullptr);
    if (bounded && !plan.binned) return SPLATRASTER_ERR_UNSUPPORTED;   // (nothing launched yet)
    written_record(geometry, Written{plan.binned, false, false});
    const BinScratch bins = bin_scratch(plan, geometry);
    HostSlot* slot = nullptr;
    const size_t nblk = (size_t)preprocess_blocks(P);
    if (!bounded) {
        st = host_slot(nblk * (size_t)V, &slot);
        if (st) return st;
        g.block_tiles = slot->dp;     // the per-(view, block) instance sums land in host memory
    }   // (bounded: nobody reads the sums; they stay in the geometry buffer's own scratch, and no kernel is left writing a pinned slot)
    // preprocess_kernel stores into the thread's pinned slot: an error return between its launch and the wait below must not
    // leave the kernel writing a slot the next call on this thread may free, reallocate or read (state 1: launched, wait for
    // the stream; 2: the event behind the kernel is recorded, wait for that; 0: nothing in flight)
    struct SlotGuard {
        HostSlot* slot; hipStream_t stream; int state;
        ~SlotGuard() { if (state == 2) (void)hipEventSynchronize(slot->ev); else if (state == 1) (void)hipStreamSynchronize(stream); }
    } guard{slot, stream, bounded ? 0 : 1};
    {
        StageTimer t(SPLATRASTER_STAGE_PREPROCESS, stream);
        // the look-back state of the depth sort and of the scan is cleared by preprocess_kernel
        if (plan.binned)
            st = launch_preprocess(*s, P, V, cams, means3D, shs, opacities, scales, rotations, cov3D_precomp, g, nullptr, 0u,
                                   reinterpret_cast<uint32_t*>(bins.scan_tmp), (uint32_t)(scan_state_bytes(bins.entries) / 4),
                                   stream, false, raw);
        else
            st = launch_preprocess(*s, P, V, cams, means3D, shs, opacities, scales, rotations, cov3D_precomp, g,
                                   g.sort_tmp, (uint32_t)(sort_zero_bytes(n, 32) / 4),
                                   reinterpret_cast<uint32_t*>(L.scan_tmp), (uint32_t)(scan_state_bytes(n) / 4), stream, true, raw);
    }
    if (st) return st;
    if (!bounded) {
        SR_HIP_CHECK(hipEventRecord(slot->ev, stream));
        guard.state = 2;
    }
    if (plan.binned) {
        // binned front end (binsort.hip): per-(tile, chunk) counts + their scan instead of the depth sort + offsets scan
        StageTimer t(SPLATRASTER_STAGE_DEPTH_SORT, stream);
        st = launch_bin_count(plan, g, bins.table, bins.scan_tmp, stream);
        if (st) return st;
    } else {
    {
        StageTimer t(SPLATRASTER_STAGE_DEPTH_SORT, stream);
        bool in_alt = false;
        st = sort_pairs_u32(n, g.sort_keys, g.depth_order, L.keys_alt, L.vals_alt, 32, g.sort_tmp, stream, &in_alt, true);
        if (st) return st;
        if (in_alt) return SPLATRASTER_ERR_UNSUPPORTED;  // 4 passes: never
    }
    {
        StageTimer t(SPLATRASTER_STAGE_SCAN, stream);
        st = inclusive_scan_u32(n, g.tiles_touched, g.depth_order, g.offsets, g.total, L.scan_tmp, stream, true,
                                g.span_owner, (uint32_t)EMIT_SPAN, SPAN_OWNER_CAP);
    }
    if (st) return st;
    }
    if (bounded) return SPLATRASTER_OK;   // R stays on the device (g.total)
    SR_HIP_CHECK(hipEventSynchronize(slot->ev));  // preprocess only: sort and scan may still be running
    guard.state = 0;
    uint64_t total = 0;
    for (int v = 0; v < V; ++v) {
        uint64_t tv = 0;
        for (size_t k = 0; k < nblk; ++k) tv += slot->p[(size_t)v * nblk + k];
        num_rendered[v] = (int64_t)tv;
        total += tv;
    }
    if (total >= ((uint64_t)1 << 31)) return SPLATRASTER_ERR_OVERFLOW;
    return SPLATRASTER_OK;
}

// Stage 2: ONE emission, ONE tile sort keyed by (view, tile), one payload pass, one compositing grid over the V views.
static int window_render(const splatraster_settings* s, int32_t V, const splatraster_window_view* views, int32_t P,
                         int64_t R, const float* bg, const float* colors_precomp, void* geometry, void* binning,
                         void* image, hipStream_t stream,
                         const BoundedRun* bd = nullptr /*bounded sequence: R is the CAPACITY `binning` was laid out for*/)
{
    int st = check_window(s, V, views);
    if (st) return st;
    if (P < 0 || R < 0 || !image) return SPLATRASTER_ERR_BAD_ARG;
    for (int v = 0; v < V; ++v)
        if (!views[v].out_color || !views[v].out_depth || !views[v].out_alpha) return SPLATRASTER_ERR_BAD_ARG;
    if (s->bg_channels > 0 && !bg) return SPLATRASTER_ERR_BAD_ARG;
    if (P > 0 && (!geometry || !binning)) return SPLATRASTER_ERR_BAD_ARG;
    if (V > 1 && !colors_precomp && P > 0) return SPLATRASTER_ERR_UNSUPPORTED;
    st = check_row_index_range(P, V, s->channels);
    if (st) return st;
    if (!binning) return SPLATRASTER_ERR_BAD_ARG;
    const FramePlan plan = frame_plan(s->image_width, s->image_height, s->channels, P, V, R, geometry, nullptr);
    const int W = plan.W, H = plan.H;
    const int64_t gtiles = plan.gtiles;
    if (gtiles >= ((int64_t)1 << 31)) return SPLATRASTER_ERR_OVERFLOW;
    const ImgView im = img_view(image, W, H, V);
    GeomView g{};
    if (geometry) g = geom_view(geometry, P, V);
    const BinView b = bin_view(binning, P, V, R, W, H, s->channels);
    const float* feat = colors_precomp ? colors_precomp : g.rgb;
    if ((R > 0 || bd) && !feat) return SPLATRASTER_ERR_BAD_ARG;
    const int bits = tile_bits((int)gtiles);
    const int passes = (bits + 7) / 8;
    // emit into the buffer pair from which `passes` ping-pongs end in (tile_list, point_list); with 16-bit keys (sort_keys16) the
    // same pair: the uint16_t keys fill the first half of k0 (and of k1 after the first of two passes), and the last pass
    // reads them from the buffer that is NOT tile_list (1 pass: keys_tmp -> tile_list; 2: tile_list -> keys_tmp -> tile_list)
    uint32_t* k0 = (passes & 1) ? b.keys_tmp : b.tile_list;
    uint32_t* v0 = (passes & 1) ? b.vals_tmp : b.point_list;
    uint32_t* k1 = (passes & 1) ? b.tile_list : b.keys_tmp;
    uint32_t* v1 = (passes & 1) ? b.point_list : b.vals_tmp;
    // a bounded sequence always has the binned front end: whether the frame is empty is known on the device only, and the
    // front end itself leaves a cleared range table and a valid launch order when the total is 0
    if (bd && !plan.binned) return SPLATRASTER_ERR_UNSUPPORTED;
    const BinScratch bins = bin_scratch(plan, geometry);
    const bool binned = plan.binned && (R > 0 || bd);   // (its launches run)
    if (binned) {
        // binned front end: scatter the 64-bit keys into their (tile, chunk) pieces, sort every tile's list in LDS and write
        // the payload + lists + ranges (binsort.hip); the keys live where the radix path keeps its unsorted pairs
        StageTimer t(SPLATRASTER_STAGE_TILE_SORT, stream);
        st = launch_bin_scatter_sort(plan, g, bins.table, b, reinterpret_cast<uint64_t*>(b.keys_tmp), stream, bd);
        if (st) return st;
    }
    if (R > 0 && !plan.binned) {
        const bool keys16 = SR_TILE_KEYS16 && sort_keys16(R, bits);
        {
            StageTimer t(SPLATRASTER_STAGE_EMIT, stream);
            st = launch_emit(plan, R, g, k0, v0, b.ranges, 2u * (uint32_t)gtiles, stream, keys16);  // also clears the range table
        }
        if (st) return st;
        bool in_alt = false;
        {
            StageTimer t(SPLATRASTER_STAGE_TILE_SORT, stream);
            st = keys16 ? sort_pairs_k16(R, k0, v0, k1, v1, bits, b.sort_tmp, stream, &in_alt)
                        : sort_pairs_u32(R, k0, v0, k1, v1, bits, b.sort_tmp, stream, &in_alt);
        }
        if (st) return st;
    }
    if (R == 0 && !bd) {   // nothing was emitted: the table is cleared here instead
        StageTimer t(SPLATRASTER_STAGE_RANGES, stream);
        st = launch_ranges_clear((int32_t)gtiles, b.ranges, stream);
    }
    if (st) return st;
    const float* featp = feat;  // 16-byte aligned rows for the compositing kernels
    written_record(binning, Written{plan.binned, plan.compact, plan.split});
    if (R > 0 || bd) {
        StageTimer t(SPLATRASTER_STAGE_PAYLOAD, stream);
        if (plan.compact) st = launch_payload_compact(plan, R, g, b, im.cranges, stream);
        else if (!plan.binned) st = launch_payload(plan, R, g, b, stream);
        if (st) return st;
        if (s->channels % 4) {
            st = launch_pad_features(P, s->channels, feat, b.featp, stream);
            featp = b.featp;
        }
    }
    if (st) return st;
    if (!binned) {               // launch order of the compositing grids (the range table is final here, also when nothing was
                                 // emitted); the binned front end's last launch has computed it (binsort.hip)
        StageTimer t(SPLATRASTER_STAGE_RANGES, stream);
        st = launch_tile_order(plan, b, stream);
    }
    if (st) return st;
    WinOut outs{};
    for (int v = 0; v < V; ++v) {
        outs.color[v] = views[v].out_color;
        outs.depth[v] = views[v].out_depth;
        outs.alpha[v] = views[v].out_alpha;
    }
    const CompositeViews cv = composite_views(plan, b, im, false);
    StageTimer t(SPLATRASTER_STAGE_COMPOSITE_FWD, stream);
    return launch_composite_fwd(*s, plan, cv.b, cv.im, featp, bg, outs, stream);
}

// What every backward of a window starts with (after its own argument checks): the per-view gradient planes, the fill of the
// accumulator rows (`pose`: and of the camera-gradient sets right behind them) and the compositing backward into them, the
// deterministic debug mode included.  `out`: the buffer views, cameras and gradient planes the per-Gaussian pass then reads.
struct BwdRows { GeomView g; BinView b; WinCams cams; WinGrad grads; };
static int window_accumulate(const splatraster_settings* s, int32_t V, const splatraster_window_view* views, int32_t P, int64_t R,
                             const float* bg, const float* colors_precomp, bool sh_colours, void* geometry, const void* binning,
                             const void* image, bool pose, hipStream_t stream, BwdRows* out)
{
    int st = check_row_index_range(P, V, s->channels);
    if (st) return st;
    const int W = s->image_width, H = s->image_height;
    GeomView& g = out->g;
    BinView& b = out->b;
    g = geom_view(geometry, P, V);
    b = bin_view(const_cast<void*>(binning), P, V, R, W, H, s->channels);
    // the stream and the segment records as the render stage wrote them (`out` keeps the plain views)
    const FramePlan plan = frame_plan(W, H, s->channels, P, V, R, geometry, binning);
    const CompositeViews cv = composite_views(plan, b, img_view(const_cast<void*>(image), W, H, V), true);
    const int C = s->channels;
    const float* feat = sh_colours ? g.rgb : colors_precomp;
    WinCams& cams = out->cams;
    WinGrad& grads = out->grads;
    cams = make_cams(V, views);
    grads = WinGrad{};
    grads.gc = C;
    for (int v = 0; v < V; ++v) {
        const int gcv = views[v].color_grad_channels;
        if (gcv < 0 || gcv > C) return SPLATRASTER_ERR_BAD_ARG;
        if (gcv != 0 && gcv < C) grads.gc = gcv;
    }
    for (int v = 0; v < V; ++v) {   // one convention per launch: all views split the last channel off, or none does
        const int gcv = views[v].color_grad_channels ? views[v].color_grad_channels : C;
        if (gcv != grads.gc) return SPLATRASTER_ERR_BAD_ARG;
        grads.dL_dlast[v] = grads.gc < C ? views[v].dL_dout_last : nullptr;
    }
    for (int v = 0; v < V; ++v) {
        grads.out_color[v] = views[v].out_color;
        grads.out_depth[v] = views[v].out_depth;
        grads.dL_dcolor[v] = views[v].dL_dout_color;
        grads.dL_ddepth[v] = views[v].dL_dout_depth;
        grads.dL_dalpha[v] = views[v].dL_dout_alpha;
        grads.dL_dmeans2D[v] = views[v].dL_dmeans2D;
    }
    // zero the accumulator rows (outside the stage bracket: the stage is the kernel alone, so its
    // figure can be held against the per-kernel rocprofv3 average)
    const size_t gacc_n = gacc_total_floats(C, (size_t)P, (size_t)V);   // shared colour rows + per-(view, Gaussian) rows
    const bool det = g_deterministic != 0;
    long long* gacc64 = nullptr;   // debug mode only: stream-ordered scratch, freed below (never part of `binning`)
    if (det) {
        SR_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&gacc64), sizeof(long long) * gacc_n, stream));
        SR_HIP_CHECK(hipMemsetAsync(gacc64, 0, sizeof(long long) * gacc_n, stream));
    }
    // (one fill: the camera-gradient accumulator sets lie directly behind the rows)
    const size_t fill = pose ? (size_t)(reinterpret_cast<char*>(b.pose_acc) - reinterpret_cast<char*>(b.gacc)) + POSE_ACC_BYTES
                             : sizeof(float) * gacc_n;
    SR_HIP_CHECK(hipMemsetAsync(b.gacc, 0, fill, stream));
    grads.bg = bg;
    grads.bg_channels = bg ? s->bg_channels : 0;
    {
        StageTimer t(SPLATRASTER_STAGE_COMPOSITE_BWD, stream);
        // deterministic mode: the kernel runs twice — per-element max of |partial| (into the zeroed float rows), then the
        // fixed-point sums scaled by that maximum (composite_bwd.hip acc_add)
        if (det) st = launch_composite_bwd(plan, R, cv.b, cv.im, (C % 4) ? b.featp : feat, C, grads, b.gacc, gacc64, 0, stream);
        if (!st) st = launch_composite_bwd(plan, R, cv.b, cv.im, (C % 4) ? b.featp : feat, C, grads, b.gacc, gacc64, 1, stream);
    }
    if (det) {
        if (!st) st = launch_fixed_to_float((int64_t)gacc_n, gacc64, b.gacc, gacc_det_headroom_drop(C, V), stream);
        (void)hipFreeAsync(gacc64, stream);
    }
    return st;
}

// Backward of the window: one compositing grid over the V views into per-(view, Gaussian) accumulator rows, then
// ONE per-Gaussian pass that sums the views into a single set of parameter gradients.
static int window_backward(const splatraster_settings* s, int32_t V, const splatraster_window_view* views, int32_t P,
                           int64_t R, const float* bg, const float* means3D, const float* shs, const float* colors_precomp,
                           const float* scales, const float* rotations, const float* cov3D_precomp, void* geometry,
                           const void* binning, const void* image, float* dL_dmeans3D, float* dL_dcolors,
                           float* dL_dopacities, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                           float* dL_dshs, float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos,
                           hipStream_t stream, const RawBwd* raw = nullptr)
{
    int st = check_window(s, V, views);
    if (st) return st;
    if (P < 0 || R < 0) return SPLATRASTER_ERR_BAD_ARG;
    if (V > 1 && (shs || dL_dviewmatrix || dL_dprojmatrix || dL_dcampos)) return SPLATRASTER_ERR_UNSUPPORTED;
    if (raw && (shs || cov3D_precomp || dL_dviewmatrix || dL_dprojmatrix || dL_dcampos)) return SPLATRASTER_ERR_UNSUPPORTED;
    if (P == 0) {   // nothing to differentiate: the camera gradients are still defined (zero)
        if (dL_dviewmatrix) SR_HIP_CHECK(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), stream));
        if (dL_dprojmatrix) SR_HIP_CHECK(hipMemsetAsync(dL_dprojmatrix, 0, 16 * sizeof(float), stream));
        if (dL_dcampos) SR_HIP_CHECK(hipMemsetAsync(dL_dcampos, 0, 3 * sizeof(float), stream));
        return SPLATRASTER_OK;
    }
    if (!means3D || !geometry || !binning || !image || !dL_dmeans3D || (!dL_dopacities && !raw)) return SPLATRASTER_ERR_BAD_ARG;
    if (raw && (P > 0) && (!raw->scaling || !raw->rotation || !raw->opacity || !raw->f_dc || !raw->d_scaling || !raw->d_rotation ||
                           !raw->d_opacity || !raw->d_f_dc || raw->E != s->channels - 3 || (raw->E > 0 && !raw->d_extra)))
        return SPLATRASTER_ERR_BAD_ARG;
    for (int v = 0; v < V; ++v)
        if (!views[v].viewmatrix || !views[v].projmatrix || !views[v].radii || !views[v].out_color || !views[v].out_depth ||
            !views[v].dL_dout_color || !views[v].dL_dmeans2D)
            return SPLATRASTER_ERR_BAD_ARG;
    if (shs && (!dL_dshs || !views[0].campos)) return SPLATRASTER_ERR_BAD_ARG;
    if (!shs && (!colors_precomp || (!dL_dcolors && !raw))) return SPLATRASTER_ERR_BAD_ARG;
    if (cov3D_precomp ? !dL_dcov3D : (!scales || !rotations || ((!dL_dscales || !dL_drotations) && !raw)))
        return SPLATRASTER_ERR_BAD_ARG;
    BwdRows rows;
    st = window_accumulate(s, V, views, P, R, bg, colors_precomp, shs != nullptr, geometry, binning, image,
                           dL_dviewmatrix && dL_dprojmatrix, stream, &rows);
    if (st) return st;
    const GeomView& g = rows.g;
    const BinView& b = rows.b;
    const WinCams& cams = rows.cams;
    const WinGrad& grads = rows.grads;
    const int C = s->channels;
    StageTimer t(SPLATRASTER_STAGE_PREPROCESS_BWD, stream);
    return launch_preprocess_bwd(*s, P, V, cams, grads, means3D, shs, scales, rotations, cov3D_precomp, g.clamped, g.rec,
                                 b.gacc, C, shs ? nullptr : dL_dcolors, dL_dmeans3D, dL_dopacities,
                                 cov3D_precomp ? nullptr : dL_dscales, cov3D_precomp ? nullptr : dL_drotations,
                                 cov3D_precomp ? dL_dcov3D : nullptr, dL_dshs, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos,
                                 b.pose_acc, stream, raw);
}

static RawFwd raw_forward(const splatraster_raw_forward& rf)
{
    return RawFwd{rf.scaling, rf.rotation, rf.opacity, rf.f_dc, rf.extra, rf.extra_channels, rf.scales, rf.rotations, rf.opacities, rf.colors};
}

// R of a window: the sum of the per-view instance counts its geometry stage returned
static int window_instances(int32_t V, const int64_t* num_rendered, int64_t* R)
{
    if (!num_rendered || V < 1 || V > MAX_VIEWS) return SPLATRASTER_ERR_BAD_ARG;
    *R = 0;
    for (int v = 0; v < V; ++v) {
        if (num_rendered[v] < 0) return SPLATRASTER_ERR_BAD_ARG;
        *R += num_rendered[v];
    }
    return SPLATRASTER_OK;
}

// What splatraster_backward_window_cameras and _joint check first: the window, then P, the workspace, the camera outputs and the
// counts (summed into *R).  P == 0 leaves nothing to differentiate, but the camera gradients are still defined: zero, filled here.
static int camera_window_begin(const splatraster_settings* s, int32_t V, const splatraster_window_view* views, int32_t P,
                               const int64_t* num_rendered, const void* workspace, float* dL_dviewmatrix, float* dL_dprojmatrix,
                               float* dL_dcampos, hipStream_t stream, int64_t* R)
{
    int st = check_window(s, V, views);
    if (st) return st;
    if (P < 0 || !workspace || !dL_dviewmatrix || !dL_dprojmatrix || window_instances(V, num_rendered, R)) return SPLATRASTER_ERR_BAD_ARG;
    if (P == 0) {
        SR_HIP_CHECK(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float) * (size_t)V, stream));
        SR_HIP_CHECK(hipMemsetAsync(dL_dprojmatrix, 0, 16 * sizeof(float) * (size_t)V, stream));
        if (dL_dcampos) SR_HIP_CHECK(hipMemsetAsync(dL_dcampos, 0, 3 * sizeof(float) * (size_t)V, stream));
    }
    return SPLATRASTER_OK;
}

}  // namespace sr

extern "C" {

int splatraster_forward_geometry(const splatraster_settings* s, int32_t P, const float* means3D,
                                 const float* shs, const float* opacities, const float* scales,
                                 const float* rotations, const float* cov3D_precomp,
                                 const float* viewmatrix, const float* projmatrix, const float* campos,
                                 void* geometry, int32_t* radii, int64_t* num_rendered, void* stream_)
{
    if (!s) return SPLATRASTER_ERR_BAD_ARG;
    splatraster_window_view w{};
    w.viewmatrix = viewmatrix; w.projmatrix = projmatrix; w.campos = campos;
    w.tanfovx = s->tanfovx; w.tanfovy = s->tanfovy; w.radii = radii;
    if (num_rendered) *num_rendered = 0;
    if (P > 0 && !radii) return SPLATRASTER_ERR_BAD_ARG;
    return window_geometry(s, 1, &w, P, means3D, shs, opacities, scales, rotations, cov3D_precomp, geometry, num_rendered,
                           reinterpret_cast<hipStream_t>(stream_));
}

int splatraster_forward_render(const splatraster_settings* s, int32_t P, int64_t R, const float* bg,
                               const float* colors_precomp, void* geometry, void* binning, void* image,
                               float* out_color, float* out_depth, float* out_alpha, void* stream_)
{
    if (!s) return SPLATRASTER_ERR_BAD_ARG;
    splatraster_window_view w{};
    w.tanfovx = s->tanfovx; w.tanfovy = s->tanfovy;
    w.out_color = out_color; w.out_depth = out_depth; w.out_alpha = out_alpha;
    return window_render(s, 1, &w, P, R, bg, colors_precomp, geometry, binning, image, reinterpret_cast<hipStream_t>(stream_));
}

int splatraster_backward(const splatraster_settings* s, int32_t P, int64_t R, const float* bg,
                         const float* means3D, const float* shs, const float* colors_precomp,
                         const float* opacities, const float* scales, const float* rotations,
                         const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                         const float* campos, const int32_t* radii, void* geometry,
                         const void* binning, const void* image, const float* out_color,
                         const float* out_depth, const float* out_alpha, const float* dL_dout_color,
                         const float* dL_dout_depth, const float* dL_dout_alpha, float* dL_dmeans3D,
                         float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacities, float* dL_dscales,
                         float* dL_drotations, float* dL_dcov3D, float* dL_dshs, float* dL_dviewmatrix,
                         float* dL_dprojmatrix, float* dL_dcampos, void* stream_)
{
    (void)opacities; (void)out_alpha;
    if (!s) return SPLATRASTER_ERR_BAD_ARG;
    splatraster_window_view w{};
    w.viewmatrix = viewmatrix; w.projmatrix = projmatrix; w.campos = campos;
    w.tanfovx = s->tanfovx; w.tanfovy = s->tanfovy; w.radii = const_cast<int32_t*>(radii);
    w.out_color = const_cast<float*>(out_color); w.out_depth = const_cast<float*>(out_depth);
    w.dL_dout_color = dL_dout_color; w.dL_dout_depth = dL_dout_depth; w.dL_dout_alpha = dL_dout_alpha;
    w.dL_dmeans2D = dL_dmeans2D;
    return window_backward(s, 1, &w, P, R, bg, means3D, shs, colors_precomp, scales, rotations, cov3D_precomp, geometry, binning,
                           image, dL_dmeans3D, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D, dL_dshs,
                           dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, reinterpret_cast<hipStream_t>(stream_));
}

int splatraster_forward_window_geometry(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                        int32_t P, const float* means3D, const float* opacities, const float* scales,
                                        const float* rotations, const float* cov3D_precomp, void* geometry,
                                        int64_t* num_rendered, void* stream)
{
    return window_geometry(s, n_views, views, P, means3D, nullptr, opacities, scales, rotations, cov3D_precomp, geometry,
                           num_rendered, reinterpret_cast<hipStream_t>(stream));
}

int splatraster_forward_window_render(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                      int32_t P, const int64_t* num_rendered, const float* bg, const float* colors_precomp,
                                      void* geometry, void* binning, void* image, void* stream)
{
    int64_t R;
    if (window_instances(n_views, num_rendered, &R)) return SPLATRASTER_ERR_BAD_ARG;
    return window_render(s, n_views, views, P, R, bg, colors_precomp, geometry, binning, image,
                         reinterpret_cast<hipStream_t>(stream));
}

int splatraster_backward_window(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                int32_t P, const int64_t* num_rendered, const float* bg, const float* means3D, const float* colors_precomp,
                                const float* scales, const float* rotations, const float* cov3D_precomp, void* geometry,
                                const void* binning, const void* image, float* dL_dmeans3D, float* dL_dcolors,
                                float* dL_dopacities, float* dL_dscales, float* dL_drotations, float* dL_dcov3D, void* stream)
{
    int64_t R;
    if (window_instances(n_views, num_rendered, &R)) return SPLATRASTER_ERR_BAD_ARG;
    return window_backward(s, n_views, views, P, R, bg, means3D, nullptr, colors_precomp, scales, rotations, cov3D_precomp,
                           geometry, binning, image, dL_dmeans3D, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations,
                           dL_dcov3D, nullptr, nullptr, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
}

size_t splatraster_window_camera_workspace_bytes(int32_t n_views)
{
    return (n_views < 1 || n_views > MAX_VIEWS) ? 0 : (size_t)n_views * POSE_ACC_BYTES;
}

int splatraster_backward_window_cameras(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                        int32_t P, const int64_t* num_rendered, const float* bg, const float* means3D,
                                        const float* colors_precomp, const float* scales, const float* rotations,
                                        const float* cov3D_precomp, void* geometry, const void* binning, const void* image,
                                        void* workspace, float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos,
                                        void* stream_)
{
    const int32_t V = n_views;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    int64_t R;
    int st = camera_window_begin(s, V, views, P, num_rendered, workspace, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, stream, &R);
    if (st || P == 0) return st;
    if (!means3D || !colors_precomp || !geometry || !binning || !image) return SPLATRASTER_ERR_BAD_ARG;
    if (cov3D_precomp ? (scales || rotations) : (!scales || !rotations)) return SPLATRASTER_ERR_BAD_ARG;
    for (int v = 0; v < V; ++v)     // (dL_dmeans2D is not written here and may be NULL)
        if (!views[v].viewmatrix || !views[v].projmatrix || !views[v].radii || !views[v].out_color || !views[v].out_depth ||
            !views[v].dL_dout_color)
            return SPLATRASTER_ERR_BAD_ARG;
    BwdRows rows;
    st = window_accumulate(s, V, views, P, R, bg, colors_precomp, false, geometry, binning, image, false, stream, &rows);
    if (st) return st;
    // the sets and tickets of the V views: the caller's memory, zeroed on the stream in front of the kernel that adds to them
    SR_HIP_CHECK(hipMemsetAsync(workspace, 0, splatraster_window_camera_workspace_bytes(V), stream));
    StageTimer t(SPLATRASTER_STAGE_PREPROCESS_BWD, stream);
    return launch_camera_bwd(*s, P, V, rows.cams, means3D, scales, rotations, cov3D_precomp, rows.g.rec, rows.b.gacc, s->channels,
                             reinterpret_cast<float*>(workspace), dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, stream);
}

int splatraster_backward_window_joint(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                      int32_t P, const int64_t* num_rendered, const float* bg, const float* means3D,
                                      const float* colors_precomp, const float* scales, const float* rotations,
                                      const float* cov3D_precomp, void* geometry, const void* binning, const void* image,
                                      float* dL_dmeans3D, float* dL_dcolors, float* dL_dopacities, float* dL_dscales,
                                      float* dL_drotations, float* dL_dcov3D, void* workspace, float* dL_dviewmatrix,
                                      float* dL_dprojmatrix, float* dL_dcampos, void* stream_)
{
    const int32_t V = n_views;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    int64_t R;
    int st = camera_window_begin(s, V, views, P, num_rendered, workspace, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, stream, &R);
    if (st || P == 0) return st;
    if (!means3D || !colors_precomp || !geometry || !binning || !image || !dL_dmeans3D || !dL_dcolors || !dL_dopacities)
        return SPLATRASTER_ERR_BAD_ARG;
    if (cov3D_precomp ? (scales || rotations || !dL_dcov3D) : (!scales || !rotations || !dL_dscales || !dL_drotations))
        return SPLATRASTER_ERR_BAD_ARG;
    for (int v = 0; v < V; ++v)
        if (!views[v].viewmatrix || !views[v].projmatrix || !views[v].radii || !views[v].out_color || !views[v].out_depth ||
            !views[v].dL_dout_color || !views[v].dL_dmeans2D)
            return SPLATRASTER_ERR_BAD_ARG;
    // ONE accumulator fill and ONE compositing backward for both gradient sets
    BwdRows rows;
    st = window_accumulate(s, V, views, P, R, bg, colors_precomp, false, geometry, binning, image, false, stream, &rows);
    if (st) return st;
    // the sets and tickets of the V views: the caller's memory, zeroed on the stream in front of the kernel that adds to them
    SR_HIP_CHECK(hipMemsetAsync(workspace, 0, splatraster_window_camera_workspace_bytes(V), stream));
    StageTimer t(SPLATRASTER_STAGE_PREPROCESS_BWD, stream);
    return launch_window_joint_bwd(*s, P, V, rows.cams, rows.grads, means3D, scales, rotations, cov3D_precomp, rows.g.rec,
                                   rows.b.gacc, s->channels, dL_dcolors, dL_dmeans3D, dL_dopacities,
                                   cov3D_precomp ? nullptr : dL_dscales, cov3D_precomp ? nullptr : dL_drotations,
                                   cov3D_precomp ? dL_dcov3D : nullptr, reinterpret_cast<float*>(workspace), dL_dviewmatrix,
                                   dL_dprojmatrix, dL_dcampos, stream);
}

int splatraster_forward_window_geometry_raw(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                            int32_t P, const float* means3D, const splatraster_raw_forward* rf, void* geometry,
                                            int64_t* num_rendered, void* stream)
{
    if (!rf) return SPLATRASTER_ERR_BAD_ARG;
    const RawFwd raw = raw_forward(*rf);
    return window_geometry(s, n_views, views, P, means3D, nullptr, nullptr, nullptr, nullptr, nullptr, geometry, num_rendered,
                           reinterpret_cast<hipStream_t>(stream), &raw);
}

// Geometry + render as one launch sequence into a binning buffer of `capacity` instances (include/splatraster.h, "bounded window
// forward"): every check of both stages that can fail does so before the first launch.
static int window_bounded(const splatraster_settings* s, int32_t V, const splatraster_window_view* views, int32_t P,
                          const float* means3D, const float* opacities, const float* scales, const float* rotations,
                          const float* cov3D_precomp, const RawFwd* raw, const float* bg, const float* colors_precomp, void* geometry,
                          void* binning, void* image, int64_t capacity, uint32_t tag, void* status, hipStream_t stream)
{
    int st = check_window(s, V, views);
    if (st) return st;
    if (!status || capacity < 0 || P < 0 || !geometry || !binning || !image || !colors_precomp) return SPLATRASTER_ERR_BAD_ARG;
    if (capacity >= ((int64_t)1 << 31)) return SPLATRASTER_ERR_OVERFLOW;
    if (s->bg_channels > 0 && !bg) return SPLATRASTER_ERR_BAD_ARG;
    for (int v = 0; v < V; ++v)
        if (!views[v].out_color || !views[v].out_depth || !views[v].out_alpha) return SPLATRASTER_ERR_BAD_ARG;
    const BoundedStatus* h = reinterpret_cast<const BoundedStatus*>(status);
    const BoundedRun bd{(uint32_t)capacity, tag, h->dev, h->host_dev};
    st = window_geometry(s, V, views, P, means3D, nullptr, opacities, scales, rotations, cov3D_precomp, geometry, nullptr, stream,
                         raw, true);
    if (st) return st;
    return window_render(s, V, views, P, capacity, bg, colors_precomp, geometry, binning, image, stream, &bd);
}

int splatraster_forward_window_bounded_supported(int32_t P, int32_t n_views, int32_t width, int32_t height)
{
    if (P <= 0 || n_views < 1 || n_views > MAX_VIEWS || width <= 0 || height <= 0) return 0;
    return frame_plan(width, height, 1, P, n_views, 0, nullptr, nullptr).binned ? 1 : 0;
}

int splatraster_forward_window_bounded(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                       int32_t P, const float* means3D, const float* opacities, const float* scales,
                                       const float* rotations, const float* cov3D_precomp, const float* bg,
                                       const float* colors_precomp, void* geometry, void* binning, void* image,
                                       int64_t capacity, uint32_t tag, void* status, void* stream)
{
    return window_bounded(s, n_views, views, P, means3D, opacities, scales, rotations, cov3D_precomp, nullptr, bg, colors_precomp,
                          geometry, binning, image, capacity, tag, status, reinterpret_cast<hipStream_t>(stream));
}

int splatraster_forward_window_bounded_raw(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                           int32_t P, const float* means3D, const splatraster_raw_forward* rf, const float* bg,
                                           void* geometry, void* binning, void* image, int64_t capacity, uint32_t tag,
                                           void* status, void* stream)
{
    if (!rf) return SPLATRASTER_ERR_BAD_ARG;
    const RawFwd raw = raw_forward(*rf);
    return window_bounded(s, n_views, views, P, means3D, nullptr, nullptr, nullptr, nullptr, &raw, bg, rf->colors, geometry, binning,
                          image, capacity, tag, status, reinterpret_cast<hipStream_t>(stream));
}

int splatraster_backward_window_raw(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                    int32_t P, const int64_t* num_rendered, const float* bg, const float* means3D,
                                    const float* colors_precomp, const float* scales, const float* rotations, void* geometry,
                                    const void* binning, const void* image, const splatraster_raw_params* rp, float* dL_dmeans3D,
                                    void* stream)
{
    int64_t R;
    if (window_instances(n_views, num_rendered, &R) || !rp) return SPLATRASTER_ERR_BAD_ARG;
    if (rp->reg_row_grad && !rp->reg_out) return SPLATRASTER_ERR_BAD_ARG;
    const RawBwd raw{rp->scaling, rp->rotation, rp->opacity, rp->f_dc, rp->extra_channels, rp->dL_dscaling, rp->dL_drotation,
                     rp->dL_dopacity, rp->dL_df_dc, rp->dL_dextra, rp->reg_row_grad, rp->reg_out, rp->reg_weight};
    return window_backward(s, n_views, views, P, R, bg, means3D, nullptr, colors_precomp, scales, rotations, nullptr,
                           geometry, binning, image, dL_dmeans3D, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, nullptr, reinterpret_cast<hipStream_t>(stream), &raw);
}

int splatraster_debug_set_small_panel_max_waves(int waves)
{
    set_small_panel_max_waves(waves);
    return SPLATRASTER_OK;
}

int splatraster_debug_set_payload_stream_min(int64_t instances)
{
    sr::set_payload_stream_min(instances);
    return SPLATRASTER_OK;
}

int splatraster_debug_set_payload_compact(int mode)
{
    g_payload_compact = mode < 0 ? -1 : (mode ? 1 : 0);
    return SPLATRASTER_OK;
}

int splatraster_debug_set_dead_marks(int on)
{
    g_dead_marks = on ? 1 : 0;
    return SPLATRASTER_OK;
}

int splatraster_debug_set_front_end(int mode)
{
    g_bin_mode = mode < 0 ? -1 : (mode > 1 ? 1 : mode);
    return SPLATRASTER_OK;
}

int splatraster_debug_set_sort_fork(int mode)
{
    set_bin_fork(mode);
    return SPLATRASTER_OK;
}

int splatraster_debug_set_tile_sort_cap(int keys)
{
    set_bin_tile_cap(keys);
    return SPLATRASTER_OK;
}

int splatraster_debug_set_split_max_waves(int waves)
{
    g_split_max_waves = waves < 0 ? SPLIT_MAX_WAVES : (waves > SPLIT_MAX_WAVES ? SPLIT_MAX_WAVES : waves);
    return SPLATRASTER_OK;
}

int splatraster_debug_set_fwd_team(int mode)
{
    g_fwd_team = mode < 0 ? -1 : (mode > 2 ? 2 : mode);
    return SPLATRASTER_OK;
}

int splatraster_mark_visible(int32_t P, const float* means3D, const float* viewmatrix,
                             const float* projmatrix, uint8_t* present, void* stream)
{
    (void)projmatrix;
    if (P < 0) return SPLATRASTER_ERR_BAD_ARG;
    if (P == 0) return SPLATRASTER_OK;
    if (!means3D || !viewmatrix || !present) return SPLATRASTER_ERR_BAD_ARG;
    return launch_mark_visible(P, means3D, viewmatrix, present, reinterpret_cast<hipStream_t>(stream));
}

int splatraster_poll_errors(void) { return lookback_error_poll(); }

int splatraster_debug_set_deterministic(int on)
{
    g_deterministic = on ? 1 : 0;
    return SPLATRASTER_OK;
}

int splatraster_debug_set_spin_limit(uint32_t limit)
{
    int st = lookback_error_init();
    if (st) return st;
    return lookback_set_spin_limit(limit);
}

int splatraster_debug_exp2(int64_t n, const float* x, float* y, void* stream)
{
    if (n < 0) return SPLATRASTER_ERR_BAD_ARG;
    if (n == 0) return SPLATRASTER_OK;
    if (!x || !y) return SPLATRASTER_ERR_BAD_ARG;
    return launch_debug_exp2(n, x, y, reinterpret_cast<hipStream_t>(stream));
}

int splatraster_debug_poison_lds(uint32_t pattern, void* stream)
{
    return launch_poison_lds(pattern, reinterpret_cast<hipStream_t>(stream));
}

// keys / vals sorted in place: the alternate arrays are the first two sections of tmp, the sort's own scratch the third
struct SortInPlace { uint32_t *keys_alt, *vals_alt; void* tmp; size_t bytes; };
static SortInPlace sort_in_place_layout(void* base, int64_t n)
{
    const size_t m = (size_t)(n > 0 ? n : 1);
    SortInPlace L;
    Carver c{base};
    L.keys_alt = c.take<uint32_t>(m);
    L.vals_alt = c.take<uint32_t>(m);
    L.tmp = c.take<char>(sort_tmp_bytes(n));
    L.bytes = c.o;
    return L;
}
size_t splatraster_sort_tmp_bytes(int64_t n) { return sort_in_place_layout(nullptr, n).bytes; }

static int sort_in_place(bool keys16, int64_t n, uint32_t* keys, uint32_t* vals, int32_t key_bits, void* tmp, void* stream_)
{
    if (!keys || !vals || !tmp) return SPLATRASTER_ERR_BAD_ARG;
    {
        int st0 = lookback_error_init();
        if (st0) return st0;
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const SortInPlace L = sort_in_place_layout(tmp, n);
    uint32_t *ka = L.keys_alt, *va = L.vals_alt;
    bool in_alt = false;
    int st = keys16 ? sort_pairs_k16(n, keys, vals, ka, va, key_bits, L.tmp, stream, &in_alt)
                    : sort_pairs_u32(n, keys, vals, ka, va, key_bits, L.tmp, stream, &in_alt);
    if (st) return st;
    if (in_alt) {
        SR_HIP_CHECK(hipMemcpyAsync(keys, ka, 4 * (size_t)n, hipMemcpyDeviceToDevice, stream));
        SR_HIP_CHECK(hipMemcpyAsync(vals, va, 4 * (size_t)n, hipMemcpyDeviceToDevice, stream));
    }
    return SPLATRASTER_OK;
}

int splatraster_sort_pairs_u32(int64_t n, uint32_t* keys, uint32_t* vals, int32_t key_bits, void* tmp,
                               void* stream_)
{
    if (n < 0 || key_bits < 0 || key_bits > 32) return SPLATRASTER_ERR_BAD_ARG;
    if (n == 0 || key_bits == 0) return SPLATRASTER_OK;
    return sort_in_place(false, n, keys, vals, key_bits, tmp, stream_);
}

int splatraster_debug_sort_pairs_k16(int64_t n, uint32_t* keys, uint32_t* vals, int32_t key_bits, void* tmp, void* stream_)
{
    if (n < 0 || key_bits < 0 || key_bits > 32 || !sort_keys16(n, key_bits)) return SPLATRASTER_ERR_BAD_ARG;
    return sort_in_place(true, n, keys, vals, key_bits, tmp, stream_);
}

int splatraster_debug_sort_path(int64_t n, int32_t key_bits, int32_t keys16)
{
    if (n < 0 || key_bits < 0 || key_bits > 32 || (keys16 && !sort_keys16(n, key_bits))) return -1;
    return sort_path(n, key_bits, keys16 != 0);
}

int splatraster_debug_scan_path(int64_t n) { return n < 0 ? -1 : scan_path(n); }

size_t splatraster_debug_scan_tmp_bytes(int64_t n) { return scan_tmp_bytes(n > 0 ? n : 0); }

int splatraster_debug_scan_u32(int64_t n, const uint32_t* in, const uint32_t* perm, uint32_t* out, uint64_t* total,
                               int32_t exclusive, uint32_t* span_owner, uint32_t span, uint32_t span_cap, void* tmp, void* stream_)
{
    if (n < 0) return SPLATRASTER_ERR_BAD_ARG;
    if (exclusive && (perm || in != out || span_owner)) return SPLATRASTER_ERR_BAD_ARG;
    if (span_owner && span == 0) return SPLATRASTER_ERR_BAD_ARG;
    if (n > 0 && (!in || !out || !tmp)) return SPLATRASTER_ERR_BAD_ARG;
    if (n > 0 && perm && in == out) return SPLATRASTER_ERR_BAD_ARG;   // the gather would read rows that other blocks overwrite
    if (n == 0 && !total) return SPLATRASTER_OK;
    {
        int st0 = lookback_error_init();
        if (st0) return st0;
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    uint32_t* total32 = reinterpret_cast<uint32_t*>(total);
    if (exclusive) return exclusive_scan_u32(n, out, total32, tmp, stream, false);
    return inclusive_scan_u32(n, in, perm, out, total32, tmp, stream, false, span_owner, span, span_cap);
}

int splatraster_timing_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_timing_mu);
    g_timing_mask = on ? 0xffffffffu : 0u;
    return SPLATRASTER_OK;
}

int splatraster_timing_select(uint32_t stage_mask)
{
    std::lock_guard<std::mutex> lk(g_timing_mu);
    g_timing_mask = stage_mask;
    return SPLATRASTER_OK;
}

int splatraster_timing_collect(double* ms, int64_t* counts)
{
    if (!ms || !counts) return SPLATRASTER_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(g_timing_mu);
    for (const StageRec& r : g_recs) {
        SR_HIP_CHECK(hipEventSynchronize(r.b));
        float t = 0.f;
        SR_HIP_CHECK(hipEventElapsedTime(&t, r.a, r.b));
        if (r.stage >= 0 && r.stage < SPLATRASTER_STAGE_COUNT) { ms[r.stage] += (double)t; counts[r.stage] += 1; }
        g_pool.push_back(r.a);
        g_pool.push_back(r.b);
    }
    g_recs.clear();
    return SPLATRASTER_OK;
}

}  // extern "C"
