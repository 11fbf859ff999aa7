// api.hip -- the extern "C" entry points of libgsr_hip.so (include/gsr.h): argument checks, workspace
// carving and the launch sequence of each stage.  No device memory is allocated here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "gsr_antialias.h"
#include "gsr_aux_grads.h"
#include "gsr_camera_grads.h"
#include "gsr_capacity.h"
#include "gsr_debug_layout.h"
#include "gsr_densify_stats.h"
#include "gsr_internal.h"

namespace {

#define HIP_TRY(expr)                                                                                                         \
    do {                                                                                                                      \
        hipError_t e_ = (expr);                                                                                               \
        if (e_ != hipSuccess) {                                                                                               \
            fprintf(stderr, "libgsr_hip: %s failed at %s:%d: %s\n", #expr, __FILE__, __LINE__, hipGetErrorString(e_));       \
            return GSR_E_HIP;                                                                                                 \
        }                                                                                                                     \
    } while (0)

struct Carver {
    char *p;
    size_t off = 0;
    explicit Carver(void *base) : p((char *)base) {}
    template <class T> T *take(size_t count)
    {
        T *r = (T *)(p ? p + off : nullptr);
        off += gsr_align(count * sizeof(T));
        return r;
    }
};

BinWs carve_bin(void *base, int64_t D)
{
    Carver c(base);
    BinWs w;
    w.hist = c.take<int32_t>(256 * ((size_t)gsr_radix_blocks(D) + 1));
    w.acc[0] = c.take<int32_t>(gsr_radix_acc_ints(D));
    w.acc[1] = c.take<int32_t>(gsr_radix_acc_ints(D));
    w.edge = c.take<int32_t>(3 * 256 * ((size_t)gsr_radix_blocks(D) + 1));
    w.tile_a = c.take<uint64_t>((size_t)D);
    w.tile_b = c.take<uint64_t>((size_t)D);
    w.bytes = c.off + 256;
    return w;
}

struct BwdWs {
    BlendRec *rec; // [N]
    GradRec *acc;  // [N]
    size_t bytes;
};
BwdWs carve_bwd(void *base, int64_t N)
{
    Carver c(base);
    BwdWs w;
    w.rec = c.take<BlendRec>((size_t)N);
    w.acc = c.take<GradRec>((size_t)N);
    w.bytes = c.off + 256;
    return w;
}

int check_scene_cam(const GsrScene *sc, const GsrCamera *cam)
{
    if (!sc || !cam) return GSR_E_NULL;
    if (sc->N < 0 || sc->N > 0x7FFFFFFFLL || cam->W <= 0 || cam->H <= 0 || sc->sh_degree < 0 || sc->sh_degree > 3) return GSR_E_DIMS;
    if ((cam->W + 15) / 16 > 65535 || (cam->H + 15) / 16 > 65535) return GSR_E_DIMS;
    if (sc->N > 0 && (!sc->means || !sc->scales || !sc->rotations || !sc->opacity || !sc->sh)) return GSR_E_NULL;
    if (!gsr_aligned16(sc->means) || !gsr_aligned16(sc->scales) || !gsr_aligned16(sc->rotations) || !gsr_aligned16(sc->opacity) ||
        !gsr_aligned16(sc->sh))
        return GSR_E_ALIGN;
    return GSR_OK;
}

CamK make_cam(const GsrCamera *c)
{
    CamK k;
    memcpy(k.view, c->view, sizeof(k.view));
    memcpy(k.proj, c->proj, sizeof(k.proj));
    memcpy(k.campos, c->campos, sizeof(k.campos));
    memcpy(k.bg, c->bg, sizeof(k.bg));
    k.tan_fovx = c->tan_fovx;
    k.tan_fovy = c->tan_fovy;
    k.focal_x = c->focal_x;
    k.focal_y = c->focal_y;
    k.W = c->W;
    k.H = c->H;
    k.grid_x = (c->W + GSR_TILE - 1) / GSR_TILE;
    k.grid_y = (c->H + GSR_TILE - 1) / GSR_TILE;
    return k;
}

bool geom_aligned(const GsrGeom *g)
{
    return gsr_aligned16(g->radii) && gsr_aligned16(g->tiles_touched) && gsr_aligned16(g->point_offsets) && gsr_aligned16(g->xy) &&
           gsr_aligned16(g->depths) && gsr_aligned16(g->cov3D) && gsr_aligned16(g->rgb) && gsr_aligned16(g->conic_opacity) &&
           gsr_aligned16(g->clamped_state) && gsr_aligned16(g->blend_records) && gsr_aligned16(g->sh_dir_grad);
}
bool grads_aligned(const GsrGrads *g)
{
    return gsr_aligned16(g->dL_dmean3D) && gsr_aligned16(g->dL_dscale) && gsr_aligned16(g->dL_drot) && gsr_aligned16(g->dL_dopacity) &&
           gsr_aligned16(g->dL_dshs) && gsr_aligned16(g->dL_dcolor) && gsr_aligned16(g->dL_dmean2D) && gsr_aligned16(g->dL_dconic) &&
           gsr_aligned16(g->dL_drgb);
}

bool geom_ok(const GsrGeom *g)
{
    // xy / conic_opacity / rgb may be absent when the caller takes them as columns of its own record buffer (GsrGeom.blend_records)
    const bool arrays = g && ((g->xy && g->rgb && g->conic_opacity) || g->blend_records);
    return arrays && g->radii && g->tiles_touched && g->point_offsets && g->depths && g->cov3D &&
           g->clamped_state;
}

// ---- the argument checks gsr_forward_render and gsr_forward_capacity share (every one before anything is enqueued) ----
int check_frame(const GsrScene *sc, const GsrCamera *cam, const GsrBinning *b, const GsrImage *img)
{
    if (int rc = check_scene_cam(sc, cam)) return rc;
    if (!b || !img || !img->image || !img->inv_depth || !img->final_T || !img->n_contrib || !b->ranges) return GSR_E_NULL;
    if (b->D < 0 || b->D > GSR_MAX_RENDERED) return GSR_E_OVERFLOW;
    return GSR_OK;
}
bool frame_aligned(const GsrGeom *g, const void *geom_ws, const void *bin_ws, const GsrBinning *b, const GsrImage *img)
{
    return (!g || geom_aligned(g)) && gsr_aligned16(geom_ws) && gsr_aligned16(bin_ws) && gsr_aligned16(b->point_list) && gsr_aligned16(b->ranges) &&
           gsr_aligned16(b->block_order) && gsr_aligned16(b->backward_ws) && gsr_aligned16(img->image) && gsr_aligned16(img->inv_depth) &&
           gsr_aligned16(img->final_T) && gsr_aligned16(img->n_contrib);
}
// both workspaces, sized for N Gaussians and D pairs (the capacity K in capacity mode)
int check_workspaces(int64_t N, int64_t D, const void *geom_ws, size_t geom_ws_bytes, const void *bin_ws, size_t bin_ws_bytes, const GsrCamera *cam)
{
    if (N > 0 && (!geom_ws || geom_ws_bytes < gsr_geom_workspace_bytes(N))) return GSR_E_WORKSPACE;
    if (N > 0 && (!bin_ws || bin_ws_bytes < gsr_binning_workspace_bytes(N, D, cam->W, cam->H))) return GSR_E_WORKSPACE;
    return GSR_OK;
}

// ---- stage timing (profiling aid) ----
// Process-wide by design (one benchmark drives it); `on` is atomic so the hot path pays one relaxed load when it is off,
// and every read-modify-write of the counters happens under g_timer_mu, so host threads driving different streams may
// all run with timing enabled (their samples interleave in the one record).
struct StageTimer {
    std::atomic<bool> on{false};
    int max_steps = 0, fwd_step = 0, bwd_step = 0; // recorded (sampled) steps so far
    int every = 1, fwd_calls = 0, bwd_calls = 0;    // record one call in `every`; event records cost ~3 us each
    hipEvent_t *ev = nullptr; // [max_steps][GSR_NSTAGES + 3]
    static constexpr int PER = GSR_NSTAGES + 3;
    hipEvent_t &at(int step, int k) { return ev[(size_t)step * PER + k]; }
} g_timer;
std::mutex g_timer_mu;
// event slots: 0..9 forward boundaries (before stage 0 .. after stage 8, with slot 3 = after sync),
// 10..13 backward boundaries
inline void mark(int step, int slot, hipStream_t s)
{
    if (step >= 0 && step < g_timer.max_steps) (void)hipEventRecord(g_timer.at(step, slot), s);
}
// which record (if any) a call samples into: -1 = not sampled.  The forward's two entry points share one record, as do
// the two halves of a split backward; the step is carried between them per host thread.
thread_local int t_fwd_record = -1, t_bwd_record = -1;
int timer_open(bool forward)
{
    if (!g_timer.on.load(std::memory_order_relaxed)) return -1;
    std::lock_guard<std::mutex> lk(g_timer_mu);
    if (!g_timer.on.load(std::memory_order_relaxed)) return -1;
    int &calls = forward ? g_timer.fwd_calls : g_timer.bwd_calls;
    int &step = forward ? g_timer.fwd_step : g_timer.bwd_step;
    if (g_timer.every == 0) return -1; // paused: the events exist, nothing is recorded
    if ((calls++ % g_timer.every) != 0 || step >= g_timer.max_steps) return -1;
    return step++;
}

// ---- readback slots for D ----
// 4 bytes of pinned host memory + an event per call IN FLIGHT: gsr_forward_count leases a slot of its device from this
// pool and returns it before it returns, so two host threads counting on the same device never share a word, and a
// thread that exits leaks nothing (slots are created on demand and kept for the life of the process).  With the pinned
// word the host can wait for D alone while the GPU already runs the depth sort, which does not depend on D.
struct Readback {
    int dev = -1;
    bool busy = false;
    int32_t *pinned = nullptr;
    hipEvent_t ev = nullptr;
};
std::mutex g_rb_mu;
std::vector<Readback *> g_rb_pool;
Readback *readback_acquire()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_rb_mu);
    for (Readback *r : g_rb_pool)
        if (r->dev == dev && !r->busy) {
            r->busy = true;
            return r;
        }
    Readback *r = new Readback;
    r->dev = dev;
    if (hipHostMalloc((void **)&r->pinned, 256, hipHostMallocMapped) != hipSuccess ||       // device-writable
        hipEventCreateWithFlags(&r->ev, hipEventDisableTiming) != hipSuccess) {
        if (r->pinned) (void)hipHostFree(r->pinned);
        delete r;
        return nullptr;
    }
    r->busy = true;
    g_rb_pool.push_back(r);
    return r;
}
struct ReadbackLease {
    Readback *r;
    ReadbackLease() : r(readback_acquire()) {}
    ~ReadbackLease()
    {
        if (!r) return;
        std::lock_guard<std::mutex> lk(g_rb_mu);
        r->busy = false;
    }
};

// ---- the count gsr_forward_count returned, per geom workspace ----
// gsr_forward_render trusts nothing about GsrBinning.D that it can check: the expansion, both partition passes and the
// range scan are sized by D, and a D that is not the count of the depth-sorted items in geom_ws would make them write out
// of bounds (too large) or truncate the list silently (too small).  The true count never leaves the host, so it is
// remembered here, keyed by (device, geom_ws); a small LRU table, guarded by a mutex.
struct CountNote {
    int dev;
    const void *ws;
    int64_t N, D;
    uint64_t stamp;
    int depth_passes; // how many depth-sort passes the last frame counted in this workspace needed: the next frame's launch guess
};
std::mutex g_note_mu;
std::vector<CountNote> g_notes;
uint64_t g_note_clock = 0;
constexpr size_t MAX_NOTES = 256;
void note_count(const void *ws, int64_t N, int64_t D, int depth_passes)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_note_mu);
    CountNote *slot = nullptr;
    for (CountNote &c : g_notes)
        if (c.dev == dev && c.ws == ws) slot = &c;
    if (!slot) {
        if (g_notes.size() < MAX_NOTES) {
            g_notes.push_back(CountNote{});
            slot = &g_notes.back();
        } else {
            slot = &*std::min_element(g_notes.begin(), g_notes.end(), [](const CountNote &a, const CountNote &b) { return a.stamp < b.stamp; });
        }
    }
    *slot = CountNote{dev, ws, N, D, ++g_note_clock, depth_passes};
}
// the depth-sort launch guess for a workspace: what its last frame needed, four if it has none
int depth_pass_guess(const void *ws)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_note_mu);
    for (CountNote &c : g_notes)
        if (c.dev == dev && c.ws == ws) return c.depth_passes >= 1 && c.depth_passes <= 4 ? c.depth_passes : 4;
    return 4;
}
// 1 = matches, 0 = mismatch, -1 = this workspace has no recorded count
int check_count(const void *ws, int64_t N, int64_t D)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_note_mu);
    for (CountNote &c : g_notes)
        if (c.dev == dev && c.ws == ws) {
            c.stamp = ++g_note_clock;
            return (c.N == N && c.D == D) ? 1 : 0;
        }
    return -1;
}

bool fwd_order_wanted(int tiles) { return tiles > 0 && tiles <= GSR_FO_MAX_TILES && !(gsr_debug_flags & 8192); } // GSR_DEBUG bit 13: row-major (tests)

std::once_flag g_tuning_once;
void read_tuning()
{
    std::call_once(g_tuning_once, [] {
        if (const char *e = getenv("GSR_DEBUG")) gsr_debug_flags = atoi(e) & GSR_DEBUG_ALLOWED;
        if (const char *e = getenv("GSR_BWD_BLOCK")) {
            const int px = atoi(e);
            gsr_bwd_block = (px == 32 || px == 64) ? px : 0;
        }
    });
}

// The front half of the forward, shared by gsr_forward_count and gsr_forward_capacity: preprocess, the id-order scan and the
// depth sort's last `depth_passes` passes.  With a readback slot the scan's last wave stores D, and its control workgroups the
// depth extremes, straight into the pinned words, and rb->ev marks the scan's end: work that does not need D goes out before the
// host waits for it.  Without one D stays in point_offsets[N-1].
int enqueue_depth_stage(const GsrScene *scene, const CamK &cam, const GsrGeom *geom, const GeomWs &ws, Readback *rb, int depth_passes, hipStream_t s,
                        int st, float *aa_scale)
{
    mark(st, 0, s);
    HIP_TRY(gsr_launch_preprocess(*scene, cam, *geom, ws, s, fwd_order_wanted(cam.grid_x * cam.grid_y), aa_scale));
    mark(st, 1, s);
    HIP_TRY(gsr_launch_id_scan(geom->tiles_touched, geom->point_offsets, ws, scene->N, rb ? rb->pinned : nullptr, s));
    mark(st, 2, s);
    if (rb) HIP_TRY(hipEventRecord(rb->ev, s));
    HIP_TRY(gsr_launch_depth_sort(ws, scene->N, cam.grid_x, cam.grid_y, depth_passes, s));
    return GSR_OK;
}

} // namespace

GeomWs gsr_carve_geom(void *base, int64_t N)
{
    Carver c(base);
    GeomWs w;
    w.rec = c.take<BlendRec>((size_t)N); // FIRST: a caller may hand the start of geom_ws back to gsr_backward as GsrGeom.blend_records
    w.rect = c.take<TileRect>((size_t)N);
    w.depth_item = c.take<uint64_t>((size_t)N);
    w.sort_tmp = c.take<uint64_t>((size_t)N);
    w.id_sorted = c.take<uint32_t>((size_t)N);
    w.blk_minmax = c.take<uint32_t>(4 * (size_t)gsr_div_up(N, 256) + 4);
    w.depth_ctl = w.blk_minmax ? w.blk_minmax + 4 * (size_t)gsr_div_up(N, 256) : nullptr; // the uint4 behind the last block's (preprocess clears it)
    w.rect_sorted = c.take<TileRect>((size_t)N);
    w.cnt_sorted = c.take<int32_t>((size_t)N);
    w.scan_tmp = c.take<int32_t>((size_t)gsr_div_up(N, 256) + 4);
    w.hist = c.take<int32_t>(256 * ((size_t)gsr_radix_blocks(N) + 1));
    w.acc[0] = c.take<int32_t>(3 * gsr_radix_acc_ints(N)); // the accumulators of both pass parities and of the first active pass, contiguous: preprocess clears them in one go
    w.acc[1] = w.acc[0] ? w.acc[0] + gsr_radix_acc_ints(N) : nullptr;
    w.acc_first = w.acc[0] ? w.acc[0] + 2 * gsr_radix_acc_ints(N) : nullptr;
    w.sum4096 = c.take<int32_t>((size_t)gsr_div_up(N, 4096) + 4);
    w.fwd_cost = c.take<int32_t>(4 * (size_t)GSR_FO_MAX_TILES); // (behind everything else: they move when N changes, and the order
    w.fwd_order = c.take<int32_t>((size_t)GSR_FO_MAX_TILES);    // made from a moved -- i.e. arbitrary -- cost table is still a permutation)
    w.bytes = c.off + 256;
    return w;
}

// gsr_forward_count and (include/gsr_antialias.h) gsr_forward_count_aa: aa_scale = NULL is the classic call
static int forward_count(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, void *geom_ws, size_t geom_ws_bytes,
                         int64_t *num_rendered, float *aa_scale, void *stream);
static int forward_capacity(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                            void *geom_ws, size_t geom_ws_bytes, void *bin_ws, size_t bin_ws_bytes, int64_t shape_hint, float *aa_scale, void *stream);

extern "C" {

int gsr_abi_version(void) { return GSR_ABI_VERSION; }

int gsr_build_flags(void)
{
#ifdef GSR_ABLATE
    return GSR_BUILD_ABLATE;
#else
    return 0;
#endif
}

const char *gsr_strerror(int code)
{
    switch (code) {
    case GSR_OK: return "ok";
    case GSR_E_NULL: return "required pointer is null";
    case GSR_E_DIMS: return "invalid dimensions or SH degree";
    case GSR_E_OVERFLOW: return "Number of rendered points exceeds the maximum supported (2^30)";
    case GSR_E_WORKSPACE: return "workspace missing or too small";
    case GSR_E_HIP: return "HIP runtime error (see stderr)";
    case GSR_E_CAPACITY: return "GsrBinning.D is not the count gsr_forward_count returned for this geom workspace";
    case GSR_E_ALIGN: return "an array pointer is not 16-byte aligned";
    default: return "unknown error";
    }
}

size_t gsr_geom_workspace_bytes(int64_t N) { return gsr_carve_geom(nullptr, N < 0 ? 0 : N).bytes; }
size_t gsr_binning_workspace_bytes(int64_t, int64_t D, int32_t, int32_t) { return carve_bin(nullptr, D < 0 ? 0 : D).bytes; }
size_t gsr_backward_workspace_bytes(int64_t N, int64_t, int32_t, int32_t) { return carve_bwd(nullptr, N < 0 ? 0 : N).bytes; }
size_t gsr_backward_accumulators_offset(int64_t N) { return gsr_align((size_t)(N < 0 ? 0 : N) * sizeof(BlendRec)); } // carve_bwd: the records come first
// (include/gsr_debug_layout.h) the two tile-order tables inside the geom workspace, from the carve itself
int gsr_fwd_order_tables_offset(int64_t N, size_t *fwd_cost_offset, size_t *fwd_order_offset)
{
    static_assert(GSR_FWD_ORDER_MAX_TILES == GSR_FO_MAX_TILES, "the header's table size is the kernels'");
    if (!fwd_cost_offset || !fwd_order_offset) return GSR_E_NULL;
    if (N < 0 || N > 0x7FFFFFFFLL) return GSR_E_DIMS;
    static char base[1]; // carved, never dereferenced
    const GeomWs w = gsr_carve_geom(base, N);
    *fwd_cost_offset = (size_t)((const char *)w.fwd_cost - base);
    *fwd_order_offset = (size_t)((const char *)w.fwd_order - base);
    return GSR_OK;
}
size_t gsr_block_order_ints(int32_t W, int32_t H)
{
    if (W <= 0 || H <= 0) return 0;
    const int64_t tiles = (int64_t)((W + GSR_TILE - 1) / GSR_TILE) * ((H + GSR_TILE - 1) / GSR_TILE);
    // images of more than GSR_BO_MAX_TILES tiles are never filed (gsr_internal.h): only the header (counters + the `filed` flag) is touched
    return tiles > GSR_BO_MAX_TILES ? (size_t)GSR_BO_HEADER : gsr_bo_ints((int)tiles);
}

int gsr_forward_count(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, void *geom_ws, size_t geom_ws_bytes,
                      int64_t *num_rendered, void *stream)
{
    return forward_count(scene, camera, geom, geom_ws, geom_ws_bytes, num_rendered, nullptr, stream);
}

int gsr_forward_count_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, void *geom_ws, size_t geom_ws_bytes,
                         int64_t *num_rendered, float *aa_scale, void *stream)
{
    return forward_count(scene, camera, geom, geom_ws, geom_ws_bytes, num_rendered, aa_scale, stream);
}

} // extern "C"

static int forward_count(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, void *geom_ws, size_t geom_ws_bytes,
                         int64_t *num_rendered, float *aa_scale, void *stream)
{
    read_tuning();
    if (int rc = check_scene_cam(scene, camera)) return rc;
    if (!num_rendered) return GSR_E_NULL;
    *num_rendered = 0;
    const int64_t N = scene->N;
    if (N == 0) return GSR_OK; // reference behaviour undefined (quirk Q10): empty buffers, D = 0
    if (!geom_ok(geom)) return GSR_E_NULL;
    if (!geom_aligned(geom) || !gsr_aligned16(geom_ws) || !gsr_aligned16(aa_scale)) return GSR_E_ALIGN;
    if (!geom_ws || geom_ws_bytes < gsr_geom_workspace_bytes(N)) return GSR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const CamK cam = make_cam(camera);
    const GeomWs ws = gsr_carve_geom(geom_ws, N);
    ReadbackLease lease;
    Readback *rb = lease.r;
    if (!rb) return GSR_E_HIP;
    const int st = t_fwd_record = timer_open(true);
    // How many of the depth sort's four passes this frame needs is decided on the device (DepthCtl); the host launches as many as
    // the previous frame in this workspace needed (its guess; four the first time).  If the guess turns out too low the launched
    // passes leave the data alone and all four are launched once the readback has said so.
    const int guess = (gsr_debug_flags & 256) ? 4 : depth_pass_guess(geom_ws);
    if (int rc = enqueue_depth_stage(scene, cam, geom, ws, rb, guess, s, st, aa_scale)) return rc;
    HIP_TRY(hipEventSynchronize(rb->ev)); // D (and the pass count) are on the host; the GPU keeps sorting
    const int32_t last = *rb->pinned;
    const int needed = gsr_depth_passes_needed(rb->pinned, N);
    if (needed > guess && !gsr_small_depth_path(N)) HIP_TRY(gsr_launch_depth_sort(ws, N, cam.grid_x, cam.grid_y, 4, s));
    mark(st, 3, s);
    // (the depth-order offsets -- the exclusive scan of those counts -- are made by gsr_forward_render, next to their one reader,
    // the expansion)
    *num_rendered = (int64_t)last;
    if (last < 0 || (int64_t)last > GSR_MAX_RENDERED) return GSR_E_OVERFLOW;
    note_count(geom_ws, N, (int64_t)last, needed);
    return GSR_OK;
}

namespace {

// what gsr_forward_render enqueues for a frame without pairs: zeros, not background (quirk Q10), and the promised clear of the
// backward workspace's accumulators (its alignment was checked by the caller)
int empty_frame(const GsrBinning *binning, const GsrImage *image, int64_t N, int tiles, size_t P, hipStream_t s)
{
    HIP_TRY(hipMemsetAsync(binning->ranges, 0, sizeof(int32_t) * 2 * tiles, s));
    HIP_TRY(hipMemsetAsync(image->image, 0, P * 3 * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(image->inv_depth, 0, P * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(image->final_T, 0, P * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(image->n_contrib, 0, P * sizeof(int32_t), s));
    // the accumulator clear of GsrBinning.backward_ws is promised whenever the workspace is handed over, blend or no blend
    if (binning->backward_ws && N > 0) HIP_TRY(hipMemsetAsync(carve_bwd(binning->backward_ws, N).acc, 0, sizeof(GradRec) * (size_t)N, s));
    return GSR_OK;
}

// The D-dependent half of the forward: expansion, tile partition, blend.  Sized path: d_count = NULL and D is the count
// gsr_forward_count returned.  Capacity mode (gsr_forward_capacity): D is the capacity K, which sizes every launch and every
// buffer, the kernels read the real count at d_count, and `shape_D` (the caller's hint) stands in for the count in the one
// choice the host still makes from it, the block filing for the backward's 8x4 blocks.
int enqueue_render(const GsrScene *scene, const CamK &cam, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                   const GeomWs &gw, const BinWs &bw, const int32_t *d_count, int64_t shape_D, hipStream_t s, int st)
{
    const int64_t N = scene->N, D = binning->D;
    const int tiles = cam.grid_x * cam.grid_y;
    if (!d_count) shape_D = D;
    mark(st, 4, s); // (stage 3 -> 4: the host between the two calls -- the wait for D, the caller's allocations)
    // 3. expansion of the depth-sorted Gaussians (gsr_forward_count) to tile items, 4. their stable partition by tile id, whose
    //    last pass writes point_list and the tile ranges (scan_sort.hip)
    const TilePlan plan = gsr_tile_plan(N, tiles);
    // the block order (forward -> backward scratch): header cleared here; filed by the blend below unless the image is large
    int32_t *order = binning->block_masks ? binning->block_order : nullptr;
    // (and not for a frame whose backward will take 8x8 blocks, which run in band order: the `filed` flag then stays 0)
    const bool file_order = order && tiles <= GSR_BO_MAX_TILES && gsr_bwd_block_px(N, shape_D, tiles) == 32;
    // the forward blend's tiles by last frame's cost classes (gsr_internal.h "forward tile order"): the table was made by the spare
    // workgroup of this frame's preprocess (gsr_forward_count, same condition), so it is never stale or foreign
    const bool use_fwd_order = fwd_order_wanted(tiles);
    // one offset per 256 depth-sorted Gaussians (stage "depth_scan"), then one workgroup per radix block of the item array,
    // which also leaves the first partition pass's block histograms
    HIP_TRY(gsr_launch_depth_block_offsets(gw, N, binning->ranges, 2 * tiles, bw.acc[0], (int)gsr_radix_acc_ints(D), order, order ? GSR_BO_HEADER : 0,
                                           file_order ? 1 : 0, s));
    mark(st, 5, s);
    HIP_TRY(gsr_launch_expand_blocks(plan, gw, bw, N, cam.grid_x, D, d_count, s));
    mark(st, 6, s);
    HIP_TRY(gsr_launch_tile_partition(plan, bw, binning->point_list, binning->ranges, D, d_count, s));
    mark(st, 7, s);
    mark(st, 8, s); // (stage slot "ranges": nothing left in it)
    // 6. blend
    // the backward's accumulator records are cleared by the blend kernel's spare workgroups when the caller hands its backward
    // workspace over (GsrBinning.backward_ws); it then tells gsr_backward so (GsrBinning.backward_ws_cleared)
    void *clear = binning->backward_ws ? carve_bwd(binning->backward_ws, N).acc : nullptr;
    const size_t clear_bytes = clear ? sizeof(GradRec) * (size_t)N : 0;
    HIP_TRY(gsr_launch_blend_forward(cam, binning->ranges, binning->point_list, geom->blend_records ? (const BlendRec *)geom->blend_records : gw.rec, *image, binning->block_masks, file_order ? order : nullptr,
                                     clear, clear_bytes, s, use_fwd_order ? gw.fwd_order : nullptr, tiles <= GSR_FO_MAX_TILES ? gw.fwd_cost : nullptr,
                                     d_count, D));
    mark(st, 9, s);
    return GSR_OK;
}

} // namespace

extern "C" {

int gsr_forward_render(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning,
                       const GsrImage *image, void *geom_ws, size_t geom_ws_bytes, void *bin_ws, size_t bin_ws_bytes, void *stream)
{
    read_tuning();
    if (int rc = check_frame(scene, camera, binning, image)) return rc;
    const int64_t N = scene->N, D = binning->D;
    hipStream_t s = (hipStream_t)stream;
    const CamK cam = make_cam(camera);
    if (D == 0 || N == 0) { // reference skips the blend: zeros, not background (forward.py:830, quirk Q10)
        if (!gsr_aligned16(binning->backward_ws)) return GSR_E_ALIGN;
        t_fwd_record = -1;  // a sampled record that ends here stays incomplete and is dropped by gsr_stage_times
        return empty_frame(binning, image, N, cam.grid_x * cam.grid_y, (size_t)cam.W * cam.H, s);
    }
    if (!geom_ok(geom) || !binning->point_list) return GSR_E_NULL;
    if (!frame_aligned(geom, geom_ws, bin_ws, binning, image)) return GSR_E_ALIGN;
    if (int rc = check_workspaces(N, D, geom_ws, geom_ws_bytes, bin_ws, bin_ws_bytes, camera)) return rc;
    // D must be the count gsr_forward_count returned for the items now in geom_ws (see CountNote above)
    if (check_count(geom_ws, N, D) != 1) return GSR_E_CAPACITY;
    const int st = t_fwd_record;
    t_fwd_record = -1;
    return enqueue_render(scene, cam, geom, binning, image, gsr_carve_geom(geom_ws, N), carve_bin(bin_ws, D), nullptr, D, s, st);
}

int gsr_forward_capacity(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                         void *geom_ws, size_t geom_ws_bytes, void *bin_ws, size_t bin_ws_bytes, int64_t shape_hint, void *stream)
{
    return forward_capacity(scene, camera, geom, binning, image, geom_ws, geom_ws_bytes, bin_ws, bin_ws_bytes, shape_hint, nullptr, stream);
}

int gsr_forward_capacity_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                            void *geom_ws, size_t geom_ws_bytes, void *bin_ws, size_t bin_ws_bytes, int64_t shape_hint, float *aa_scale,
                            void *stream)
{
    return forward_capacity(scene, camera, geom, binning, image, geom_ws, geom_ws_bytes, bin_ws, bin_ws_bytes, shape_hint, aa_scale, stream);
}

} // extern "C"

static int forward_capacity(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                            void *geom_ws, size_t geom_ws_bytes, void *bin_ws, size_t bin_ws_bytes, int64_t shape_hint, float *aa_scale, void *stream)
{
    read_tuning();
    // every argument is checked before anything is enqueued (include/gsr_capacity.h)
    if (int rc = check_frame(scene, camera, binning, image)) return rc;
    const int64_t N = scene->N, K = binning->D;
    if (shape_hint < 0 || shape_hint > GSR_MAX_RENDERED) return GSR_E_OVERFLOW;
    if (K > 0 && !binning->point_list) return GSR_E_NULL;
    if (N > 0 && !geom_ok(geom)) return GSR_E_NULL;
    if (!frame_aligned(geom, geom_ws, bin_ws, binning, image) || !gsr_aligned16(binning->block_masks) || !gsr_aligned16(aa_scale)) return GSR_E_ALIGN;
    if (int rc = check_workspaces(N, K, geom_ws, geom_ws_bytes, bin_ws, bin_ws_bytes, camera)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const CamK cam = make_cam(camera);
    if (N == 0) return empty_frame(binning, image, N, cam.grid_x * cam.grid_y, (size_t)cam.W * cam.H, s);
    const GeomWs gw = gsr_carve_geom(geom_ws, N);
    const int st = timer_open(true);
    // All four depth passes: with no readback there is no guess to check, and the device plan (DepthCtl) makes the passes this
    // frame does not need return at once -- one or two launches of early-exit workgroups, a few microseconds of GPU time.
    // D stays in point_offsets[N-1], where every D-dependent kernel below reads it.
    if (int rc = enqueue_depth_stage(scene, cam, geom, gw, nullptr, 4, s, st, aa_scale)) return rc;
    mark(st, 3, s);
    return enqueue_render(scene, cam, geom, binning, image, gw, carve_bin(bin_ws, K), geom->point_offsets + (N - 1), shape_hint, s, st);
}

namespace {

// ---- the backward: every exported call below fills one BwdCall.  check_bwd refuses it or passes it, whole, before anything is
// enqueued; the two enqueue halves take a checked call.  (include/gsr.h, gsr_aux_grads.h, gsr_densify_stats.h) ----
enum { BWD_BLEND = 1, BWD_GEOM = 2 };
struct BwdCall {
    const GsrScene *scene;
    const GsrCamera *camera;
    const GsrGeom *geom;
    // blend half (accumulator clear, record (re)pack, blend backward, optional view payload)
    const GsrBinning *binning;
    const GsrImage *image;
    GsrPixelGrads pix; // at least one; dL_dinv_depth or dL_dalpha selects the AUX blend kernels
    float *payload;    // optional
    // geom half (the four per-Gaussian kernels of backward_preprocess, fused)
    const GsrGrads *grads;
    float *dL_dinv_depths; // optional: GradRec slot 11, packed
    void *ws;
    size_t ws_bytes;
    uint32_t flags; // GSR_BWD_ABSGRAD: the ABS blend kernels
    int halves;     // BWD_BLEND | BWD_GEOM
    bool geom_aux;  // the AUX per-Gaussian kernel whatever the pixel gradients are (gsr_backward_geom_aux)
    void *stream;
    const float *aa_scale = nullptr; // the AA per-Gaussian kernel (include/gsr_antialias.h): the forward's rho; NULL = classic
};
GsrPixelGrads pix_of(const GsrPixelGrads *pg) { return pg ? *pg : GsrPixelGrads{}; }

// the pieces gsr_backward_camera checks too
bool geom_core(const GsrGeom *g) { return g && g->radii && g->clamped_state; } // (cov3D may be NULL: recomputed, gsr.h GsrGeom)
bool bwd_ws_fits(const void *ws, size_t ws_bytes, const GsrScene *sc, const GsrCamera *cam)
{
    return ws && ws_bytes >= gsr_backward_workspace_bytes(sc->N, 0, cam->W, cam->H); // (the size does not depend on D)
}

// Every argument of the halves the call runs, in the order NULL, ALIGN, OVERFLOW, WORKSPACE; nothing is enqueued.  GSR_OK with
// N == 0 means there is nothing to do (and nothing else was looked at).
int check_bwd(const BwdCall &c)
{
    if (c.flags & ~GSR_BWD_ABSGRAD) return GSR_E_DIMS;
    if (int rc = check_scene_cam(c.scene, c.camera)) return rc;
    if (c.scene->N == 0) return GSR_OK;
    const GsrGeom *g = c.geom;
    const GsrGrads *gr = c.grads;
    const GsrBinning *b = c.binning;
    const GsrImage *img = c.image;
    const bool blend = c.halves & BWD_BLEND, per_gaussian = c.halves & BWD_GEOM;
    // dL_dshs and dL_drgb may both be NULL in a geom half alone: the payload was taken from the blend half and the SH gradient is
    // rebuilt later (dL_dcolor / dL_dmean2D / dL_dconic may each be NULL: columns of the accumulator records in `ws`, gsr.h GsrGrads)
    if (per_gaussian && (!gr || !gr->dL_dmean3D || !gr->dL_dscale || !gr->dL_drot || !gr->dL_dopacity || (blend && !gr->dL_dshs && !gr->dL_drgb)))
        return GSR_E_NULL;
    if (!geom_core(g)) return GSR_E_NULL;
    if (blend) {
        if (!g->blend_records && (!g->xy || !g->rgb || !g->conic_opacity)) return GSR_E_NULL; // the records, or what they are rebuilt from
        if (!b || !img || (!c.pix.dL_dpixels && !c.pix.dL_dinv_depth && !c.pix.dL_dalpha)) return GSR_E_NULL;
        if (c.pix.dL_dinv_depth && !g->blend_records && !g->depths) return GSR_E_NULL; // a re-pack without depths would carry invd = 0
    }
    if (!geom_aligned(g) || !gsr_aligned16(c.ws)) return GSR_E_ALIGN;
    if (per_gaussian && (!grads_aligned(gr) || !gsr_aligned16(c.dL_dinv_depths) || !gsr_aligned16(c.aa_scale))) return GSR_E_ALIGN;
    if (blend) {
        if (!gsr_aligned16(b->point_list) || !gsr_aligned16(b->ranges) || !gsr_aligned16(b->block_masks) || !gsr_aligned16(b->block_order) ||
            !gsr_aligned16(img->final_T) || !gsr_aligned16(img->n_contrib) || !gsr_aligned16(c.pix.dL_dpixels) || !gsr_aligned16(c.payload) ||
            !gsr_aligned16(c.pix.dL_dinv_depth) || !gsr_aligned16(c.pix.dL_dalpha))
            return GSR_E_ALIGN;
        if (b->D < 0 || b->D > GSR_MAX_RENDERED) return GSR_E_OVERFLOW;
        if (b->D > 0 && (!b->point_list || !b->ranges || !img->final_T || !img->n_contrib)) return GSR_E_NULL;
    }
    return bwd_ws_fits(c.ws, c.ws_bytes, c.scene, c.camera) ? GSR_OK : GSR_E_WORKSPACE;
}

int enqueue_bwd_blend(const BwdCall &c, const CamK &cam, const BwdWs &bw, hipStream_t s, int st)
{
    const GsrBinning *b = c.binning;
    const int64_t N = c.scene->N, D = b->D;
    mark(st, 10, s);
    // (unless gsr_forward_render cleared this very workspace's accumulators in its blend kernel and nothing has used it since)
    if (!(b->backward_ws_cleared && b->backward_ws == c.ws)) HIP_TRY(hipMemsetAsync(bw.acc, 0, sizeof(GradRec) * (size_t)N, s));
    const BlendRec *records = (const BlendRec *)c.geom->blend_records;
    if (D > 0 && !records) {
        HIP_TRY(gsr_launch_pack_records(*c.geom, bw.rec, N, s));
        records = bw.rec;
    }
    mark(st, 11, s);
    if (D > 0) HIP_TRY(gsr_launch_blend_backward_splat(cam, b->ranges, b->point_list, records, *c.image, c.pix.dL_dpixels, b->block_masks,
                                                       b->block_masks ? b->block_order : nullptr, bw.acc, N, D, s, c.pix.dL_dinv_depth || c.pix.dL_dalpha,
                                                       c.pix.dL_dinv_depth, c.pix.dL_dalpha, (c.flags & GSR_BWD_ABSGRAD) != 0));
    mark(st, 12, s);
    if (c.payload) HIP_TRY(gsr_launch_view_payload(*c.scene, cam, *c.geom, bw.acc, c.payload, s));
    return GSR_OK;
}

int enqueue_bwd_geom(const BwdCall &c, const CamK &cam, const BwdWs &bw, hipStream_t s, int st)
{
    const bool aux = c.geom_aux || c.pix.dL_dinv_depth || c.pix.dL_dalpha || c.dL_dinv_depths;
    HIP_TRY(gsr_launch_geom_backward(*c.scene, cam, *c.geom, bw.acc, *c.grads, s, aux, c.aa_scale));
    if (c.dL_dinv_depths) // column 11 of the accumulator records (gsr_gradrec_slot(9)), packed
        HIP_TRY(hipMemcpy2DAsync(c.dL_dinv_depths, sizeof(float), &bw.acc[0].f[gsr_gradrec_slot(9)], sizeof(GradRec), sizeof(float),
                                 (size_t)c.scene->N, hipMemcpyDeviceToDevice, s));
    mark(st, 13, s);
    return GSR_OK;
}

int run_bwd(const BwdCall &c)
{
    read_tuning();
    if (int rc = check_bwd(c)) return rc;
    if (c.scene->N == 0) return GSR_OK;
    // stage events: a whole call opens its own record; the two halves of a split one share a record, opened by the blend half
    // and closed by the geom half
    const int st = (c.halves & BWD_BLEND) ? timer_open(false) : t_bwd_record;
    if (c.halves != (BWD_BLEND | BWD_GEOM)) t_bwd_record = (c.halves & BWD_BLEND) ? st : -1;
    hipStream_t s = (hipStream_t)c.stream;
    const CamK cam = make_cam(c.camera);
    const BwdWs bw = carve_bwd(c.ws, c.scene->N);
    if (int rc = (c.halves & BWD_BLEND) ? enqueue_bwd_blend(c, cam, bw, s, st) : GSR_OK) return rc;
    return (c.halves & BWD_GEOM) ? enqueue_bwd_geom(c, cam, bw, s, st) : GSR_OK;
}

} // namespace

extern "C" {

// (include/gsr_densify_stats.h) the whole call and its blend half: every other whole or blend call below is one of these two
int gsr_backward_flags(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                       const GsrPixelGrads *pixel_grads, const GsrGrads *grads, float *dL_dinv_depths, void *ws, size_t ws_bytes, uint32_t flags,
                       void *stream)
{
    return run_bwd({scene, camera, geom, binning, image, pix_of(pixel_grads), nullptr, grads, dL_dinv_depths, ws, ws_bytes, flags,
                    BWD_BLEND | BWD_GEOM, false, stream});
}

int gsr_backward_blend_flags(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                             const GsrPixelGrads *pixel_grads, float *payload, void *ws, size_t ws_bytes, uint32_t flags, void *stream)
{
    return run_bwd({scene, camera, geom, binning, image, pix_of(pixel_grads), payload, nullptr, nullptr, ws, ws_bytes, flags, BWD_BLEND, false, stream});
}

// (include/gsr_aux_grads.h) with neither auxiliary gradient and no dL_dinv_depths the whole call runs gsr_backward's kernels, bit for bit
int gsr_backward_aux(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                     const GsrPixelGrads *pixel_grads, const GsrGrads *grads, float *dL_dinv_depths, void *ws, size_t ws_bytes, void *stream)
{
    return gsr_backward_flags(scene, camera, geom, binning, image, pixel_grads, grads, dL_dinv_depths, ws, ws_bytes, 0, stream);
}

int gsr_backward_blend_aux(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                           const GsrPixelGrads *pixel_grads, float *payload, void *ws, size_t ws_bytes, void *stream)
{
    return gsr_backward_blend_flags(scene, camera, geom, binning, image, pixel_grads, payload, ws, ws_bytes, 0, stream);
}

int gsr_backward_geom_aux(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrGrads *grads, float *dL_dinv_depths,
                          void *ws, size_t ws_bytes, void *stream)
{
    return run_bwd({scene, camera, geom, nullptr, nullptr, {}, nullptr, grads, dL_dinv_depths, ws, ws_bytes, 0, BWD_GEOM, true, stream});
}

// (include/gsr_antialias.h) the whole call and the geom half of an antialiased frame; aa_scale = NULL is the call above
int gsr_backward_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                    const GsrPixelGrads *pixel_grads, const GsrGrads *grads, float *dL_dinv_depths, void *ws, size_t ws_bytes, uint32_t flags,
                    const float *aa_scale, void *stream)
{
    return run_bwd({scene, camera, geom, binning, image, pix_of(pixel_grads), nullptr, grads, dL_dinv_depths, ws, ws_bytes, flags,
                    BWD_BLEND | BWD_GEOM, false, stream, aa_scale});
}

int gsr_backward_geom_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrGrads *grads, float *dL_dinv_depths,
                         void *ws, size_t ws_bytes, const float *aa_scale, void *stream)
{
    return run_bwd({scene, camera, geom, nullptr, nullptr, {}, nullptr, grads, dL_dinv_depths, ws, ws_bytes, 0, BWD_GEOM, true, stream, aa_scale});
}

// (include/gsr.h) the same three with the colour image's gradient alone
int gsr_backward(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                 const float *dL_dpixels, const GsrGrads *grads, void *ws, size_t ws_bytes, void *stream)
{
    const GsrPixelGrads pg{dL_dpixels, nullptr, nullptr};
    return gsr_backward_flags(scene, camera, geom, binning, image, &pg, grads, nullptr, ws, ws_bytes, 0, stream);
}

int gsr_backward_blend(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning, const GsrImage *image,
                       const float *dL_dpixels, float *payload, void *ws, size_t ws_bytes, void *stream)
{
    const GsrPixelGrads pg{dL_dpixels, nullptr, nullptr};
    return gsr_backward_blend_flags(scene, camera, geom, binning, image, &pg, payload, ws, ws_bytes, 0, stream);
}

int gsr_backward_geom(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrGrads *grads, void *ws, size_t ws_bytes,
                      void *stream)
{
    return run_bwd({scene, camera, geom, nullptr, nullptr, {}, nullptr, grads, nullptr, ws, ws_bytes, 0, BWD_GEOM, false, stream});
}

// ---- include/gsr_camera_grads.h: dL/d(view, proj, campos) from the accumulators a backward left in `ws` ----
size_t gsr_backward_camera_scratch_bytes(int64_t N) { return gsr_camera_scratch_bytes(N); }

int gsr_backward_camera(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, float *dL_dcamera, const void *ws, size_t ws_bytes,
                        void *scratch, size_t scratch_bytes, void *stream)
{
    return gsr_backward_camera_aa(scene, camera, geom, dL_dcamera, ws, ws_bytes, scratch, scratch_bytes, nullptr, stream);
}

// (include/gsr_antialias.h) aa_scale = NULL is the call above
int gsr_backward_camera_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, float *dL_dcamera, const void *ws, size_t ws_bytes,
                           void *scratch, size_t scratch_bytes, const float *aa_scale, void *stream)
{
    read_tuning();
    if (int rc = check_scene_cam(scene, camera)) return rc;
    if (!dL_dcamera) return GSR_E_NULL;
    if (!gsr_aligned16(dL_dcamera) || !gsr_aligned16(ws) || !gsr_aligned16(scratch) || !gsr_aligned16(aa_scale)) return GSR_E_ALIGN;
    const int64_t N = scene->N;
    if (N > 0) { // (the backward's own checks of geom and ws; cov3D and sh_dir_grad are optional)
        if (!geom_core(geom)) return GSR_E_NULL;
        if (!geom_aligned(geom)) return GSR_E_ALIGN;
        if (!bwd_ws_fits(ws, ws_bytes, scene, camera)) return GSR_E_WORKSPACE;
        if (!scratch || scratch_bytes < gsr_camera_scratch_bytes(N)) return GSR_E_WORKSPACE;
    }
    const CamK cam = make_cam(camera);
    const GradRec *acc = N > 0 ? carve_bwd(const_cast<void *>(ws), N).acc : nullptr;
    HIP_TRY(gsr_launch_camera_backward(*scene, cam, N > 0 ? *geom : GsrGeom{}, acc, dL_dcamera, scratch, (hipStream_t)stream, aa_scale));
    return GSR_OK;
}

int gsr_stage_timing(int enable, int max_steps)
{
    std::lock_guard<std::mutex> lk(g_timer_mu);
    if (g_timer.ev) {
        for (size_t i = 0; i < (size_t)g_timer.max_steps * StageTimer::PER; ++i) (void)hipEventDestroy(g_timer.ev[i]);
        free(g_timer.ev);
        g_timer.ev = nullptr;
    }
    g_timer.on = false;
    g_timer.max_steps = g_timer.fwd_step = g_timer.bwd_step = g_timer.fwd_calls = g_timer.bwd_calls = 0;
    g_timer.every = 1;
    if (!enable) return GSR_OK;
    if (max_steps <= 0 || max_steps > 4096) return GSR_E_DIMS;
    g_timer.ev = (hipEvent_t *)calloc((size_t)max_steps * StageTimer::PER, sizeof(hipEvent_t));
    if (!g_timer.ev) return GSR_E_WORKSPACE;
    for (size_t i = 0; i < (size_t)max_steps * StageTimer::PER; ++i) HIP_TRY(hipEventCreate(&g_timer.ev[i]));
    g_timer.max_steps = max_steps;
    g_timer.on = true;
    return GSR_OK;
}

int gsr_stage_sampling(int every)
{
    if (every < 0) return GSR_E_DIMS;
    std::lock_guard<std::mutex> lk(g_timer_mu);
    g_timer.every = every; // 0 = paused (events stay allocated), k >= 1 = one forward/backward pair in k
    g_timer.fwd_calls = g_timer.bwd_calls = 0;
    return GSR_OK;
}

int gsr_stage_times(float *avg_ms, int *steps)
{
    if (!avg_ms || !steps) return GSR_E_NULL;
    std::lock_guard<std::mutex> lk(g_timer_mu);
    for (int k = 0; k < GSR_NSTAGES; ++k) avg_ms[k] = 0.0f;
    int n = g_timer.fwd_step < g_timer.bwd_step ? g_timer.fwd_step : g_timer.bwd_step;
    if (n > g_timer.max_steps) n = g_timer.max_steps;
    *steps = n;
    if (!g_timer.on.load() || n == 0) return GSR_OK;
    // stage k of the forward lies between event slots k and k+1 (k = 0..8); backward stages 9..11 between 10+j and 11+j.
    // A record whose call ended early (an error return, D == 0) has unrecorded events: it is left out.
    int used = 0;
    for (int st = 0; st < n; ++st) {
        float ms[GSR_NSTAGES];
        bool whole = true;
        for (int k = 0; k < 9 && whole; ++k) whole = hipEventElapsedTime(&ms[k], g_timer.at(st, k), g_timer.at(st, k + 1)) == hipSuccess;
        for (int j = 0; j < 3 && whole; ++j) whole = hipEventElapsedTime(&ms[9 + j], g_timer.at(st, 10 + j), g_timer.at(st, 11 + j)) == hipSuccess;
        if (!whole) {
            (void)hipGetLastError();
            continue;
        }
        for (int k = 0; k < GSR_NSTAGES; ++k) avg_ms[k] += ms[k];
        ++used;
    }
    *steps = n = used;
    if (n == 0) return GSR_OK;
    for (int k = 0; k < GSR_NSTAGES; ++k) avg_ms[k] /= (float)n;
    g_timer.fwd_step = g_timer.bwd_step = 0;
    return GSR_OK;
}

} // extern "C"
