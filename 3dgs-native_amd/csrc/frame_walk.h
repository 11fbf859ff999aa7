// frame_walk.h -- the replay of the forward blend's weights over a finished frame's tile lists ("The frame-list walk"):
// what features.hip, distortion.hip and normal_render.hip share.  Like fixed_sum.h, everything sits in the including file's
// anonymous namespace.  Host part: the frame as a kernel argument, the three phases of its checks and the entry points' whole check.
// Device part: FrameWalk (the block, the bounds, staging, compaction, the pipelined walk and the weight expression), ValueTile (the
// backwards' transposed flush into the accumulator records) and what the depth stages stage and evaluate (DepthFill, plane_inv_depth).
#pragma once
#include <algorithm>
#include <type_traits>

#include "gsr_internal.h"
#include "gsr_plane_depth.h" // (and through it GsrDistortionFrame and GsrFeaturesFrame)

namespace {

// ---- host: the frame ----
struct FrameK {
    int W, H, grid_x;
    long long N, D;
    const float *xy;
    long long xy_stride;
    const float *co;
    long long co_stride;
    const int32_t *point_list;
    const int32_t *ranges;
    const int32_t *n_contrib;
    const uint8_t *masks;
};

// Frame: GsrFeaturesFrame or GsrDistortionFrame (the common fields carry the same names)
template <class Frame>
FrameK frame_k(const Frame *fr)
{
    FrameK k;
    k.W = fr->W; k.H = fr->H; k.grid_x = (fr->W + 15) / 16;
    k.N = fr->N; k.D = fr->point_list ? fr->D : 0;
    k.xy = fr->xy; k.xy_stride = fr->xy_stride;
    k.co = fr->conic_opacity; k.co_stride = fr->conic_opacity_stride;
    k.point_list = fr->point_list; k.ranges = fr->ranges; k.n_contrib = fr->n_contrib; k.masks = fr->block_masks;
    return k;
}
inline int frame_tiles(const FrameK &k) { return k.grid_x * ((k.H + 15) / 16); }

// The frame's share of an entry point's checks, one helper per phase: the entry point reports NULL for the frame and all its own
// pointers, then DIMS, then ALIGN (the headers' order, which the ABI tests hold).
template <class Frame>
bool frame_has_null(const Frame *fr)
{
    return !fr || !fr->xy || !fr->conic_opacity || !fr->ranges || !fr->n_contrib || (!fr->point_list && fr->D > 0);
}
template <class Frame>
bool frame_dims_ok(const Frame *fr)
{
    return fr->W >= 1 && fr->H >= 1 && fr->W <= GSR_FEATURES_MAX_SIDE && fr->H <= GSR_FEATURES_MAX_SIDE && fr->N >= 1 && fr->N <= 0x7FFFFFFFll &&
           fr->D >= 0 && fr->D <= GSR_MAX_RENDERED && fr->xy_stride >= 2 && fr->conic_opacity_stride >= 4;
}
template <class Frame>
bool frame_aligned(const Frame *fr)
{
    return gsr_aligned4(fr->xy) && gsr_aligned4(fr->conic_opacity) && gsr_aligned4(fr->point_list) && gsr_aligned4(fr->ranges) &&
           gsr_aligned4(fr->n_contrib);
}
// the entry point's own pointers: all of them 16-byte aligned
template <class... P>
bool all_aligned16(const P *...p)
{
    return (gsr_aligned16(p) && ...);
}
// An entry point's whole check over its frame and its own pointers: NULL, DIMS, ALIGN, in the headers' order; GSR_OK when the call
// may be enqueued.  A GsrDistortionFrame's inv_depth joins each phase.
template <class Frame, class... P>
int check_frame(const Frame *fr, const P *...p)
{
    constexpr bool INVD = std::is_same<Frame, GsrDistortionFrame>::value;
    if (frame_has_null(fr) || (!p || ...)) return GSR_E_NULL;
    if constexpr (INVD) if (!fr->inv_depth) return GSR_E_NULL;
    if (!frame_dims_ok(fr)) return GSR_E_DIMS;
    if constexpr (INVD) if (fr->inv_depth_stride < 1) return GSR_E_DIMS;
    if (!frame_aligned(fr) || !all_aligned16(p...)) return GSR_E_ALIGN;
    if constexpr (INVD) if (!gsr_aligned4(fr->inv_depth)) return GSR_E_ALIGN;
    return GSR_OK;
}

// ---- device ----
constexpr int BATCH = 256;   // list entries staged per round

__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); } // blend_fwd.hip's

// lanes of one wave exchange data through LDS: in order in hardware, but the compiler must not move the accesses across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One entry at one pixel, as blend_forward_kernel (blend_fwd.hip, GSR_BLEND) weighs it, bit for bit: every float32 restatement
// under tests/ replays these lines.  G = exp(power); t = the alpha the blend applies, 0 where power > 0.  The entry is applied where
// t >= 1/255 and the pixel's n_contrib reaches it (the walk's `applied`).
// Returns t; dx, dy and G are separate outputs, not a struct: a struct's neighbours invite the compiler to pair their arithmetic.
__device__ __forceinline__ float blend_forward_weight(const float4 &ra, const float4 &rb, float pixf_x, float pixf_y, float &dx, float &dy, float &G)
{
    dx = ra.x - pixf_x; dy = ra.y - pixf_y;
    const float power = (ra.z * dx * dx + rb.x * dy * dy) + ra.w * dx * dy;
    G = fast_exp(power);
    const float alpha = fminf(0.99f, rb.y * G);
    return power > 0.0f ? 0.0f : alpha;
}

// The depth stages' `fill` for run(): 1 / depth in the spare float of the second word and, with three words, the two slopes in the third.
struct DepthFill {
    const float *invd;
    long long invd_stride;
    const float *slopes; // [N][2]; unused with two words
    __device__ __forceinline__ void operator()(int id, float4 &rb) const { rb.w = invd[(size_t)id * invd_stride]; }
    __device__ __forceinline__ void operator()(int id, float4 &rb, float4 &rc) const
    {
        (*this)(id, rb);
        const float2 sl = reinterpret_cast<const float2 *>(slopes)[id];
        rc = make_float4(sl.x, sl.y, 0.f, 0.f);
    }
};

// The plane's inverse depth at a pixel (include/gsr_plane_depth.h): mr = m0 - gx dx - gy dy in two fused multiply-adds, dx and dy as
// blend_forward_weight forms them, and m = mr clamped to [m0 / 4, m0 * GSR_PLANE_DEPTH_MAX_RATIO].  Returns m; "not clamped" is
// m == mr.  Every stage that promises another the same m or the same clamp decision, bit for bit, calls this.
__device__ __forceinline__ float plane_inv_depth(float m0, float gx, float gy, float dx, float dy, float &mr)
{
    mr = __builtin_fmaf(-gx, dx, __builtin_fmaf(-gy, dy, m0));
    return fminf(fmaxf(mr, m0 * 0.25f), m0 * GSR_PLANE_DEPTH_MAX_RATIO);
}

// run()'s default `open`: no pixel ever closes, the walk runs to the tile's largest n_contrib
struct AlwaysOpen {};

// One 256-thread workgroup per 16x16 tile, each of its four waves owning one 8x8 pixel block (lane = pixel), as in blend_fwd.hip.
// The constructor and run() are the workgroup's: both hold workgroup barriers, so both stand outside any divergent path.
struct FrameWalk {
    int lane, wv;
    int bx0, by0;        // this wave's 8x8 block; pixel q of it = (bx0 + (q & 7), by0 + (q >> 3))
    int pix_x, pix_y;    // this lane's pixel
    bool inside;         // ... is on the image
    size_t pix;          // ... its index, 0 when off the image
    float pixf_x, pixf_y;
    unsigned long long lt_mask; // the lanes below this one
    int my_bits;         // this wave's 8x8 block = the 8x4 blocks k0 and k0 + 2 of the forward's masks (blend_fwd.hip)
    long long start;     // the tile's range, clipped to [0, D]
    int nc;              // this pixel's n_contrib, clipped to the range; 0 off the image
    int wmax, tmax;      // its maximum over the wave (wave-uniform) and over the workgroup

    // every thread of the workgroup, once, at the top of the kernel: two workgroup barriers
    __device__ __forceinline__ FrameWalk(const FrameK &f)
    {
        __shared__ int s_max;
        const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
        const int tile = blockIdx.x;
        const int tile_x = tile % f.grid_x, tile_y = tile / f.grid_x;
        const int bx0 = tile_x * 16 + (wv & 1) * 8, by0 = tile_y * 16 + (wv >> 1) * 8;
        const int pix_x = bx0 + (lane & 7), pix_y = by0 + (lane >> 3);
        const bool inside = pix_x < f.W && pix_y < f.H;
        pixf_x = (float)pix_x; pixf_y = (float)pix_y;
        lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        my_bits = 5 << ((wv >> 1) * 4 + (wv & 1));

        // the walk's bounds: the range clipped to [0, D], n_contrib to the range
        long long start = f.ranges[2 * tile], end = f.ranges[2 * tile + 1];
        start = std::min(std::max(start, 0ll), f.D);
        end = std::min(std::max(end, start), f.D);
        const int len = (int)(end - start);
        size_t pix = 0;
        int nc = 0;
        if (inside) {
            pix = (size_t)pix_y * f.W + pix_x;
            nc = std::min(std::max(f.n_contrib[pix], 0), len);
        }
        int wmax = nc;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d, 64));
        wmax = __builtin_amdgcn_readfirstlane(wmax);
        if (tid == 0) s_max = 0;
        __syncthreads();
        if (lane == 0) atomicMax(&s_max, wmax);
        __syncthreads();
        tmax = s_max;
        this->lane = lane; this->wv = wv; this->bx0 = bx0; this->by0 = by0; this->pix_x = pix_x; this->pix_y = pix_y;
        this->inside = inside; this->pix = pix; this->start = start; this->nc = nc; this->wmax = wmax;
    }

    // The tile's list, staged through LDS in batches of BATCH entries of WORDS float4 each: ra = {x, y, a', b'}, rb = {c', opacity, id,
    // spare} and, with WORDS = 3, a spare word rc (a', b', c' = the conic pre-scaled as in blend_fwd.hip).  An id outside [0, N) is
    // staged as zeros: opacity 0, never applied.  Each wave compacts a batch to the entries its block may see (the forward's 8x4-block
    // masks when the frame has them, every entry below the block's largest n_contrib otherwise) and walks them with lane = pixel.
    //   fill(id, rb[, rc])                         the spare float rb.w and the spare word of a staged record, from the Gaussian id
    //                                              in [0, N); may do nothing
    //   entry(ra, rb[, rc], dx, dy, G, t, applied) once per compacted entry, in list order, by all 64 lanes.  The kernel keeps its own
    //                                              transmittance: T *= 1 - t where `applied`, at the point its own arithmetic has it.
    // The words are separate values, not an array, so that each stays one 16-byte LDS access and four registers.
    // A wave with wmax == 0 compacts nothing and still serves every batch's two barriers.
    //   open()                                     optional: "this lane's pixel may still change".  A walk with it is the early-exit
    //                                              walk: entry() gets one more argument, the entry's 1-based list position; before
    //                                              every batch but the first a lane counts as open while open() holds and its
    //                                              n_contrib reaches into the batch; a wave without an open lane compacts nothing,
    //                                              and the workgroup leaves when no wave has one.  The exit is taken between batches
    //                                              only, by all 256 threads together (the verdict is read from LDS behind a barrier).
    template <int WORDS, class Fill, class Entry, class Open = AlwaysOpen>
    __device__ __forceinline__ void run(const FrameK &f, Fill fill, Entry entry, Open open = Open()) const
    {
        static_assert(WORDS == 2 || WORDS == 3, "two words, or three with the spare one");
        constexpr bool EXIT = !std::is_same<Open, AlwaysOpen>::value;
        __shared__ int s_open[EXIT ? 2 : 1]; // batch b's verdict in s_open[b & 1]; written only by an early-exit walk
        __shared__ float4 s_rec[BATCH][WORDS];
        __shared__ uint8_t s_mask[BATCH];
        __shared__ uint16_t s_list[4][BATCH + 2]; // per wave: the batch entries its block may see, in list order (+ two the walk reads ahead)
        const int tid = threadIdx.x;
        int wlim = wmax; // where this wave's compaction ends: wmax, or 0 once none of its lanes is open
        if constexpr (EXIT) {
            if (tid < 2) s_open[tid] = 0; // (ordered before the first write, batch 1's, by batch 0's barriers)
        }
        for (int base = 0; base < tmax; base += BATCH) {
            if constexpr (EXIT) {
                if (base > 0) {
                    if (__builtin_amdgcn_ballot_w64(base < nc && open()) == 0ull) wlim = 0;
                    else if (lane == 0) s_open[(base / BATCH) & 1] = 1;
                }
            }
            __syncthreads(); // every wave has walked the last batch
            if constexpr (EXIT) {
                if (base > 0 && s_open[(base / BATCH) & 1] == 0) break; // the same word for all 256 threads: a uniform exit
                if (tid == 0) s_open[(base / BATCH + 1) & 1] = 0;         // last read two barriers ago, next written behind the one below
            }
            const int cnt = min(BATCH, tmax - base);
            if (tid < cnt) {
                const long long at = start + base + tid; // < start + tmax <= end <= D
                const int id = f.point_list[at];
                float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra;
                if (id >= 0 && (long long)id < f.N) {
                    const float *pxy = f.xy + (size_t)id * f.xy_stride, *pco = f.co + (size_t)id * f.co_stride;
                    ra = make_float4(pxy[0], pxy[1], -0.5f * pco[0], -pco[1]);
                    rb = make_float4(-0.5f * pco[2], pco[3], __int_as_float(id), 0.f);
                    if constexpr (WORDS == 3) fill(id, rb, rc);
                    else fill(id, rb);
                }
                s_rec[tid][0] = ra;
                s_rec[tid][1] = rb;
                if constexpr (WORDS == 3) s_rec[tid][2] = rc;
                s_mask[tid] = f.masks ? f.masks[at] : (uint8_t)0xFF;
            }
            __syncthreads();
            int n = 0;
            for (int gb = 0; gb < cnt; gb += 64) {
                const int e = gb + lane;
                const bool hit = e < cnt && base + e < wlim && (s_mask[e] & my_bits) != 0;
                const unsigned long long bits = __ballot(hit);
                if (hit) s_list[wv][n + __popcll(bits & lt_mask)] = (uint16_t)e;
                n += __popcll(bits);
            }
            if (lane < 2) s_list[wv][n + lane] = 0; // the walk reads two list entries ahead; entry 0 of a batch always exists
            wave_lds_sync();
            // one-deep software pipeline: the record of entry k + 1 and the list slot of entry k + 2 are in flight while entry k is weighed
            int e = s_list[wv][0], e1 = s_list[wv][1];
            float4 ra = s_rec[e][0], rb = s_rec[e][1], rc, nn; // rc, nn: the third word, untouched with WORDS = 2
            if constexpr (WORDS == 3) rc = s_rec[e][2];
            for (int k = 0; k < n; ++k) {
                const int e2 = s_list[wv][k + 2];
                const float4 na = s_rec[e1][0], nb = s_rec[e1][1];
                if constexpr (WORDS == 3) nn = s_rec[e1][2];
                float dx, dy, G;
                const float t = blend_forward_weight(ra, rb, pixf_x, pixf_y, dx, dy, G);
                const bool applied = base + e < nc && !(t < (1.0f / 255.0f));
                if constexpr (EXIT) {
                    if constexpr (WORDS == 3) entry(ra, rb, rc, dx, dy, G, t, applied, base + e + 1);
                    else entry(ra, rb, dx, dy, G, t, applied, base + e + 1);
                } else if constexpr (WORDS == 3) entry(ra, rb, rc, dx, dy, G, t, applied);
                else entry(ra, rb, dx, dy, G, t, applied);
                e = e1; e1 = e2;
                ra = na; rb = nb;
                if constexpr (WORDS == 3) rc = nn;
            }
        }
    }
};

// The backwards' value tile: each lane files VALS per-(pixel, entry) values as VALS rows of a (SLOTS * VALS) x 64 tile in the wave's
// LDS; every SLOTS entries the flush sums each row with two lanes (32 pixels each, in order, then the two halves), applies the
// per-entry constants once and adds the entry's VALS sums with ONE atomic wave-instruction, whichever array a lane's value goes
// to: an atomic wave-instruction has a fixed issue price (profiles/normal_render/README.md).  blend_bwd_splat.hip's transposed
// flush, turned round for lane = pixel.  The first six values are S1, S2, Sxx, Sxy, Syy, Sop and go to the accumulator record's
// dmean2D x y | dconic a b c | dopacity; value k >= 6 of Gaussian id is added to tail[id * tail_stride + tail_column + k - 6], the
// kernel's choice.
template <int VALS, int SLOTS>
struct ValueTile {
    static constexpr int ROWS = SLOTS * VALS;
    static constexpr int PITCH = 65; // floats per row: odd, so the row-parallel reads of the flush spread over the 64 banks
    static_assert(VALS >= 6 && 2 * ROWS <= 64, "the flush sums a row with two lanes");
    // Its LDS, declared by the kernel as three arrays; LIVE = false (a forward instantiation) makes the tile one float.
    template <bool LIVE> using V = float[LIVE ? 4 : 1][LIVE ? ROWS * PITCH : 1]; // per wave: [entry slot][value][pixel]
    using Red = float[4][ROWS];                                                  // per wave: the rows' sums
    using Con = float4[4][SLOTS];                                                // per wave: {a', b', c', id} of each slot

    float *v;            // this wave's part of each
    float *red;
    float4 *con;
    float *acc;          // the accumulator records
    float *tail;         // where the values past the sixth go
    size_t tail_stride;
    int tail_column;
    float half_w, half_h;
    int lane;
    int ns = 0;          // slots filed since the last flush

    // v, red, con: this wave's rows of the three arrays
    __device__ __forceinline__ ValueTile(float *v, float *red, float4 *con, const FrameWalk &walk, const FrameK &f, float *accumulators, float *tail,
                                         int tail_stride, int tail_column)
        : v(v), red(red), con(con), acc(accumulators), tail(tail), tail_stride(tail_stride), tail_column(tail_column),
          half_w(0.5f * (float)f.W), half_h(0.5f * (float)f.H), lane(walk.lane)
    {
    }

    // the sums of entry slots [0, n), added to the accumulator records and the tail
    __device__ __forceinline__ void flush(int n)
    {
        wave_lds_sync();
        float sum = 0.0f;
        if (lane < 2 * ROWS) {
            const float *row = &v[(lane % ROWS) * PITCH + (lane / ROWS) * 32];
#pragma unroll
            for (int j = 0; j < 32; ++j) sum += row[j]; // rows of slots from n on hold stale values: never added
        }
        sum += __shfl_down(sum, ROWS, 64); // pixels 0-31 + pixels 32-63
        if (lane < ROWS) red[lane] = sum;
        wave_lds_sync();
        if (lane < ROWS) {
            const int slot = lane / VALS, k = lane % VALS;
            if (slot < n) {
                const float4 c = con[slot];
                const float *r = &red[slot * VALS];
                float out;
                if (k == 0) out = (2.0f * c.x * r[0] + c.y * r[1]) * half_w;
                else if (k == 1) out = (2.0f * c.z * r[1] + c.y * r[0]) * half_h;
                else if (k < 5) out = -0.5f * r[k];
                else out = r[k];
                const size_t id = (size_t)__float_as_int(c.w); // in [0, N): only a staged, applied entry is filed
                // one column chain, then the pointer: a kernel whose tail is the record itself (tail == acc, stride 16) gets one address
                const int col = k < 2 ? 3 + k : k < 4 ? 4 + k : k == 4 ? 9 : k == 5 ? 10 : tail_column + k - 6;
                float *dst = k < 6 ? &acc[id * 16 + col] : &tail[id * tail_stride + col];
                atomicAdd(dst, out);
            }
        }
        wave_lds_sync();
    }

    // One entry that some pixel of the block applies: this lane's values (zeros where it does not apply it) and the entry's record.
    __device__ __forceinline__ void file(const float (&val)[VALS], const float4 &ra, const float4 &rb)
    {
        float *col = &v[ns * VALS * PITCH + lane];
#pragma unroll
        for (int k = 0; k < VALS; ++k) col[k * PITCH] = val[k];
        if (lane == 0) con[ns] = make_float4(ra.z, ra.w, rb.x, rb.z);
        if (++ns == SLOTS) {
            flush(SLOTS);
            ns = 0;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (ns > 0) flush(ns);
    }
};

} // namespace
