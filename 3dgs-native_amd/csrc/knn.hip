// knn.hip -- exact 3-nearest-neighbour distances of a point cloud (include/gsr_knn.h): the start of a 3DGS run from SfM or random
// points.  A stage of its own: new kernels only, on the caller's stream, no host wait, no float atomics.
//
//   knn_box_kernel / knn_box_finish_kernel   the cloud's bounding box: at most BOX_BLOCKS partial records, then one workgroup.
//   knn_morton_kernel                        item = (30-bit Morton code << 32 | id), 10 bits per axis; an axis of zero extent gives 0.
//   knn_hist_kernel + gsr_launch_exclusive_scan + knn_scatter_kernel, four times
//                                            a plain stable LSD radix sort by 8-bit digits, 1024 items per workgroup: digit counts
//                                            per chunk (digit-major, so one exclusive scan places every (digit, chunk) run), then a
//                                            scatter whose rank inside the chunk comes from wave ballots (lanes with the same digit,
//                                            in lane order) and a 16-row count table in LDS.  It runs once per training run: written
//                                            to be read, not tuned like the binning chain, and it shares none of that chain's passes.
//   knn_gather_kernel                        the points in sorted order as (x, y, z, id), and each block of 256's bounding box.
//   knn_search_kernel                        one workgroup per block, one query per thread.  The own block first (that seeds the
//                                            three best), then the other blocks outwards in sorted order, 256 at a time: a thread
//                                            each tests one block's box against the own box and the workgroup's largest third-best
//                                            distance; for each block that passed, every thread tests ITS point against the box with its
//                                            current third best and the workgroup votes: a block some query needs is staged through
//                                            LDS, and the threads that need it scan it.
//   nearest_search_kernel                    the nearest point of ANOTHER set (include/gsr_mesh_eval.h, gsr_nearest): both sets through
//                                            the same chain under one common box, then the same walk with one best instead of three,
//                                            seeded by a binary search over the sorted reference codes.
// Nothing but pruning depends on the Morton order: every distance is the header's float32 expression, every comparison is by (d2, id).
#include <limits.h>
#include <math.h>

#include "gsr_internal.h"
#include "gsr_knn.h"
#include "gsr_mesh_eval.h"

namespace {

constexpr int NT = 256;               // threads per workgroup, everywhere
constexpr int BOX_BLOCKS = 1024;      // partial records of the bounding box at most
constexpr int SORT_ITEMS = 4;         // items per thread of a radix pass
constexpr int SORT_CHUNK = NT * SORT_ITEMS;
constexpr int SORT_ROWS = SORT_ITEMS * (NT / GSR_WAVE);   // (round, wave) pairs of a chunk, in item order
static_assert(GSR_KNN_BLOCK_POINTS == NT, "one query per thread, one staged candidate per thread");
static_assert(GSR_KNN_K == 3, "the three best are three registers");

struct Box { float4 lo, hi; };        // 32 bytes; .w unused

__device__ __forceinline__ float3 min3(float3 a, float3 b) { return make_float3(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)); }
__device__ __forceinline__ float3 max3(float3 a, float3 b) { return make_float3(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z)); }

// The workgroup's box from every thread's (lo, hi): a butterfly per wave, the 4 waves through LDS; thread 0 holds the result.
// min and max do not depend on the order.
__device__ __forceinline__ void block_box(float3 &lo, float3 &hi)
{
    __shared__ float s_box[NT / GSR_WAVE][6];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min3(lo, make_float3(__shfl_xor(lo.x, d, 64), __shfl_xor(lo.y, d, 64), __shfl_xor(lo.z, d, 64)));
        hi = max3(hi, make_float3(__shfl_xor(hi.x, d, 64), __shfl_xor(hi.y, d, 64), __shfl_xor(hi.z, d, 64)));
    }
    if ((threadIdx.x & 63) == 0) {
        float *r = s_box[threadIdx.x >> 6];
        r[0] = lo.x, r[1] = lo.y, r[2] = lo.z, r[3] = hi.x, r[4] = hi.y, r[5] = hi.z;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < NT / GSR_WAVE; ++w) {
            lo = min3(lo, make_float3(s_box[w][0], s_box[w][1], s_box[w][2]));
            hi = max3(hi, make_float3(s_box[w][3], s_box[w][4], s_box[w][5]));
        }
}
__device__ __forceinline__ void store_box(Box *b, float3 lo, float3 hi)
{
    b->lo = make_float4(lo.x, lo.y, lo.z, 0.0f);
    b->hi = make_float4(hi.x, hi.y, hi.z, 0.0f);
}

__global__ __launch_bounds__(NT) void knn_box_kernel(int64_t N, const float *__restrict__ points, Box *__restrict__ part)
{
    float3 lo = make_float3(INFINITY, INFINITY, INFINITY), hi = make_float3(-INFINITY, -INFINITY, -INFINITY);
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < N; i += (int64_t)gridDim.x * NT) {
        const float3 p = make_float3(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
        lo = min3(lo, p), hi = max3(hi, p);
    }
    block_box(lo, hi);
    if (threadIdx.x == 0) store_box(part + blockIdx.x, lo, hi);
}

__global__ __launch_bounds__(NT) void knn_box_finish_kernel(const Box *__restrict__ part, int n, Box *__restrict__ box)
{
    float3 lo = make_float3(INFINITY, INFINITY, INFINITY), hi = make_float3(-INFINITY, -INFINITY, -INFINITY);
    for (int r = threadIdx.x; r < n; r += NT) {
        const Box b = part[r];
        lo = min3(lo, make_float3(b.lo.x, b.lo.y, b.lo.z)), hi = max3(hi, make_float3(b.hi.x, b.hi.y, b.hi.z));
    }
    block_box(lo, hi);
    if (threadIdx.x == 0) store_box(box, lo, hi);
}

// 10 bits -> every third bit of 30
__device__ __forceinline__ uint32_t spread3(uint32_t v)
{
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// the cell 0..1023 of x on an axis [lo, hi]; an axis of zero extent has one cell.  (The clamp also takes the 0 * inf of an extent so
// small that 1024 / extent overflows: fmaxf(NaN, 0) = 0.)
__device__ __forceinline__ uint32_t cell(float x, float lo, float hi)
{
    const float e = hi - lo;
    const float s = e > 0.0f ? 1024.0f / e : 0.0f;
    return (uint32_t)fminf(fmaxf((x - lo) * s, 0.0f), 1023.0f);
}
__global__ __launch_bounds__(NT) void knn_morton_kernel(int64_t N, const float *__restrict__ points, const Box *__restrict__ box, uint64_t *__restrict__ items)
{
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const Box b = *box;
    const uint32_t code = spread3(cell(points[3 * i], b.lo.x, b.hi.x)) | (spread3(cell(points[3 * i + 1], b.lo.y, b.hi.y)) << 1) |
                          (spread3(cell(points[3 * i + 2], b.lo.z, b.hi.z)) << 2);
    items[i] = ((uint64_t)code << 32) | (uint64_t)(uint32_t)i;
}

__device__ __forceinline__ int digit_of(uint64_t item, int shift) { return (int)((item >> (32 + shift)) & 255u); }

// hist[digit * nchunks + chunk] = how many of the chunk's items have that digit (integer LDS atomics: a count has no order)
__global__ __launch_bounds__(NT) void knn_hist_kernel(int64_t N, const uint64_t *__restrict__ items, int shift, int32_t *__restrict__ hist)
{
    __shared__ int32_t s_cnt[256];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SORT_CHUNK;
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const int64_t i = base + r * NT + threadIdx.x;
        if (i < N) atomicAdd(&s_cnt[digit_of(items[i], shift)], 1);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = s_cnt[threadIdx.x];
}

// One stable pass: `start` is the exclusive scan of the histogram above.  An item's place is start[digit][chunk] + the items of
// that digit before it in the chunk; "before" is (round, wave, lane) order, which is index order.
__global__ __launch_bounds__(NT) void knn_scatter_kernel(int64_t N, const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int shift,
                                                         const int32_t *__restrict__ start)
{
    __shared__ int32_t s_cnt[SORT_ROWS][256];
    for (int k = threadIdx.x; k < SORT_ROWS * 256; k += NT) (&s_cnt[0][0])[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SORT_CHUNK;
    uint64_t item[SORT_ITEMS];
    int rank[SORT_ITEMS];
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const int64_t i = base + r * NT + threadIdx.x;
        const bool valid = i < N;
        item[r] = valid ? src[i] : 0;
        const int dg = digit_of(item[r], shift);
        unsigned long long same = __ballot(valid);              // the valid lanes of this wave with my digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long set = __ballot(valid && ((dg >> b) & 1));
            same &= ((dg >> b) & 1) ? set : ~set;
        }
        rank[r] = __popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank[r] == 0) s_cnt[r * (NT / GSR_WAVE) + wave][dg] = __popcll(same);   // the digit's first lane files the count
    }
    __syncthreads();
    {   // thread d: the rows of digit d become running starts
        int32_t run = start[(int64_t)threadIdx.x * gridDim.x + blockIdx.x];
        for (int row = 0; row < SORT_ROWS; ++row) {
            const int32_t c = s_cnt[row][threadIdx.x];
            s_cnt[row][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const int64_t i = base + r * NT + threadIdx.x;
        if (i >= N) continue;
        const int64_t to = (int64_t)s_cnt[r * (NT / GSR_WAVE) + wave][digit_of(item[r], shift)] + rank[r];
        if (to >= 0 && to < N) dst[to] = item[r];              // (a guard: the scan of the counts places every item inside)
    }
}

// slot j of the sorted order: (x, y, z, id) of its point; and the box of every block of 256 slots
__global__ __launch_bounds__(NT) void knn_gather_kernel(int64_t N, const float *__restrict__ points, const uint64_t *__restrict__ items,
                                                        float4 *__restrict__ sorted, Box *__restrict__ boxes)
{
    const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
    float3 lo = make_float3(INFINITY, INFINITY, INFINITY), hi = make_float3(-INFINITY, -INFINITY, -INFINITY);
    if (j < N) {
        int64_t id = (int64_t)(uint32_t)items[j];
        id = id < N ? id : N - 1;                              // (a guard: the ids are a permutation of 0 .. N-1)
        const float3 p = make_float3(points[3 * id], points[3 * id + 1], points[3 * id + 2]);
        sorted[j] = make_float4(p.x, p.y, p.z, __int_as_float((int)id));
        lo = hi = p;
    }
    block_box(lo, hi);
    if (threadIdx.x == 0) store_box(boxes + blockIdx.x, lo, hi);
}

// ---- the search ----
// the header's d2, operation by operation
__device__ __forceinline__ float dist2(float dx, float dy, float dz)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
// Lower bound of d2 between a point and any point of a box.  Per axis: left of the box every |x - p| is at least lo - x, right of
// it at least x - hi, and float32 subtraction is monotone; squares and the sums of non-negative terms are monotone too.
__device__ __forceinline__ float point_box_bound(float3 q, const Box &b)
{
    const float dx = fmaxf(fmaxf(__fsub_rn(b.lo.x, q.x), __fsub_rn(q.x, b.hi.x)), 0.0f);
    const float dy = fmaxf(fmaxf(__fsub_rn(b.lo.y, q.y), __fsub_rn(q.y, b.hi.y)), 0.0f);
    const float dz = fmaxf(fmaxf(__fsub_rn(b.lo.z, q.z), __fsub_rn(q.z, b.hi.z)), 0.0f);
    return dist2(dx, dy, dz);
}
// The same between any point of box a and any point of box b: the gap between the intervals on every axis.
__device__ __forceinline__ float box_box_bound(const Box &a, const Box &b)
{
    const float dx = fmaxf(fmaxf(__fsub_rn(b.lo.x, a.hi.x), __fsub_rn(a.lo.x, b.hi.x)), 0.0f);
    const float dy = fmaxf(fmaxf(__fsub_rn(b.lo.y, a.hi.y), __fsub_rn(a.lo.y, b.hi.y)), 0.0f);
    const float dz = fmaxf(fmaxf(__fsub_rn(b.lo.z, a.hi.z), __fsub_rn(a.lo.z, b.hi.z)), 0.0f);
    return dist2(dx, dy, dz);
}

// the three best candidates so far in (d2, id) order; an empty place is (inf, INT_MAX)
struct Best {
    float d0, d1, d2;
    int i0, i1, i2;
};
__device__ __forceinline__ bool before(float d, int j, float e, int k) { return d < e || (d == e && j < k); }
__device__ __forceinline__ void offer(Best &b, float d, int j)
{
    if (!before(d, j, b.d2, b.i2)) return;
    if (before(d, j, b.d1, b.i1)) {
        b.d2 = b.d1, b.i2 = b.i1;
        if (before(d, j, b.d0, b.i0)) b.d1 = b.d0, b.i1 = b.i0, b.d0 = d, b.i0 = j;
        else b.d1 = d, b.i1 = j;
    } else {
        b.d2 = d, b.i2 = j;
    }
}
// Every one of the `count` staged points but the one in slot `skip`.  Eight at a time: the eight LDS reads (one address for the
// whole wave each: broadcasts) are in flight together, where a loop of single reads waits out the LDS latency per candidate.
constexpr int SCAN_UNROLL = 8;
__device__ __forceinline__ void scan_staged(Best &b, float3 q, const float4 *s_pts, int count, int skip)
{
    int k = 0;
    for (; k + SCAN_UNROLL <= count; k += SCAN_UNROLL) {
        float4 p[SCAN_UNROLL];
#pragma unroll
        for (int u = 0; u < SCAN_UNROLL; ++u) p[u] = s_pts[k + u];
#pragma unroll
        for (int u = 0; u < SCAN_UNROLL; ++u) {
            const float d = dist2(__fsub_rn(q.x, p[u].x), __fsub_rn(q.y, p[u].y), __fsub_rn(q.z, p[u].z));
            if (k + u != skip) offer(b, d, __float_as_int(p[u].w));
        }
    }
    for (; k < count; ++k) {
        const float4 p = s_pts[k];
        const float d = dist2(__fsub_rn(q.x, p.x), __fsub_rn(q.y, p.y), __fsub_rn(q.z, p.z));
        if (k != skip) offer(b, d, __float_as_int(p.w));
    }
}
// the largest v of the workgroup, in every thread (the barrier inside also orders the LDS traffic around the call)
__device__ __forceinline__ float block_max(float v)
{
    __shared__ float s_max[NT / GSR_WAVE];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
}

__global__ __launch_bounds__(NT) void knn_search_kernel(int64_t N, int nb, const float4 *__restrict__ sorted, const Box *__restrict__ boxes,
                                                        float *__restrict__ mean_dist2, int32_t *__restrict__ nn_index /* may be NULL */)
{
    __shared__ float4 s_pts[NT];
    __shared__ Box s_cbox[NT];
    __shared__ int s_cand[NT];
    __shared__ uint32_t s_kept[NT / 32];
    const int t = threadIdx.x, b = blockIdx.x;
    const int64_t slot = (int64_t)b * NT + t;
    const bool active = slot < N;
    const float4 me = active ? sorted[slot] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float3 q = make_float3(me.x, me.y, me.z);
    const Box own = boxes[b];
    Best best = {INFINITY, INFINITY, INFINITY, INT_MAX, INT_MAX, INT_MAX};

    // the own block: every query meets its 255 nearest places of the sorted order
    s_pts[t] = me;
    __syncthreads();
    if (active) scan_staged(best, q, s_pts, (int)min((int64_t)NT, N - (int64_t)b * NT), t);
    // a thread without a query needs nothing: -1 is below every bound
    float wg_third = block_max(active ? best.d2 : -1.0f);

    // the other blocks, b + 1, b - 1, b + 2, ... : near places of the sorted order first, they shrink the third-best soonest
    const int reach = max(b, nb - 1 - b);
    for (int k0 = 1; k0 <= 2 * reach; k0 += NT) {
        const int k = k0 + t;
        const int c = b + ((k & 1) ? (k + 1) / 2 : -(k / 2));
        int keep = -1;
        if (k <= 2 * reach && c >= 0 && c < nb) {
            const Box cb = boxes[c];
            if (!(box_box_bound(own, cb) > wg_third)) keep = c, s_cbox[t] = cb;
        }
        s_cand[t] = keep;
        const unsigned long long kept = __ballot(keep >= 0);
        if ((t & 63) == 0) s_kept[t >> 5] = (uint32_t)kept, s_kept[(t >> 5) + 1] = (uint32_t)(kept >> 32);
        __syncthreads();
        // The own box is a coarse filter: a block that straddles a high Morton boundary spans the cloud, and every box passes.  So a
        // survivor is staged only if some query needs it NOW -- every thread tests its point against the box with its current third
        // best, and the workgroup votes -- because the first blocks staged shrink a stray query's reach by orders of magnitude.
        // The masks are the same in every thread (made scalar: the loops and their barriers are uniform).
        for (int w = 0; w < NT / 32; ++w)
            for (uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_kept[w]); m; m &= m - 1) {   // nearest place first
                const int i = w * 32 + (__ffs(m) - 1);
                // skip only on a bound STRICTLY above the third best: a point at that very distance may still win on its index
                const bool need = active && !(point_box_bound(q, s_cbox[i]) > best.d2);
                if (!__syncthreads_or(need)) continue;         // (the barrier: the last staged block has been read)
                const int64_t first = (int64_t)s_cand[i] * NT;
                if (first + t < N) s_pts[t] = sorted[first + t];
                __syncthreads();
                if (need) scan_staged(best, q, s_pts, (int)min((int64_t)NT, N - first), -1);
            }
        wg_third = block_max(active ? best.d2 : -1.0f);
    }
    if (!active) return;
    const int64_t id = (int64_t)__float_as_int(me.w);
    const int k = (int)min((int64_t)GSR_KNN_K, N - 1);
    float sum = 0.0f;
    if (k >= 1) sum = best.d0;
    if (k >= 2) sum = __fadd_rn(sum, best.d1);
    if (k >= 3) sum = __fadd_rn(sum, best.d2);
    mean_dist2[id] = k >= 1 ? __fdiv_rn(sum, (float)k) : 0.0f;
    if (nn_index) {
        nn_index[3 * id + 0] = best.i0 == INT_MAX ? -1 : best.i0;
        nn_index[3 * id + 1] = best.i1 == INT_MAX ? -1 : best.i1;
        nn_index[3 * id + 2] = best.i2 == INT_MAX ? -1 : best.i2;
    }
}

// ---- the workspace ----
struct KnnWs {
    Box *box_part, *box;      // [BOX_BLOCKS], [1]
    uint64_t *item[2];        // [N] each
    int32_t *hist, *start;    // [256 * chunks] each
    int32_t *scan_tmp;        // [ceil(256 * chunks / GSR_SCAN_WAVE_ITEMS) + 4]
    float4 *sorted;           // [N]
    Box *boxes;               // [blocks]
    size_t bytes;
};
bool count_ok(int64_t N) { return N >= 1 && N <= GSR_KNN_MAX_POINTS; }
KnnWs carve(void *base, int64_t N)
{
    const size_t n = (size_t)N, chunks = (size_t)gsr_div_up(N, SORT_CHUNK), blocks = (size_t)gsr_div_up(N, NT), h = 256 * chunks;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = p + off; off += gsr_align(bytes); return q; };
    KnnWs w;
    w.box_part = reinterpret_cast<Box *>(take(sizeof(Box) * (BOX_BLOCKS + 1)));
    w.box = w.box_part + BOX_BLOCKS;
    w.item[0] = reinterpret_cast<uint64_t *>(take(8 * n));
    w.item[1] = reinterpret_cast<uint64_t *>(take(8 * n));
    w.hist = reinterpret_cast<int32_t *>(take(4 * h));
    w.start = reinterpret_cast<int32_t *>(take(4 * h));
    w.scan_tmp = reinterpret_cast<int32_t *>(take(4 * ((size_t)gsr_div_up((int64_t)h, GSR_SCAN_WAVE_ITEMS) + 4)));
    w.sorted = reinterpret_cast<float4 *>(take(16 * n));
    w.boxes = reinterpret_cast<Box *>(take(sizeof(Box) * blocks));
    w.bytes = off;
    return w;
}

// The Morton items of `points` under *box in item[0], sorted: four 8-bit digits cover the 30 bits of code, and an even count of
// passes ends in item[0].  One chain for both stages of this file.
bool sort_by_morton(int64_t N, const float *points, const Box *box, uint64_t *const item[2], int32_t *hist, int32_t *start, int32_t *scan_tmp,
                    hipStream_t s)
{
    const int blocks = (int)gsr_div_up(N, NT), chunks = (int)gsr_div_up(N, SORT_CHUNK);
    hipLaunchKernelGGL(knn_morton_kernel, dim3(blocks), dim3(NT), 0, s, N, points, box, item[0]);
    for (int pass = 0; pass < 4; ++pass) {
        const uint64_t *src = item[pass & 1];
        hipLaunchKernelGGL(knn_hist_kernel, dim3(chunks), dim3(NT), 0, s, N, src, 8 * pass, hist);
        if (gsr_launch_exclusive_scan(hist, start, scan_tmp, (int64_t)256 * chunks, s) != hipSuccess) return false;
        hipLaunchKernelGGL(knn_scatter_kernel, dim3(chunks), dim3(NT), 0, s, N, src, item[(pass & 1) ^ 1], 8 * pass, (const int32_t *)start);
    }
    return true;
}

// ---- the nearest point of ANOTHER set (include/gsr_mesh_eval.h) ----
// Both sets go through the chain above under one box, so equal codes are equal cells.  One workgroup per block of 256 sorted
// queries, one query per thread.  The walk over the reference blocks starts where a binary search places the middle query's code
// among the sorted reference codes and goes outwards, s, s + 1, s - 1, ...: near places of the sorted order first, they shrink the
// best distance soonest.  The two filters are knn_search_kernel's.  With one neighbour to keep, the best is two registers.
static_assert(GSR_NEAREST_BLOCK_POINTS == NT, "one query per thread, one staged reference per thread");
static_assert(GSR_NEAREST_MAX_POINTS == GSR_KNN_MAX_POINTS, "one count check for both stages");

__device__ __forceinline__ void scan_staged_nearest(float &bd, int &bi, float3 q, const float4 *s_pts, int count)
{
    int k = 0;
    for (; k + SCAN_UNROLL <= count; k += SCAN_UNROLL) {
        float4 p[SCAN_UNROLL];
#pragma unroll
        for (int u = 0; u < SCAN_UNROLL; ++u) p[u] = s_pts[k + u];
#pragma unroll
        for (int u = 0; u < SCAN_UNROLL; ++u) {
            const float d = dist2(__fsub_rn(q.x, p[u].x), __fsub_rn(q.y, p[u].y), __fsub_rn(q.z, p[u].z));
            const int j = __float_as_int(p[u].w);
            if (before(d, j, bd, bi)) bd = d, bi = j;
        }
    }
    for (; k < count; ++k) {
        const float4 p = s_pts[k];
        const float d = dist2(__fsub_rn(q.x, p.x), __fsub_rn(q.y, p.y), __fsub_rn(q.z, p.z));
        const int j = __float_as_int(p.w);
        if (before(d, j, bd, bi)) bd = d, bi = j;
    }
}

__global__ __launch_bounds__(NT) void nearest_search_kernel(int64_t M, int64_t N, int nbr, const float4 *__restrict__ qsorted, const Box *__restrict__ qboxes,
                                                            const uint64_t *__restrict__ qitems, const float4 *__restrict__ rsorted,
                                                            const Box *__restrict__ rboxes, const uint64_t *__restrict__ ritems, float max_dist2,
                                                            float *__restrict__ dist2_out, int32_t *__restrict__ index_out /* may be NULL */)
{
    __shared__ float4 s_pts[NT];
    __shared__ Box s_cbox[NT];
    __shared__ int s_cand[NT];
    __shared__ uint32_t s_kept[NT / 32];
    const int t = threadIdx.x, b = blockIdx.x;
    const int64_t slot = (int64_t)b * NT + t;
    const bool active = slot < M;                              // a thread without a query stays: it serves every barrier and vote below
    const float4 me = active ? qsorted[slot] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float3 q = make_float3(me.x, me.y, me.z);
    const Box own = qboxes[b];                                 // (of the block's queries only: gather leaves the empty slots out)
    // the cap is the first best: a candidate enters at d2 <= max_dist2 (INT_MAX is above every index), and it prunes from the start
    float bd = max_dist2;
    int bi = INT_MAX;

    // the seed: the first place of the sorted references whose code is not below the middle query's (the same in every thread)
    const int64_t mid = (int64_t)b * NT + min((int64_t)NT, M - (int64_t)b * NT) / 2;
    const uint32_t qcode = (uint32_t)(qitems[mid] >> 32);
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t m = lo + (hi - lo) / 2;
        if ((uint32_t)(ritems[m] >> 32) < qcode) lo = m + 1;
        else hi = m;
    }
    const int seed = __builtin_amdgcn_readfirstlane((int)min(lo / NT, (int64_t)nbr - 1));

    // a thread without a query needs nothing: -1 is below every bound
    float wg_best = block_max(active ? bd : -1.0f);
    const int reach = max(seed, nbr - 1 - seed);
    for (int k0 = 0; k0 <= 2 * reach; k0 += NT) {
        const int k = k0 + t;
        const int c = seed + ((k & 1) ? (k + 1) / 2 : -(k / 2));
        int keep = -1;
        if (k <= 2 * reach && c >= 0 && c < nbr) {
            const Box cb = rboxes[c];
            if (!(box_box_bound(own, cb) > wg_best)) keep = c, s_cbox[t] = cb;
        }
        s_cand[t] = keep;
        const unsigned long long kept = __ballot(keep >= 0);
        if ((t & 63) == 0) s_kept[t >> 5] = (uint32_t)kept, s_kept[(t >> 5) + 1] = (uint32_t)(kept >> 32);
        __syncthreads();
        // As in knn_search_kernel: a survivor of the coarse filter is staged only if some query needs it NOW.  The masks are the same
        // in every thread (made scalar: the loops and their barriers are uniform).
        for (int w = 0; w < NT / 32; ++w)
            for (uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_kept[w]); m; m &= m - 1) {   // nearest place first
                const int i = w * 32 + (__ffs(m) - 1);
                // skip only on a bound STRICTLY above the best: a reference at that very distance may still win on its index
                const bool need = active && !(point_box_bound(q, s_cbox[i]) > bd);
                if (!__syncthreads_or(need)) continue;         // (the barrier: the last staged block has been read)
                const int64_t first = (int64_t)s_cand[i] * NT;
                if (first + t < N) s_pts[t] = rsorted[first + t];
                __syncthreads();
                if (need) scan_staged_nearest(bd, bi, q, s_pts, (int)min((int64_t)NT, N - first));
            }
        wg_best = block_max(active ? bd : -1.0f);
    }
    if (!active) return;
    int64_t id = (int64_t)__float_as_int(me.w);
    id = id >= 0 && id < M ? id : 0;                           // (a guard: the ids are a permutation of 0 .. M-1)
    dist2_out[id] = bi == INT_MAX ? INFINITY : bd;
    if (index_out) index_out[id] = bi == INT_MAX ? -1 : bi;
}

struct SetWs {
    uint64_t *item[2];        // [X] each
    float4 *sorted;           // [X]
    Box *boxes;               // [ceil(X / 256)]
};
struct NearestWs {
    Box *box_part, *box;      // [2 * BOX_BLOCKS], [1]
    SetWs q, r;
    int32_t *hist, *start;    // [256 * chunks(max(M, N))] each
    int32_t *scan_tmp;
    size_t bytes;
};
NearestWs carve_nearest(void *base, int64_t M, int64_t N)
{
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = p + off; off += gsr_align(bytes); return q; };
    auto set = [&](int64_t X) {
        SetWs w;
        w.item[0] = reinterpret_cast<uint64_t *>(take(8 * (size_t)X));
        w.item[1] = reinterpret_cast<uint64_t *>(take(8 * (size_t)X));
        w.sorted = reinterpret_cast<float4 *>(take(16 * (size_t)X));
        w.boxes = reinterpret_cast<Box *>(take(sizeof(Box) * (size_t)gsr_div_up(X, NT)));
        return w;
    };
    NearestWs w;
    w.box_part = reinterpret_cast<Box *>(take(sizeof(Box) * (2 * BOX_BLOCKS + 1)));
    w.box = w.box_part + 2 * BOX_BLOCKS;
    w.q = set(M);
    w.r = set(N);
    const size_t h = 256 * (size_t)gsr_div_up(M > N ? M : N, SORT_CHUNK);
    w.hist = reinterpret_cast<int32_t *>(take(4 * h));
    w.start = reinterpret_cast<int32_t *>(take(4 * h));
    w.scan_tmp = reinterpret_cast<int32_t *>(take(4 * ((size_t)gsr_div_up((int64_t)h, GSR_SCAN_WAVE_ITEMS) + 4)));
    w.bytes = off;
    return w;
}

} // namespace

extern "C" {

size_t gsr_knn_workspace_bytes(int64_t N) { return count_ok(N) ? carve(nullptr, N).bytes : 0; }

int gsr_knn(int64_t N, const float *points, float *mean_dist2, int32_t *nn_index, void *ws, size_t ws_bytes, void *stream)
{
    if (!points || !mean_dist2 || !ws) return GSR_E_NULL;
    if (!count_ok(N)) return GSR_E_DIMS;
    if (!gsr_aligned16(points) || !gsr_aligned16(mean_dist2) || !gsr_aligned16(nn_index) || !gsr_aligned16(ws)) return GSR_E_ALIGN;
    if (ws_bytes < gsr_knn_workspace_bytes(N)) return GSR_E_WORKSPACE;
    const KnnWs w = carve(ws, N);
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (int)gsr_div_up(N, NT), box_blocks = blocks < BOX_BLOCKS ? blocks : BOX_BLOCKS;
    hipLaunchKernelGGL(knn_box_kernel, dim3(box_blocks), dim3(NT), 0, s, N, points, w.box_part);
    hipLaunchKernelGGL(knn_box_finish_kernel, dim3(1), dim3(NT), 0, s, (const Box *)w.box_part, box_blocks, w.box);
    if (!sort_by_morton(N, points, w.box, w.item, w.hist, w.start, w.scan_tmp, s)) return GSR_E_HIP;
    hipLaunchKernelGGL(knn_gather_kernel, dim3(blocks), dim3(NT), 0, s, N, points, (const uint64_t *)w.item[0], w.sorted, w.boxes);
    hipLaunchKernelGGL(knn_search_kernel, dim3(blocks), dim3(NT), 0, s, N, blocks, (const float4 *)w.sorted, (const Box *)w.boxes, mean_dist2, nn_index);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_E_HIP;
}

size_t gsr_nearest_workspace_bytes(int64_t M, int64_t N) { return count_ok(M) && count_ok(N) ? carve_nearest(nullptr, M, N).bytes : 0; }

int gsr_nearest(int64_t M, const float *queries, int64_t N, const float *refs, float max_dist2, float *dist2, int32_t *index, void *ws, size_t ws_bytes,
                void *stream)
{
    if (!queries || !refs || !dist2 || !ws) return GSR_E_NULL;
    if (!count_ok(M) || !count_ok(N) || !(max_dist2 >= 0.0f)) return GSR_E_DIMS;          // (a NaN fails the comparison)
    if (!gsr_aligned16(queries) || !gsr_aligned16(refs) || !gsr_aligned16(dist2) || !gsr_aligned16(index) || !gsr_aligned16(ws)) return GSR_E_ALIGN;
    if (ws_bytes < gsr_nearest_workspace_bytes(M, N)) return GSR_E_WORKSPACE;
    const NearestWs w = carve_nearest(ws, M, N);
    hipStream_t s = (hipStream_t)stream;
    const int qblocks = (int)gsr_div_up(M, NT), rblocks = (int)gsr_div_up(N, NT);
    const int qbox = qblocks < BOX_BLOCKS ? qblocks : BOX_BLOCKS, rbox = rblocks < BOX_BLOCKS ? rblocks : BOX_BLOCKS;
    // one box over both sets: the references' partial records lie behind the queries', and one finish takes them all
    hipLaunchKernelGGL(knn_box_kernel, dim3(qbox), dim3(NT), 0, s, M, queries, w.box_part);
    hipLaunchKernelGGL(knn_box_kernel, dim3(rbox), dim3(NT), 0, s, N, refs, w.box_part + qbox);
    hipLaunchKernelGGL(knn_box_finish_kernel, dim3(1), dim3(NT), 0, s, (const Box *)w.box_part, qbox + rbox, w.box);
    if (!sort_by_morton(M, queries, w.box, w.q.item, w.hist, w.start, w.scan_tmp, s)) return GSR_E_HIP;
    hipLaunchKernelGGL(knn_gather_kernel, dim3(qblocks), dim3(NT), 0, s, M, queries, (const uint64_t *)w.q.item[0], w.q.sorted, w.q.boxes);
    if (!sort_by_morton(N, refs, w.box, w.r.item, w.hist, w.start, w.scan_tmp, s)) return GSR_E_HIP;
    hipLaunchKernelGGL(knn_gather_kernel, dim3(rblocks), dim3(NT), 0, s, N, refs, (const uint64_t *)w.r.item[0], w.r.sorted, w.r.boxes);
    hipLaunchKernelGGL(nearest_search_kernel, dim3(qblocks), dim3(NT), 0, s, M, N, rblocks, (const float4 *)w.q.sorted, (const Box *)w.q.boxes,
                       (const uint64_t *)w.q.item[0], (const float4 *)w.r.sorted, (const Box *)w.r.boxes, (const uint64_t *)w.r.item[0], max_dist2, dist2,
                       index);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_E_HIP;
}

} // extern "C"
