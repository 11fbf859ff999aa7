// normal_render.hip -- the Gaussians' own normals, their image over a frame's lists, its gradient into the backward's accumulator
// records, and the depth-normal consistency term (include/gsr_normal_render.h), for gfx950.
//
// gaussian_normals_kernel<BWD>: one thread per Gaussian, the header's steps (a) and (b) word for word; the view matrix travels as a
// kernel argument.  consistency_kernel: one thread per pixel of a grid-stride walk, elementwise, plus fixed_sum.h's tree for the two sums.
//
// normal_render_kernel<BWD> replays the forward blend's weights the way distortion.hip does: one 256-thread workgroup per 16x16
// tile, each of its four waves owning one 8x8 pixel block (lane = pixel), the tile's list staged through LDS in batches of 256
// entries (48 bytes each: position, pre-scaled conic, opacity, id, the Gaussian's normal), each wave compacting a batch to the
// entries its block may see and walking them with blend_forward_kernel's weight expression.
//   - forward: three running registers per lane, one fmaf per channel and applied entry in list order: what features.hip's exact
//     float32 MFMA computes at C = 3, without filing 32-column weight tiles for a product that uses 3 of its 32 channels.
//   - backward: distortion.hip's walk with u = G . n, and nine per-(pixel, entry) values instead of seven.  The flush there sums each
//     row of the value tile with two lanes (32 pixels each, in order, then the two halves), which needs 2 * ROWS <= 64 lanes.  Nine
//     values at four slots are 36 rows, 72 lanes: over.  The choices were (1) four slots and a second flush round for rows 32-35 --
//     two rounds of 32 dependent LDS adds for 8 more rows, and 36 x 65 x 4 B x 4 waves = 37 KB of LDS on top of the 12 KB of staging;
//     (2) one lane per row, 7 slots = 63 rows -- every lane busy, but 64 dependent adds per flush and 66 KB of LDS, two workgroups
//     per CU; (3) THREE slots: 27 rows, 54 of 64 lanes busy in the same two-lanes-per-row, 32-add flush, the header's summation
//     order unchanged, 28 KB of LDS for the value tile (distortion.hip's own figure).  With the 12 KB of staging (4 KB more than
//     that kernel's: the normals) the workgroup holds 43 KB, so three workgroups fit a CU's 160 KB where distortion.hip's 40 KB
//     fits four; the compiler's report (profiles/normal_render/kres.txt) says so too.  (3): the flush's cost
//     per entry is 32 adds / 3 entries against 32 / 4, a quarter more LDS read issue on a kernel whose walk, not whose flush,
//     is the long pole (the walk's per-entry chain -- exp, division, nine LDS stores -- is paid for every applied entry either way),
//     and it keeps the fixed order that the float32 restatement of the tests replays.  PITCH 65 (odd) spreads the flush's
//     row-parallel reads over the 64 banks; the walk's column stores (lane = consecutive floats) are conflict-free by construction.
//     Float atomics: one per (block, applied entry, value), 36 bytes per entry over two cache lines (the record's columns 3-10
//     and the Gaussian's row of dL_dnormals); -munsafe-fp-atomics makes them the hardware's global_atomic_add_f32, no CAS loop.
#include <algorithm>
#include <math.h>

#include "gsr_internal.h"
#include "gsr_normal_render.h"
#include "fixed_sum.h"

namespace {

constexpr int BATCH = 256;   // list entries staged per round
constexpr int SLOTS = 3;     // entries per flush of the backward (see above)
constexpr int VALS = 9;      // S1, S2, Sxx, Sxy, Syy, Sop, Snx, Sny, Snz
constexpr int ROWS = SLOTS * VALS;
constexpr int PITCH = 65;    // floats per row of the value tile: odd, so the row-parallel reads of the flush spread over the 64 banks
static_assert(2 * ROWS <= 64, "the flush sums a row with two lanes");

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

struct ViewK {
    float v[16];
};

__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); } // blend_fwd.hip's

// lanes of one wave exchange data through LDS: in order in hardware, but the compiler must not move the accesses across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// accumulator column of the k-th value the flush adds (k < 6): dmean2D x y | dconic a b c | dopacity
__device__ __forceinline__ int acc_column(int k) { return k < 2 ? 3 + k : k < 4 ? 4 + k : k == 4 ? 9 : 10; }

// ---- (a), (b): one thread per Gaussian ----
// BWD: `g_in` is dL_dnormals [N][3] and `out` dL_drot [N][4] (added to); else `out` is normals [N][3].
template <bool BWD>
__global__ __launch_bounds__(256) void gaussian_normals_kernel(long long N, const float *__restrict__ scales, const float *__restrict__ rots,
                                                               const float *__restrict__ means, ViewK V, const float *__restrict__ g_in,
                                                               float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
    const float4 q = *reinterpret_cast<const float4 *>(rots + 4 * i);
    int c = 0;
    if (s[1] < s[c]) c = 1;
    if (s[2] < s[c]) c = 2;
    // column c of sigma3d.h's rotation matrix: its expressions, its order
    const float cs = 2.0f * q.w * q.w - 1.0f;
    const float qv[3] = {q.x, q.y, q.z};
    const float v[3] = {c == 0 ? 1.0f : 0.0f, c == 1 ? 1.0f : 0.0f, c == 2 ? 1.0f : 0.0f};
    const float cr[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
    float d = qv[0] * v[0];
    d += qv[1] * v[1];
    d += qv[2] * v[2];
    float a[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) a[r] = v[r] * cs + cr[r] * q.w * 2.0f + qv[r] * d * 2.0f;
    const float l2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const bool ok = l2 >= GSR_NORMAL_RENDER_MIN_AXIS2 && !(q.x == 0.0f && q.y == 0.0f && q.z == 0.0f && q.w == 0.0f);
    const float len = __fsqrt_rn(ok ? l2 : 1.0f);
    float ah[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) ah[r] = __fdiv_rn(a[r], len);
    float nc[3], pv[3];
    const float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        nc[j] = (ah[0] * V.v[j] + ah[1] * V.v[4 + j]) + ah[2] * V.v[8 + j];
        pv[j] = ((V.v[j] * p[0] + V.v[4 + j] * p[1]) + V.v[8 + j] * p[2]) + V.v[12 + j];
    }
    const float t = (nc[0] * pv[0] + nc[1] * pv[1]) + nc[2] * pv[2];
    const float sigma = t > 0.0f ? -1.0f : 1.0f;
    if (!BWD) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = ok ? sigma * nc[j] : 0.0f;
        return;
    }
    if (!ok) return;
    float gc[3], gw[3], ga[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) gc[j] = sigma * g_in[3 * i + j];
#pragma unroll
    for (int r = 0; r < 3; ++r) gw[r] = (V.v[4 * r] * gc[0] + V.v[4 * r + 1] * gc[1]) + V.v[4 * r + 2] * gc[2];
    const float e = (ah[0] * gw[0] + ah[1] * gw[1]) + ah[2] * gw[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) ga[r] = __fdiv_rn(gw[r] - ah[r] * e, len);
    const float k = (q.x * ga[0] + q.y * ga[1]) + q.z * ga[2];
    const float X[3] = {v[1] * ga[2] - v[2] * ga[1], v[2] * ga[0] - v[0] * ga[2], v[0] * ga[1] - v[1] * ga[0]};
    const float qc = qv[c], gac = ga[c];
    float4 dq = *reinterpret_cast<float4 *>(out + 4 * i);
    dq.x += ((2.0f * q.w) * X[0] + (2.0f * qc) * ga[0]) + (2.0f * k) * v[0];
    dq.y += ((2.0f * q.w) * X[1] + (2.0f * qc) * ga[1]) + (2.0f * k) * v[1];
    dq.z += ((2.0f * q.w) * X[2] + (2.0f * qc) * ga[2]) + (2.0f * k) * v[2];
    dq.w += (4.0f * q.w) * gac + 2.0f * ((ga[0] * cr[0] + ga[1] * cr[1]) + ga[2] * cr[2]);
    *reinterpret_cast<float4 *>(out + 4 * i) = dq;
}

// ---- (c), (d): the list walk ----
// BWD: `g_in` is dL_dout [H][W][3], `img` the stored forward image (read), `acc` the accumulator records, `dnorm` dL_dnormals [N][3]
// (cleared by the caller); else `img` is written.
template <bool BWD>
__global__ __launch_bounds__(256) void normal_render_kernel(FrameK f, const float *__restrict__ normals, const float *__restrict__ g_in, float *img,
                                                            float *__restrict__ acc, float *__restrict__ dnorm)
{
    __shared__ float4 s_rec[BATCH][3];    // {x, y, a', b'} {c', opacity, id, -} {n.x, n.y, n.z, -}
    __shared__ uint8_t s_mask[BATCH];
    __shared__ uint16_t s_list[4][BATCH + 2]; // per wave: the batch entries its block may see, in list order (+ two the walk reads ahead)
    __shared__ float s_v[BWD ? 4 : 1][BWD ? ROWS * PITCH : 1]; // per wave: [entry slot][value][pixel]
    __shared__ float s_red[4][ROWS];      // per wave: the rows' sums
    __shared__ float4 s_con[4][SLOTS];    // per wave: {a', b', c', id} of each slot
    __shared__ int s_max;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = blockIdx.x;
    const int tile_x = tile % f.grid_x, tile_y = tile / f.grid_x;
    const int bx0 = tile_x * 16 + (wv & 1) * 8, by0 = tile_y * 16 + (wv >> 1) * 8; // this wave's 8x8 block; pixel q of it = (q & 7, q >> 3)
    const int pix_x = bx0 + (lane & 7), pix_y = by0 + (lane >> 3);
    const bool inside = pix_x < f.W && pix_y < f.H;
    const size_t pix = inside ? (size_t)pix_y * f.W + pix_x : 0;
    const float pixf_x = (float)pix_x, pixf_y = (float)pix_y;
    const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int my_bits = 5 << ((wv >> 1) * 4 + (wv & 1)); // this wave's 8x8 block = the 8x4 blocks k0 and k0 + 2 (blend_fwd.hip)

    // the walk's bounds: the range clipped to [0, D], n_contrib to the range
    long long start = f.ranges[2 * tile], end = f.ranges[2 * tile + 1];
    start = std::min(std::max(start, 0ll), f.D);
    end = std::min(std::max(end, start), f.D);
    const int len = (int)(end - start);
    int nc = 0;
    if (inside) nc = std::min(std::max(f.n_contrib[pix], 0), len);
    int wmax = nc;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d, 64));
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    if (tid == 0) s_max = 0;
    __syncthreads();
    if (lane == 0) atomicMax(&s_max, wmax);
    __syncthreads();
    const int tmax = s_max;

    float ox = 0.0f, oy = 0.0f, oz = 0.0f;       // forward: the running image
    float gx = 0.0f, gy = 0.0f, gz = 0.0f, total = 0.0f, P = 0.0f;
    if (BWD && inside && nc > 0) {
        gx = g_in[3 * pix]; gy = g_in[3 * pix + 1]; gz = g_in[3 * pix + 2];
        total = (gx * img[3 * pix] + gy * img[3 * pix + 1]) + gz * img[3 * pix + 2];
    }
    const float half_w = 0.5f * (float)f.W, half_h = 0.5f * (float)f.H;

    // backward: the sums of the wave's value tile, entry slots [0, ns), added to the accumulator records and the normals' rows
    auto flush = [&](int ns) {
        wave_lds_sync();
        float v = 0.0f;
        if (lane < 2 * ROWS) {
            const float *row = &s_v[BWD ? wv : 0][(lane % ROWS) * PITCH + (lane / ROWS) * 32];
#pragma unroll
            for (int j = 0; j < 32; ++j) v += row[j]; // rows of slots from ns on hold stale values: never added
        }
        v += __shfl_down(v, ROWS, 64); // pixels 0-31 + pixels 32-63
        if (lane < ROWS) s_red[wv][lane] = v;
        wave_lds_sync();
        if (lane < ROWS) {
            const int slot = lane / VALS, k = lane % VALS;
            if (slot < ns) {
                const float4 c = s_con[wv][slot];
                const float *r = &s_red[wv][slot * VALS];
                const size_t id = (size_t)__float_as_int(c.w); // in [0, N): only a staged, applied entry is filed
                float out;
                if (k == 0) out = (2.0f * c.x * r[0] + c.y * r[1]) * half_w;
                else if (k == 1) out = (2.0f * c.z * r[1] + c.y * r[0]) * half_h;
                else if (k < 5) out = -0.5f * r[k];
                else out = r[k];
                // ONE atomic instruction for the wave's 27 lanes, whichever array a lane's value goes to: an atomic wave-instruction has a
                // fixed issue price, and one per destination array and column group was five of them per flush
                float *dst = k < 6 ? &acc[id * 16 + acc_column(k)] : &dnorm[id * 3 + (k - 6)];
                atomicAdd(dst, out);
            }
        }
        wave_lds_sync();
    };

    float T = 1.0f;
    int ns = 0;
    for (int base = 0; base < tmax; base += BATCH) {
        __syncthreads(); // every wave has walked the last batch
        const int cnt = min(BATCH, tmax - base);
        if (tid < cnt) {
            const long long at = start + base + tid; // < start + tmax <= end <= D
            const int id = f.point_list[at];
            float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra; // an id outside [0, N): opacity 0, never applied
            if (id >= 0 && (long long)id < f.N) {
                const float *pxy = f.xy + (size_t)id * f.xy_stride, *pco = f.co + (size_t)id * f.co_stride, *pn = normals + (size_t)id * 3;
                ra = make_float4(pxy[0], pxy[1], -0.5f * pco[0], -pco[1]);
                rb = make_float4(-0.5f * pco[2], pco[3], __int_as_float(id), 0.f);
                rc = make_float4(pn[0], pn[1], pn[2], 0.f);
            }
            s_rec[tid][0] = ra;
            s_rec[tid][1] = rb;
            s_rec[tid][2] = rc;
            s_mask[tid] = f.masks ? f.masks[at] : (uint8_t)0xFF;
        }
        __syncthreads();
        int n = 0;
        for (int gb = 0; gb < cnt; gb += 64) {
            const int e = gb + lane;
            const bool hit = e < cnt && base + e < wmax && (s_mask[e] & my_bits) != 0;
            const unsigned long long bits = __ballot(hit);
            if (hit) s_list[wv][n + __popcll(bits & lt_mask)] = (uint16_t)e;
            n += __popcll(bits);
        }
        if (lane < 2) s_list[wv][n + lane] = 0; // the walk reads two list entries ahead; entry 0 of a batch always exists
        wave_lds_sync();
        // one-deep software pipeline: the record of entry k + 1 and the list slot of entry k + 2 are in flight while entry k is weighed
        int e = s_list[wv][0], e1 = s_list[wv][1];
        float4 ra = s_rec[e][0], rb = s_rec[e][1], rc = s_rec[e][2];
        for (int k = 0; k < n; ++k) {
            const int e2 = s_list[wv][k + 2];
            const float4 na = s_rec[e1][0], nb = s_rec[e1][1], nn = s_rec[e1][2];
            const float dx = ra.x - pixf_x, dy = ra.y - pixf_y;
            const float power = (ra.z * dx * dx + rb.x * dy * dy) + ra.w * dx * dy;
            const float G = fast_exp(power);
            const float alpha = fminf(0.99f, rb.y * G);
            const float t = power > 0.0f ? 0.0f : alpha;
            const bool applied = base + e < nc && !(t < (1.0f / 255.0f));
            if (BWD) {
                if (__builtin_amdgcn_ballot_w64(applied) != 0ull) {
                    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f, v5 = 0.f, v6 = 0.f, v7 = 0.f, v8 = 0.f;
                    if (applied) {
                        const float u = (gx * rc.x + gy * rc.y) + gz * rc.z;
                        const float w = t * T;
                        P = P + w * u;
                        const float R = total - P;
                        const float om = 1.0f - t;
                        const float q = T * u - R / om;
                        const float gd = G * q;
                        const float h = rb.y * gd;
                        const float hx = h * dx, hy = h * dy;
                        v0 = hx; v1 = hy; v2 = hx * dx; v3 = hx * dy; v4 = hy * dy; v5 = gd;
                        v6 = w * gx; v7 = w * gy; v8 = w * gz;
                        T = T * om;
                    }
                    float *col = &s_v[BWD ? wv : 0][ns * VALS * PITCH + lane];
                    col[0 * PITCH] = v0; col[1 * PITCH] = v1; col[2 * PITCH] = v2; col[3 * PITCH] = v3; col[4 * PITCH] = v4;
                    col[5 * PITCH] = v5; col[6 * PITCH] = v6; col[7 * PITCH] = v7; col[8 * PITCH] = v8;
                    if (lane == 0) s_con[wv][ns] = make_float4(ra.z, ra.w, rb.x, rb.z);
                    if (++ns == SLOTS) {
                        flush(SLOTS);
                        ns = 0;
                    }
                }
            } else if (applied) {
                const float w = t * T;
                T = T * (1.0f - t);
                ox = __builtin_fmaf(w, rc.x, ox);
                oy = __builtin_fmaf(w, rc.y, oy);
                oz = __builtin_fmaf(w, rc.z, oz);
            }
            e = e1; e1 = e2;
            ra = na; rb = nb; rc = nn;
        }
    }
    if (BWD) {
        if (ns > 0) flush(ns);
    } else if (inside) {
        img[3 * pix] = ox; img[3 * pix + 1] = oy; img[3 * pix + 2] = oz;
    }
}

// ---- (e): the consistency term ----
constexpr int LOSS_MAX_BLOCKS = 2048;   // <= GSR_NORMALS_MAX_BLOCKS, and ceil(P / 256) <= that header's 32x8 tile count: its workspace holds the records

__global__ __launch_bounds__(GSR_SUM_THREADS) void consistency_kernel(long long npix, const float *__restrict__ Nimg, const float *__restrict__ nd,
                                                                      const float *__restrict__ valid, const float *__restrict__ m, float c,
                                                                      float *__restrict__ gN, float *__restrict__ gnd, double *__restrict__ part)
{
    __shared__ double s_red[GSR_SUM_WAVES][2];
    double s[2] = {0.0, 0.0};
    const float min2 = GSR_NORMAL_RENDER_MIN_LENGTH * GSR_NORMAL_RENDER_MIN_LENGTH;
    for (long long p = (long long)blockIdx.x * GSR_SUM_THREADS + threadIdx.x; p < npix; p += (long long)gridDim.x * GSR_SUM_THREADS) {
        const float Nx = Nimg[3 * p], Ny = Nimg[3 * p + 1], Nz = Nimg[3 * p + 2];
        const float L2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
        float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (valid[p] != 0.0f && L2 >= min2) {
            const float mm = m ? m[p] : 1.0f;
            const float len = __fsqrt_rn(L2);
            const float th[3] = {__fdiv_rn(Nx, len), __fdiv_rn(Ny, len), __fdiv_rn(Nz, len)};
            const float d[3] = {nd[3 * p], nd[3 * p + 1], nd[3 * p + 2]};
            const float dot = (d[0] * th[0] + d[1] * th[1]) + d[2] * th[2];
            const float km = c * mm;
            s[0] += (double)(mm * (1.0f - dot));
            s[1] += (double)mm;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                o[j] = -__fdiv_rn(km * (d[j] - th[j] * dot), len);
                o[3 + j] = -(km * th[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            gN[3 * p + j] = o[j];
            gnd[3 * p + j] = o[3 + j];
        }
    }
    const GsrBlockSums<double, 2> b = gsr_block_sums<GSR_SUM_THREADS>(s, s_red);
    if (threadIdx.x < 2) part[2 * (size_t)blockIdx.x + threadIdx.x] = b.pairwise(threadIdx.x);
}

// one workgroup: the record walk, the same tree, the two totals rounded once
__global__ __launch_bounds__(GSR_SUM_THREADS) void consistency_finish_kernel(const double *__restrict__ part, int n, float *__restrict__ sums)
{
    __shared__ double s_red[GSR_SUM_WAVES][2];
    GsrLaneSums<double, 2> s = gsr_record_walk<2, 2>(part, n);
    const GsrBlockSums<double, 2> b = gsr_block_sums<GSR_SUM_THREADS>(s.v, s_red);
    if (threadIdx.x < 2) sums[threadIdx.x] = (float)b.pairwise(threadIdx.x);
}

// NULL, DIMS, ALIGN, in the header's order; GSR_OK when the call may be enqueued
int check_frame(const GsrFeaturesFrame *fr, const void *a, const void *b, const void *c, const void *d, const void *e)
{
    if (!fr || !fr->xy || !fr->conic_opacity || !fr->ranges || !fr->n_contrib || !a || !b || !c || !d || !e) return GSR_E_NULL;
    if (!fr->point_list && fr->D > 0) return GSR_E_NULL;
    if (fr->W < 1 || fr->H < 1 || fr->W > GSR_FEATURES_MAX_SIDE || fr->H > GSR_FEATURES_MAX_SIDE || fr->N < 1 || fr->N > 0x7FFFFFFFll || fr->D < 0 ||
        fr->D > GSR_MAX_RENDERED || fr->xy_stride < 2 || fr->conic_opacity_stride < 4)
        return GSR_E_DIMS;
    if (!gsr_aligned4(fr->xy) || !gsr_aligned4(fr->conic_opacity) || !gsr_aligned4(fr->point_list) || !gsr_aligned4(fr->ranges) ||
        !gsr_aligned4(fr->n_contrib) || !gsr_aligned16(a) || !gsr_aligned16(b) || !gsr_aligned16(c) || !gsr_aligned16(d) || !gsr_aligned16(e))
        return GSR_E_ALIGN;
    return GSR_OK;
}

int check_gaussians(int64_t N, const float *scales, const float *rots, const float *means, const float *view, const void *a, const void *b)
{
    if (!scales || !rots || !means || !view || !a || !b) return GSR_E_NULL;
    if (N < 1 || N > 0x7FFFFFFFll) return GSR_E_DIMS;
    for (int k = 0; k < 16; ++k)
        if (!isfinite(view[k])) return GSR_E_DIMS;
    if (!gsr_aligned16(scales) || !gsr_aligned16(rots) || !gsr_aligned16(means) || !gsr_aligned16(a) || !gsr_aligned16(b)) return GSR_E_ALIGN;
    return GSR_OK;
}

FrameK frame_k(const GsrFeaturesFrame *fr)
{
    FrameK k;
    k.W = fr->W; k.H = fr->H; k.grid_x = (fr->W + 15) / 16;
    k.N = fr->N; k.D = fr->point_list ? fr->D : 0;
    k.xy = fr->xy; k.xy_stride = fr->xy_stride;
    k.co = fr->conic_opacity; k.co_stride = fr->conic_opacity_stride;
    k.point_list = fr->point_list; k.ranges = fr->ranges; k.n_contrib = fr->n_contrib; k.masks = fr->block_masks;
    return k;
}

ViewK view_k(const float *view)
{
    ViewK v;
    for (int k = 0; k < 16; ++k) v.v[k] = view[k];
    return v;
}

} // namespace

extern "C" int gsr_gaussian_normals(int64_t N, const float *scales, const float *rotations, const float *means, const float *viewmatrix,
                                    float *normals, void *stream)
{
    const int rc = check_gaussians(N, scales, rotations, means, viewmatrix, normals, normals);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL((gaussian_normals_kernel<false>), dim3((unsigned)gsr_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, (long long)N, scales,
                       rotations, means, view_k(viewmatrix), nullptr, normals);
    return gsr_done();
}

extern "C" int gsr_gaussian_normals_backward(int64_t N, const float *scales, const float *rotations, const float *means, const float *viewmatrix,
                                             const float *dL_dnormals, float *dL_drot, void *stream)
{
    const int rc = check_gaussians(N, scales, rotations, means, viewmatrix, dL_dnormals, dL_drot);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL((gaussian_normals_kernel<true>), dim3((unsigned)gsr_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, (long long)N, scales,
                       rotations, means, view_k(viewmatrix), dL_dnormals, dL_drot);
    return gsr_done();
}

extern "C" int gsr_normal_render_forward(const GsrFeaturesFrame *frame, const float *normals, float *out, void *stream)
{
    const int rc = check_frame(frame, normals, out, out, out, out);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    const int tiles = k.grid_x * ((k.H + 15) / 16);
    // a frame with D = 0 walks nothing: every pixel is written as 0
    hipLaunchKernelGGL((normal_render_kernel<false>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, k, normals, nullptr, out, nullptr, nullptr);
    return gsr_done();
}

extern "C" int gsr_normal_render_backward(const GsrFeaturesFrame *frame, const float *normals, const float *dL_dout, const float *out,
                                          float *accumulators, float *dL_dnormals, void *stream)
{
    const int rc = check_frame(frame, normals, dL_dout, out, accumulators, dL_dnormals);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (hipMemsetAsync(dL_dnormals, 0, sizeof(float) * 3 * (size_t)k.N, (hipStream_t)stream) != hipSuccess) return GSR_E_HIP;
    if (k.D == 0) return gsr_done(); // nothing was blended: nothing to add
    const int tiles = k.grid_x * ((k.H + 15) / 16);
    hipLaunchKernelGGL((normal_render_kernel<true>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, k, normals, dL_dout, const_cast<float *>(out),
                       accumulators, dL_dnormals);
    return gsr_done();
}

extern "C" int gsr_normal_consistency_loss(const float *Nimg, const float *n_d, const float *valid, const float *m, int32_t W, int32_t H, float weight,
                                           float *gN, float *gnd, float *sums, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!Nimg || !n_d || !valid || !gN || !gnd || !sums || !workspace) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H) || !isfinite(weight)) return GSR_E_DIMS;
    if (!gsr_aligned16(Nimg) || !gsr_aligned16(n_d) || !gsr_aligned16(valid) || !gsr_aligned16(m) || !gsr_aligned16(gN) || !gsr_aligned16(gnd) ||
        !gsr_aligned4(sums) || !gsr_aligned16(workspace))
        return GSR_E_ALIGN;
    if (workspace_bytes < gsr_normals_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    const long long npix = (long long)W * H;
    const int nb = (int)gsr_record_count(npix, GSR_SUM_THREADS, LOSS_MAX_BLOCKS);
    const float c = (float)((double)weight / ((double)W * (double)H));
    double *part = static_cast<double *>(workspace);
    hipLaunchKernelGGL(consistency_kernel, dim3(nb), dim3(GSR_SUM_THREADS), 0, (hipStream_t)stream, npix, Nimg, n_d, valid, m, c, gN, gnd, part);
    hipLaunchKernelGGL(consistency_finish_kernel, dim3(1), dim3(GSR_SUM_THREADS), 0, (hipStream_t)stream, part, nb, sums);
    return gsr_done();
}
