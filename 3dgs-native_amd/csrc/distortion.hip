// distortion.hip -- the depth-distortion regulariser over a frame's lists, and its gradient (include/gsr_distortion.h), for gfx950.
//
// Both directions replay the forward blend's weights w_k(p) from the frame's buffers the way features.hip does: one 256-thread
// workgroup per 16x16 tile, each of its four waves owning one 8x8 pixel block (lane = pixel), the tile's list staged through LDS in
// batches of 256 entries (32 bytes each: position, pre-scaled conic, opacity, id, 1/depth), each wave compacting a batch to the
// entries its block may see and walking them with blend_forward_kernel's weight expression (power, alpha, the two skip tests).
//   - forward: the running sums A, mu, S of the header live in three registers per lane over the whole list.  No LDS beyond the
//     staging, no atomics, the same bits every call and with or without masks (an entry no pixel applies changes nothing).
//   - backward: a second front-to-back walk with the stored A, mu, S; the suffix sum of dL/dalpha is the stored total minus the
//     running prefix.  Each lane files its seven per-(pixel, entry) values as seven rows of a 28 x 64 tile in LDS (four entries per
//     tile); the flush sums each row with two lanes (32 pixels each, in order, then the two halves), applies the per-entry
//     constants once and adds the entry's seven columns to its accumulator record: blend_bwd_splat.hip's transposed flush, turned
//     round for lane = pixel.  Seven values cannot fill the 32 columns of an MFMA tile (features.hip's transpose would run at 7/32
//     of its rate and needs the values to factor into weight x image, which they do not), so the reduction is LDS reads and adds.
#include <algorithm>

#include "gsr_internal.h"
#include "gsr_distortion.h"

namespace {

constexpr int BATCH = 256;   // list entries staged per round
constexpr int SLOTS = 4;     // entries per flush of the backward
constexpr int VALS = 7;      // S1, S2, Sxx, Sxy, Syy, Sop, Sdm
constexpr int ROWS = SLOTS * VALS;
constexpr int PITCH = 65;    // floats per row of the value tile: odd, so the row-parallel reads of the flush spread over the 64 banks

struct FrameK {
    int W, H, grid_x;
    long long N, D;
    const float *xy;
    long long xy_stride;
    const float *co;
    long long co_stride;
    const float *invd;
    long long invd_stride;
    const int32_t *point_list;
    const int32_t *ranges;
    const int32_t *n_contrib;
    const uint8_t *masks;
};

__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); } // blend_fwd.hip's

// lanes of one wave exchange data through LDS: in order in hardware, but the compiler must not move the accesses across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// accumulator column of the k-th value the flush adds: dmean2D x y | dconic a b c | dopacity | d(1/depth)
__device__ __forceinline__ int acc_column(int k) { return k < 2 ? 3 + k : k < 4 ? 4 + k : k == 4 ? 9 : 5 + k; }

// BWD: `g_in` is dL_ddist [H][W], `mom` the forward's moments (read), `acc` the accumulator records; else `dist` and `mom` are written.
template <bool BWD>
__global__ __launch_bounds__(256) void distortion_kernel(FrameK f, const float *__restrict__ g_in, float *__restrict__ dist, float *mom,
                                                         float *__restrict__ acc)
{
    __shared__ float4 s_rec[BATCH][2];    // {x, y, a', b'} {c', opacity, id, 1/depth}
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

    float A = 0.0f, mu = 0.0f, S = 0.0f; // forward: running; backward: the stored totals
    float g = 0.0f, gA = 0.0f, total = 0.0f, P = 0.0f;
    if (BWD && inside && nc > 0) {
        const float4 mo = *reinterpret_cast<const float4 *>(mom + 4 * pix);
        A = mo.x; mu = mo.y; S = mo.z;
        g = g_in[pix];
        gA = g * A;
        total = 2.0f * (gA * S);
    }
    const float half_w = 0.5f * (float)f.W, half_h = 0.5f * (float)f.H;

    // backward: the sums of the wave's value tile, entry slots [0, ns), added to the accumulator records
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
                float out;
                if (k == 0) out = (2.0f * c.x * r[0] + c.y * r[1]) * half_w;
                else if (k == 1) out = (2.0f * c.z * r[1] + c.y * r[0]) * half_h;
                else if (k < 5) out = -0.5f * r[k];
                else out = r[k];
                const int id = __float_as_int(c.w); // in [0, N): only a staged, applied entry is filed
                atomicAdd(&acc[(size_t)id * 16 + acc_column(k)], out);
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
            float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra; // an id outside [0, N): opacity 0, never applied
            if (id >= 0 && (long long)id < f.N) {
                const float *pxy = f.xy + (size_t)id * f.xy_stride, *pco = f.co + (size_t)id * f.co_stride;
                ra = make_float4(pxy[0], pxy[1], -0.5f * pco[0], -pco[1]);
                rb = make_float4(-0.5f * pco[2], pco[3], __int_as_float(id), f.invd[(size_t)id * f.invd_stride]);
            }
            s_rec[tid][0] = ra;
            s_rec[tid][1] = rb;
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
        float4 ra = s_rec[e][0], rb = s_rec[e][1];
        for (int k = 0; k < n; ++k) {
            const int e2 = s_list[wv][k + 2];
            const float4 na = s_rec[e1][0], nb = s_rec[e1][1];
            const float dx = ra.x - pixf_x, dy = ra.y - pixf_y;
            const float power = (ra.z * dx * dx + rb.x * dy * dy) + ra.w * dx * dy;
            const float G = fast_exp(power);
            const float alpha = fminf(0.99f, rb.y * G);
            const float t = power > 0.0f ? 0.0f : alpha;
            const bool applied = base + e < nc && !(t < (1.0f / 255.0f));
            if (BWD) {
                if (__builtin_amdgcn_ballot_w64(applied) != 0ull) {
                    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f, v5 = 0.f, v6 = 0.f;
                    if (applied) {
                        const float w = t * T;
                        const float d = rb.w - mu;
                        const float u = (((A * d) * d) + S) * g;
                        P = P + w * u;
                        const float R = total - P;
                        const float om = 1.0f - t;
                        const float q = T * u - R / om;
                        const float gd = G * q;
                        const float h = rb.y * gd;
                        const float hx = h * dx, hy = h * dy;
                        v0 = hx; v1 = hy; v2 = hx * dx; v3 = hx * dy; v4 = hy * dy; v5 = gd;
                        v6 = ((2.0f * gA) * w) * d;
                        T = T * om;
                    }
                    float *col = &s_v[BWD ? wv : 0][ns * VALS * PITCH + lane];
                    col[0 * PITCH] = v0; col[1 * PITCH] = v1; col[2 * PITCH] = v2; col[3 * PITCH] = v3;
                    col[4 * PITCH] = v4; col[5 * PITCH] = v5; col[6 * PITCH] = v6;
                    if (lane == 0) s_con[wv][ns] = make_float4(ra.z, ra.w, rb.x, rb.z);
                    if (++ns == SLOTS) {
                        flush(SLOTS);
                        ns = 0;
                    }
                }
            } else if (applied) {
                const float w = t * T;
                T = T * (1.0f - t);
                const float A1 = A + w;
                const float d = rb.w - mu;
                const float r = w / A1;
                S = S + ((A * r) * d) * d;
                mu = mu + r * d;
                A = A1;
            }
            e = e1; e1 = e2;
            ra = na; rb = nb;
        }
    }
    if (BWD) {
        if (ns > 0) flush(ns);
    } else if (inside) {
        dist[pix] = A * S;
        *reinterpret_cast<float4 *>(mom + 4 * pix) = make_float4(A, mu, S, 0.0f);
    }
}

// NULL, DIMS, ALIGN, in the header's order; GSR_OK when the call may be enqueued
int check(const GsrDistortionFrame *fr, const void *a, const void *b, const void *c)
{
    if (!fr || !fr->xy || !fr->conic_opacity || !fr->inv_depth || !fr->ranges || !fr->n_contrib || !a || !b || !c) return GSR_E_NULL;
    if (!fr->point_list && fr->D > 0) return GSR_E_NULL;
    if (fr->W < 1 || fr->H < 1 || fr->W > GSR_FEATURES_MAX_SIDE || fr->H > GSR_FEATURES_MAX_SIDE || fr->N < 1 || fr->N > 0x7FFFFFFFll || fr->D < 0 ||
        fr->D > GSR_MAX_RENDERED || fr->xy_stride < 2 || fr->conic_opacity_stride < 4 || fr->inv_depth_stride < 1)
        return GSR_E_DIMS;
    if (!gsr_aligned4(fr->xy) || !gsr_aligned4(fr->conic_opacity) || !gsr_aligned4(fr->inv_depth) || !gsr_aligned4(fr->point_list) ||
        !gsr_aligned4(fr->ranges) || !gsr_aligned4(fr->n_contrib) || !gsr_aligned16(a) || !gsr_aligned16(b) || !gsr_aligned16(c))
        return GSR_E_ALIGN;
    return GSR_OK;
}

FrameK frame_k(const GsrDistortionFrame *fr)
{
    FrameK k;
    k.W = fr->W; k.H = fr->H; k.grid_x = (fr->W + 15) / 16;
    k.N = fr->N; k.D = fr->point_list ? fr->D : 0;
    k.xy = fr->xy; k.xy_stride = fr->xy_stride;
    k.co = fr->conic_opacity; k.co_stride = fr->conic_opacity_stride;
    k.invd = fr->inv_depth; k.invd_stride = fr->inv_depth_stride;
    k.point_list = fr->point_list; k.ranges = fr->ranges; k.n_contrib = fr->n_contrib; k.masks = fr->block_masks;
    return k;
}

} // namespace

extern "C" int gsr_distortion_forward(const GsrDistortionFrame *frame, float *dist, float *moments, void *stream)
{
    const int rc = check(frame, dist, moments, moments);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    const int tiles = k.grid_x * ((k.H + 15) / 16);
    // a frame with D = 0 walks nothing: every pixel is written as 0
    hipLaunchKernelGGL((distortion_kernel<false>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, k, nullptr, dist, moments, nullptr);
    return gsr_done();
}

extern "C" int gsr_distortion_backward(const GsrDistortionFrame *frame, const float *dL_ddist, const float *moments, float *accumulators,
                                       void *stream)
{
    const int rc = check(frame, dL_ddist, moments, accumulators);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (k.D == 0) return GSR_OK; // nothing was blended: nothing to add
    const int tiles = k.grid_x * ((k.H + 15) / 16);
    hipLaunchKernelGGL((distortion_kernel<true>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, k, dL_ddist, nullptr,
                       const_cast<float *>(moments), accumulators);
    return gsr_done();
}
