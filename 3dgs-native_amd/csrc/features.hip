// features.hip -- N-channel feature rendering over a frame's lists, and its transpose (include/gsr_features.h), for gfx950.
//
// Both directions replay the forward blend's weights w_k(p) from the frame's buffers and are matrix products per tile:
//     forward    out[p][c]   = sum_k w_k(p) F[i_k][c]       pixels x entries x channels
//     backward   dL_dF[i][c] = sum_p w_i(p) G[p][c]         entries x pixels x channels
// One 256-thread workgroup per 16x16 tile, each of its four waves owning one 8x8 pixel block (lane = pixel), as in blend_fwd.hip.
// The tile's list is staged through LDS in batches of 256 entries (32 bytes each: position, pre-scaled conic, opacity, id).  A wave
// compacts the batch to the entries its block may see (the forward's 8x4-block masks when the caller has them, every entry below
// the block's largest n_contrib otherwise), walks them with lane = pixel -- the weight expression of blend_fwd.hip:307, restated
// here -- and files the weights of every entry that some pixel of the block applies as one column of a 64 x 32 tile in LDS.
// Every 32 columns the tile is multiplied on the matrix cores with v_mfma_f32_32x32x2_f32, which is exact float32: its result is
// bit for bit a k-ordered fmaf chain, so
//   - the forward's sum per pixel is one fused multiply-add per entry in list order (k = the tile's columns, in list order), the
//     accumulators -- 64 pixels x 32 or 64 channels -- staying in registers over the whole list; no atomics, the same bits every
//     call and with or without masks (a column is filed only when some pixel applies the entry; a column of zeros adds nothing);
//   - the backward sums the block's 64 pixels inside the MFMA's K (G's fragments stay in registers over the whole list) and adds
//     one row of 4 C bytes per (8x8 block, applied entry) with float atomics: lanes 0-31 and 32-63 of an accumulator register are
//     two rows' consecutive channels, the shape the atomic unit takes at full rate for C = 32 and above.
// Channels are padded to 32 (C <= 32) or 64 inside the registers only; F, G and the outputs are read and written as C wide.
#include <algorithm>

#include "gsr_internal.h"
#include "gsr_features.h"

namespace {

constexpr int BATCH = 256;   // list entries staged per round
constexpr int SLOTS = 32;    // columns of a wave's weight tile: one MFMA row / K block
constexpr int PITCH = 33;    // floats per pixel row of the weight tile: odd, so column writes and row reads both spread over the banks

typedef float f32x16 __attribute__((ext_vector_type(16)));

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

__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); } // blend_fwd.hip's

// lanes of one wave exchange data through LDS: in order in hardware, but the compiler must not move the accesses across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// row of a 32x32 accumulator held in register r of lane `lane` (its column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// NCB: 32-channel blocks in registers (1 or 2).  BWD: `in` is G [H][W][C] and `out` dL_dF [N][C] (cleared by the caller), else `in`
// is F [N][C] and `out` the image [H][W][C].
template <int NCB, bool BWD>
__global__ __launch_bounds__(256) void features_kernel(FrameK f, int C, const float *__restrict__ in, float *__restrict__ out)
{
    __shared__ float4 s_rec[BATCH][2];    // {x, y, a', b'} {c', opacity, id, -}
    __shared__ uint8_t s_mask[BATCH];
    __shared__ uint16_t s_list[4][BATCH + 2]; // per wave: the batch entries its block may see, in list order (+ two the walk reads ahead)
    __shared__ float s_w[4][64 * PITCH];  // per wave: weights [pixel][column]
    __shared__ int s_id[4][SLOTS];        // per wave: Gaussian of each column
    __shared__ int s_max;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = blockIdx.x;
    const int tile_x = tile % f.grid_x, tile_y = tile / f.grid_x;
    const int bx0 = tile_x * 16 + (wv & 1) * 8, by0 = tile_y * 16 + (wv >> 1) * 8; // this wave's 8x8 block; pixel q of it = (q & 7, q >> 3)
    const int pix_x = bx0 + (lane & 7), pix_y = by0 + (lane >> 3);
    const bool inside = pix_x < f.W && pix_y < f.H;
    const float pixf_x = (float)pix_x, pixf_y = (float)pix_y;
    const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int my_bits = 5 << ((wv >> 1) * 4 + (wv & 1)); // this wave's 8x8 block = the 8x4 blocks k0 and k0 + 2 (blend_fwd.hip)
    const int col = lane & 31, hi = lane >> 5;

    // the walk's bounds: the range clipped to [0, D], n_contrib to the range
    long long start = f.ranges[2 * tile], end = f.ranges[2 * tile + 1];
    start = std::min(std::max(start, 0ll), f.D);
    end = std::min(std::max(end, start), f.D);
    const int len = (int)(end - start);
    int nc = 0;
    if (inside) nc = std::min(std::max(f.n_contrib[(size_t)pix_y * f.W + pix_x], 0), len);
    int wmax = nc;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, __shfl_xor(wmax, d, 64));
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    if (tid == 0) s_max = 0;
    __syncthreads();
    if (lane == 0) atomicMax(&s_max, wmax);
    __syncthreads();
    const int tmax = s_max;

    // backward: G of this wave's block as the B operands of its 32 K steps (pixels 2 s and 2 s + 1), zero off the image and past C
    float g[NCB][32];
    f32x16 acc[BWD ? 1 : 2][NCB]; // forward: [pixel half][channel block], over the whole list; backward: per product, [0][channel block]
    if (BWD) {
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const int q = 2 * s + hi, qx = bx0 + (q & 7), qy = by0 + (q >> 3);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const int ch = 32 * cb + col;
                g[cb][s] = (wmax > 0 && qx < f.W && qy < f.H && ch < C) ? in[((size_t)qy * f.W + qx) * C + ch] : 0.0f;
            }
        }
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][cb][r] = 0.0f;
    }

    // the product of the wave's weight tile, columns [0, ns)
    auto flush = [&](int ns) {
        wave_lds_sync();
        if (BWD) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][cb][r] = 0.0f;
            // D[column][channel] += W^T[column][pixel] G[pixel][channel], K = the 64 pixels in order; columns from ns on hold stale
            // weights: their rows are never added
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                const float a = s_w[wv][(2 * s + hi) * PITCH + col];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) acc[0][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, g[cb][s], acc[0][cb], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int slot = acc_row(r, lane);
                if (slot < ns) {
                    const int id = s_id[wv][slot];
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) {
                        const int ch = 32 * cb + col;
                        if (ch < C) atomicAdd(&out[(size_t)id * C + ch], acc[0][cb][r]);
                    }
                }
            }
        } else {
            // D[pixel][channel] += W[pixel][column] F[id of column][channel], K = the columns in list order.  A full tile runs its 16
            // K steps, the last, partial one the (ns + 1) / 2 steps it has (in an odd ns the missing column enters as zeros on both
            // sides); the call with ns = SLOTS is inlined with the guards folded away, the gathers of F in flight together
            auto k_step = [&](int s) {
                const int slot = 2 * s + hi;
                const bool live = slot < ns;
                const int id = live ? s_id[wv][slot] : 0;
                float b[NCB];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const int ch = 32 * cb + col;
                    b[cb] = (live && ch < C) ? in[(size_t)id * C + ch] : 0.0f;
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float w = s_w[wv][(32 * h + col) * PITCH + slot];
                    const float a = live ? w : 0.0f;
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) acc[h][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[cb], acc[h][cb], 0, 0, 0);
                }
            };
#pragma unroll
            for (int s = 0; s < SLOTS / 2; ++s)
                if (2 * s < ns) k_step(s); // wave-uniform
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
                rb = make_float4(-0.5f * pco[2], pco[3], __int_as_float(id), 0.f);
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
            const float alpha = fminf(0.99f, rb.y * fast_exp(power));
            const float t = power > 0.0f ? 0.0f : alpha;
            const bool applied = base + e < nc && !(t < (1.0f / 255.0f));
            if (__builtin_amdgcn_ballot_w64(applied) != 0ull) {
                const float w = applied ? t * T : 0.0f;
                T = applied ? T * (1.0f - t) : T;
                s_w[wv][lane * PITCH + ns] = w;
                if (lane == 0) s_id[wv][ns] = __float_as_int(rb.z);
                if (++ns == SLOTS) {
                    flush(SLOTS);
                    ns = 0;
                }
            }
            e = e1; e1 = e2;
            ra = na; rb = nb;
        }
    }
    if (ns > 0) flush(ns);

    if (!BWD) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = 32 * h + acc_row(r, lane), qx = bx0 + (q & 7), qy = by0 + (q >> 3);
                if (qx < f.W && qy < f.H) {
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) {
                        const int ch = 32 * cb + col;
                        if (ch < C) out[((size_t)qy * f.W + qx) * C + ch] = acc[h][cb][r];
                    }
                }
            }
    }
}

// NULL, DIMS, ALIGN, in the header's order; GSR_OK when the call may be enqueued
int check(const GsrFeaturesFrame *fr, int32_t C, const void *a, const void *b)
{
    if (!fr || !fr->xy || !fr->conic_opacity || !fr->ranges || !fr->n_contrib || !a || !b) return GSR_E_NULL;
    if (!fr->point_list && fr->D > 0) return GSR_E_NULL;
    if (fr->W < 1 || fr->H < 1 || fr->W > GSR_FEATURES_MAX_SIDE || fr->H > GSR_FEATURES_MAX_SIDE || fr->N < 1 || fr->N > 0x7FFFFFFFll || fr->D < 0 ||
        fr->D > GSR_MAX_RENDERED || fr->xy_stride < 2 || fr->conic_opacity_stride < 4 || C < 1 || C > GSR_FEATURES_MAX_CHANNELS)
        return GSR_E_DIMS;
    if (!gsr_aligned4(fr->xy) || !gsr_aligned4(fr->conic_opacity) || !gsr_aligned4(fr->point_list) || !gsr_aligned4(fr->ranges) ||
        !gsr_aligned4(fr->n_contrib) || !gsr_aligned16(a) || !gsr_aligned16(b))
        return GSR_E_ALIGN;
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

template <bool BWD>
void launch(const FrameK &k, int C, const float *in, float *out, hipStream_t s)
{
    const int tiles = k.grid_x * ((k.H + 15) / 16);
    if (C <= 32)
        hipLaunchKernelGGL((features_kernel<1, BWD>), dim3(tiles), dim3(256), 0, s, k, C, in, out);
    else
        hipLaunchKernelGGL((features_kernel<2, BWD>), dim3(tiles), dim3(256), 0, s, k, C, in, out);
}

} // namespace

extern "C" int gsr_features_forward(const GsrFeaturesFrame *frame, int32_t C, const float *features, float *out, void *stream)
{
    const int rc = check(frame, C, features, out);
    if (rc != GSR_OK) return rc;
    launch<false>(frame_k(frame), C, features, out, (hipStream_t)stream); // a frame with D = 0 walks nothing: every pixel is written as 0
    return gsr_done();
}

extern "C" int gsr_features_backward(const GsrFeaturesFrame *frame, int32_t C, const float *dL_dout, float *dL_dF, void *stream)
{
    const int rc = check(frame, C, dL_dout, dL_dF);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (hipMemsetAsync(dL_dF, 0, sizeof(float) * (size_t)k.N * (size_t)C, (hipStream_t)stream) != hipSuccess) return GSR_E_HIP;
    if (k.D > 0) launch<true>(k, C, dL_dout, dL_dF, (hipStream_t)stream);
    return gsr_done();
}
