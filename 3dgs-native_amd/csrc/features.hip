// features.hip -- N-channel feature rendering over a frame's lists, and its transpose (include/gsr_features.h), for gfx950.
//
// Both directions replay the forward blend's weights w_k(p) from the frame's buffers and are matrix products per tile:
//     forward    out[p][c]   = sum_k w_k(p) F[i_k][c]       pixels x entries x channels
//     backward   dL_dF[i][c] = sum_p w_i(p) G[p][c]         entries x pixels x channels
// frame_walk.h's FrameWalk stages the tile's list, compacts it per wave and weighs each entry (lane = pixel); this file files the
// weights of every entry that some pixel of the block applies as one column of a 64 x 32 tile in LDS.
// Every 32 columns the tile is multiplied on the matrix cores with v_mfma_f32_32x32x2_f32, which is exact float32: its result is
// bit for bit a k-ordered fmaf chain, so
//   - the forward's sum per pixel is one fused multiply-add per entry in list order (k = the tile's columns, in list order), the
//     accumulators -- 64 pixels x 32 or 64 channels -- staying in registers over the whole list; no atomics, the same bits every
//     call and with or without masks (a column is filed only when some pixel applies the entry; a column of zeros adds nothing);
//   - the backward sums the block's 64 pixels inside the MFMA's K (G's fragments stay in registers over the whole list) and adds
//     one row of 4 C bytes per (8x8 block, applied entry) with float atomics: lanes 0-31 and 32-63 of an accumulator register are
//     two rows' consecutive channels, the shape the atomic unit takes at full rate for C = 32 and above.
// Channels are padded to 32 (C <= 32) or 64 inside the registers only; F, G and the outputs are read and written as C wide.
#include "frame_walk.h"

namespace {

constexpr int SLOTS = 32;    // columns of a wave's weight tile: one MFMA row / K block
constexpr int PITCH = 33;    // floats per pixel row of the weight tile: odd, so column writes and row reads both spread over the banks

typedef float f32x16 __attribute__((ext_vector_type(16)));

// row of a 32x32 accumulator held in register r of lane `lane` (its column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// NCB: 32-channel blocks in registers (1 or 2).  BWD: `in` is G [H][W][C] and `out` dL_dF [N][C] (cleared by the caller), else `in`
// is F [N][C] and `out` the image [H][W][C].
template <int NCB, bool BWD>
__global__ __launch_bounds__(256) void features_kernel(FrameK f, int C, const float *__restrict__ in, float *__restrict__ out)
{
    __shared__ float s_w[4][64 * PITCH];  // per wave: weights [pixel][column]
    __shared__ int s_id[4][SLOTS];        // per wave: Gaussian of each column
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6; // = walk.lane, walk.wv
    const int col = lane & 31, hi = lane >> 5;
    const FrameWalk walk(f);
    const int bx0 = walk.bx0, by0 = walk.by0, wmax = walk.wmax;

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
    walk.run<2>(
        f, [](int, float4 &) {},
        [&](const float4 &, const float4 &rb, float, float, float, float t, bool applied) {
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
        });
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
    if (frame_has_null(fr) || !a || !b) return GSR_E_NULL;
    if (!frame_dims_ok(fr) || C < 1 || C > GSR_FEATURES_MAX_CHANNELS) return GSR_E_DIMS;
    if (!frame_aligned(fr) || !all_aligned16(a, b)) return GSR_E_ALIGN;
    return GSR_OK;
}

template <bool BWD>
void launch(const FrameK &k, int C, const float *in, float *out, hipStream_t s)
{
    const int tiles = frame_tiles(k);
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
