// median_depth.hip -- the median inverse depth over a frame's lists, and its gradient (include/gsr_median_depth.h), for gfx950.
//
//   - forward: frame_walk.h's FrameWalk with its early exit.  The staged record's spare float carries 1/depth, as in distortion.hip;
//     T, the chosen 1/depth and its list position live in three registers per lane.  A pixel is finished once T <= 0.5, usually
//     within the first batch, so the workgroup leaves the list as soon as none of its pixels is open.  No LDS beyond the staging, no
//     atomics: the same bits every call and with or without masks.
//   - backward: no walk.  One wave per 8x8 block, lane = pixel; the wave loops over the distinct Gaussians its pixels chose, sums
//     dL_dmedian over each one's pixels in the header's fixed order through one 64-float LDS row, and adds the sum to column 11 of the
//     Gaussian's accumulator record with one atomic.
#include "frame_walk.h"
#include "gsr_median_depth.h"

namespace {

__global__ __launch_bounds__(256) void median_depth_kernel(FrameK f, const float *__restrict__ invd, long long invd_stride, float *__restrict__ med_out,
                                                           int32_t *__restrict__ contrib_out)
{
    const FrameWalk walk(f);
    float T = 1.0f, med = 0.0f;
    int c = 0;
    walk.run<2>(
        f, [&](int id, float4 &rb) { rb.w = invd[(size_t)id * invd_stride]; },
        [&](const float4 &ra, const float4 &rb, float dx, float dy, float G, float t, bool applied, int pos) {
            if (applied) {
                if (T > 0.5f) {
                    med = rb.w;
                    c = pos;
                }
                T = T * (1.0f - t);
            }
        },
        [&] { return T > 0.5f; });
    if (walk.inside) {
        med_out[walk.pix] = med;
        contrib_out[walk.pix] = c;
    }
}

// The forward's geometry without its walk: workgroup = tile, wave = 8x8 block, lane = pixel.
__global__ __launch_bounds__(256) void median_depth_backward_kernel(FrameK f, const float *__restrict__ g_in, const int32_t *__restrict__ contrib,
                                                                    float *__restrict__ acc)
{
    __shared__ float s_g[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = blockIdx.x;
    const int tile_x = tile % f.grid_x, tile_y = tile / f.grid_x;
    const int pix_x = tile_x * 16 + (wv & 1) * 8 + (lane & 7), pix_y = tile_y * 16 + (wv >> 1) * 8 + (lane >> 3);
    // the tile's range clipped to [0, D], the position to the range, the id to [0, N): frame_walk.h's bounds
    long long start = f.ranges[2 * tile], end = f.ranges[2 * tile + 1];
    start = std::min(std::max(start, 0ll), f.D);
    end = std::min(std::max(end, start), f.D);
    int id = -1;
    float g = 0.0f;
    if (pix_x < f.W && pix_y < f.H) {
        const size_t pix = (size_t)pix_y * f.W + pix_x;
        const int c = std::min(std::max(contrib[pix], 0), (int)(end - start));
        if (c > 0) {
            id = f.point_list[start + c - 1]; // start + c - 1 < end <= D
            if ((long long)id >= f.N) id = -1;
            g = g_in[pix];
        }
    }
    // every lane follows the loop; a lane without a Gaussian, or with g = 0, adds nothing (its g is 0, or it matches no id)
    unsigned long long todo = __builtin_amdgcn_ballot_w64(id >= 0);
    while (todo != 0ull) {
        const int leader = __builtin_ctzll(todo);
        const int cur = __builtin_amdgcn_readlane(id, leader);
        const bool match = id == cur;
        s_g[wv][lane] = match ? g : 0.0f;
        wave_lds_sync();
        float sum = 0.0f;
        if (lane < 2) {
            const float *row = &s_g[wv][lane * 32];
#pragma unroll
            for (int j = 0; j < 32; ++j) sum += row[j];
        }
        sum += __shfl_down(sum, 1, 64); // pixels 0-31 + pixels 32-63
        if (lane == 0 && sum != 0.0f) atomicAdd(&acc[(size_t)cur * 16 + 11], sum); // (a zero sum is not added: x + 0 is x, but for the sign of a zero)
        wave_lds_sync(); // the row is read before the next Gaussian's values overwrite it
        todo &= ~__builtin_amdgcn_ballot_w64(match);
    }
}

// NULL, DIMS, ALIGN, in the header's order; GSR_OK when the call may be enqueued
int check(const GsrDistortionFrame *fr, const void *a, const void *b, const void *c)
{
    if (frame_has_null(fr) || !fr->inv_depth || !a || !b || !c) return GSR_E_NULL;
    if (!frame_dims_ok(fr) || fr->inv_depth_stride < 1) return GSR_E_DIMS;
    if (!frame_aligned(fr) || !gsr_aligned4(fr->inv_depth) || !all_aligned16(a, b, c)) return GSR_E_ALIGN;
    return GSR_OK;
}

} // namespace

extern "C" int gsr_median_depth_forward(const GsrDistortionFrame *frame, float *median_inv_depth, int32_t *median_contrib, void *stream)
{
    const int rc = check(frame, median_inv_depth, median_contrib, median_contrib);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    // a frame with D = 0 walks nothing: every pixel is written as 0 / 0
    hipLaunchKernelGGL(median_depth_kernel, dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, frame->inv_depth,
                       (long long)frame->inv_depth_stride, median_inv_depth, median_contrib);
    return gsr_done();
}

extern "C" int gsr_median_depth_backward(const GsrDistortionFrame *frame, const float *dL_dmedian, const int32_t *median_contrib, float *accumulators,
                                         void *stream)
{
    const int rc = check(frame, dL_dmedian, median_contrib, accumulators);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (k.D == 0) return GSR_OK; // nothing was blended: nothing to add
    hipLaunchKernelGGL(median_depth_backward_kernel, dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, dL_dmedian, median_contrib, accumulators);
    return gsr_done();
}
