// plane_median.hip -- the ray-plane intersection depth under the median rule over a frame's lists, and its gradient into the plane
// moments (include/gsr_plane_median.h), for gfx950.
//
//   - forward: median_depth.hip's walk (frame_walk.h's FrameWalk with its early exit) over plane_depth.hip's 48-byte staged records:
//     1 / depth in the spare float of the second word, the two slopes in the third.  Two fused multiply-adds and a clamp per entry for
//     m; T, the chosen m and its list position live in three registers per lane.  No LDS beyond the staging, no atomics: the same
//     bits every call and with or without masks.
//   - backward: no walk.  median_depth.hip's geometry: one wave per 8x8 block, lane = pixel.  Each lane gathers its chosen Gaussian's
//     staged xy, 1 / depth and slopes, repeats the forward's clamp decision and holds (g, g (-dx), g (-dy)), zeros where clamped; the
//     wave loops over the distinct Gaussians its pixels chose, sums the three values over each one's pixels in the header's fixed
//     order through three 64-float LDS rows, and adds the three sums to the Gaussian's row of dL_dplane_moments with one atomic
//     wave-instruction.
#include "frame_walk.h"
#include "gsr_plane_median.h"

namespace {

constexpr int VALS = 3; // S0, Sx, Sy: the Gaussian's row of dL_dplane_moments

__global__ __launch_bounds__(256) void plane_median_kernel(FrameK f, const float *__restrict__ invd, long long invd_stride, const float *__restrict__ slopes,
                                                           float *__restrict__ med_out, int32_t *__restrict__ contrib_out)
{
    const FrameWalk walk(f);
    float T = 1.0f, med = 0.0f;
    int c = 0;
    walk.run<3>(
        f,
        [&](int id, float4 &rb, float4 &rc) {
            rb.w = invd[(size_t)id * invd_stride];
            const float2 sl = *reinterpret_cast<const float2 *>(slopes + (size_t)id * 2);
            rc = make_float4(sl.x, sl.y, 0.f, 0.f);
        },
        [&](const float4 &ra, const float4 &rb, const float4 &rc, float dx, float dy, float G, float t, bool applied, int pos) {
            if (applied) {
                if (T > 0.5f) {
                    const float mr = __builtin_fmaf(-rc.x, dx, __builtin_fmaf(-rc.y, dy, rb.w));
                    med = fminf(fmaxf(mr, rb.w * 0.25f), rb.w * GSR_PLANE_DEPTH_MAX_RATIO);
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
__global__ __launch_bounds__(256) void plane_median_backward_kernel(FrameK f, const float *__restrict__ invd, long long invd_stride,
                                                                    const float *__restrict__ slopes, const float *__restrict__ g_in,
                                                                    const int32_t *__restrict__ contrib, float *__restrict__ dmom)
{
    __shared__ float s_v[4][VALS][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = blockIdx.x;
    const int tile_x = tile % f.grid_x, tile_y = tile / f.grid_x;
    const int pix_x = tile_x * 16 + (wv & 1) * 8 + (lane & 7), pix_y = tile_y * 16 + (wv >> 1) * 8 + (lane >> 3);
    // the tile's range clipped to [0, D], the position to the range, the id to [0, N): frame_walk.h's bounds
    long long start = f.ranges[2 * tile], end = f.ranges[2 * tile + 1];
    start = std::min(std::max(start, 0ll), f.D);
    end = std::min(std::max(end, start), f.D);
    int id = -1;
    float v[VALS] = {0.0f, 0.0f, 0.0f};
    if (pix_x < f.W && pix_y < f.H) {
        const size_t pix = (size_t)pix_y * f.W + pix_x;
        const int c = std::min(std::max(contrib[pix], 0), (int)(end - start));
        if (c > 0) {
            id = f.point_list[start + c - 1]; // start + c - 1 < end <= D
            if ((long long)id >= f.N) id = -1;
        }
        if (id >= 0) {
            // dx, dy as blend_forward_weight forms them, m as the forward has it: the clamp decision repeats bit for bit
            const float *pxy = f.xy + (size_t)id * f.xy_stride;
            const float dx = pxy[0] - (float)pix_x, dy = pxy[1] - (float)pix_y;
            const float m0 = invd[(size_t)id * invd_stride];
            const float2 sl = *reinterpret_cast<const float2 *>(slopes + (size_t)id * 2);
            const float mr = __builtin_fmaf(-sl.x, dx, __builtin_fmaf(-sl.y, dy, m0));
            const float m = fminf(fmaxf(mr, m0 * 0.25f), m0 * GSR_PLANE_DEPTH_MAX_RATIO);
            if (m == mr) { // not clamped
                const float g = g_in[pix];
                v[0] = g; v[1] = g * (-dx); v[2] = g * (-dy);
            }
        }
    }
    // every lane follows the loop; a lane without a Gaussian, or with a clamped entry, adds nothing (it matches no id, or holds zeros)
    unsigned long long todo = __builtin_amdgcn_ballot_w64(id >= 0);
    while (todo != 0ull) {
        const int leader = __builtin_ctzll(todo);
        const int cur = __builtin_amdgcn_readlane(id, leader);
        const bool match = id == cur;
#pragma unroll
        for (int k = 0; k < VALS; ++k) s_v[wv][k][lane] = match ? v[k] : 0.0f;
        wave_lds_sync();
        float sum = 0.0f;
        if (lane < 2 * VALS) {
            const float *row = &s_v[wv][lane % VALS][(lane / VALS) * 32];
#pragma unroll
            for (int j = 0; j < 32; ++j) sum += row[j];
        }
        sum += __shfl_down(sum, VALS, 64); // pixels 0-31 + pixels 32-63
        // (a zero sum is not added: x + 0 is x, but for the sign of a zero)
        if (lane < VALS && sum != 0.0f) atomicAdd(&dmom[(size_t)cur * VALS + lane], sum);
        wave_lds_sync(); // the rows are read before the next Gaussian's values overwrite them
        todo &= ~__builtin_amdgcn_ballot_w64(match);
    }
}

// NULL, DIMS, ALIGN, in the header's order; GSR_OK when the call may be enqueued
int check(const GsrDistortionFrame *fr, const void *a, const void *b, const void *c, const void *d)
{
    if (frame_has_null(fr) || !fr->inv_depth || !a || !b || !c || !d) return GSR_E_NULL;
    if (!frame_dims_ok(fr) || fr->inv_depth_stride < 1) return GSR_E_DIMS;
    if (!frame_aligned(fr) || !gsr_aligned4(fr->inv_depth) || !all_aligned16(a, b, c, d)) return GSR_E_ALIGN;
    return GSR_OK;
}

} // namespace

extern "C" int gsr_pmed_forward(const GsrDistortionFrame *frame, const float *slopes, float *median_inv_depth, int32_t *median_contrib,
                                void *stream)
{
    const int rc = check(frame, slopes, median_inv_depth, median_contrib, median_contrib);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    // a frame with D = 0 walks nothing: every pixel is written as 0 / 0
    hipLaunchKernelGGL(plane_median_kernel, dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, frame->inv_depth,
                       (long long)frame->inv_depth_stride, slopes, median_inv_depth, median_contrib);
    return gsr_done();
}

extern "C" int gsr_pmed_backward(const GsrDistortionFrame *frame, const float *slopes, const float *dL_dmedian, const int32_t *median_contrib,
                                 float *dL_dplane_moments, void *stream)
{
    const int rc = check(frame, slopes, dL_dmedian, median_contrib, dL_dplane_moments);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (k.D == 0) return GSR_OK; // nothing was blended: nothing to add
    hipLaunchKernelGGL(plane_median_backward_kernel, dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, frame->inv_depth,
                       (long long)frame->inv_depth_stride, slopes, dL_dmedian, median_contrib, dL_dplane_moments);
    return gsr_done();
}
