// median_depth.hip -- the median rule over a frame's lists for both depth models, with the gradients: the median inverse depth
// (include/gsr_median_depth.h) and the ray-plane intersection depth under the median rule (include/gsr_plane_median.h), for gfx950.
//
//   - forwards: frame_walk.h's FrameWalk with its early exit and MedianPick below.  The staged record's spare float carries 1/depth, as
//     in distortion.hip; the plane's records are plane_depth.hip's 48 bytes, the two slopes in the third word, and its value costs two
//     fused multiply-adds and a clamp per taken entry.  T, the chosen value and its list position live in three registers per lane.  A
//     pixel is finished once T <= 0.5, usually within the first batch, so the workgroup leaves the list as soon as none of its pixels
//     is open.  No LDS beyond the staging, no atomics: the same bits every call and with or without masks.
//   - backwards: no walk, chosen_entry_scatter below.  One wave per 8x8 block, lane = pixel; the wave loops over the distinct
//     Gaussians its pixels chose, sums each of the lane's values over each one's pixels in the headers' fixed order through one
//     64-float LDS row per value, and adds the sums with one atomic wave-instruction: dL_dmedian to column 11 of the Gaussian's
//     accumulator record; for the plane (g, g (-dx), g (-dy)), zeros where the forward clamped, to its row of dL_dplane_moments.
#include "frame_walk.h"
#include "gsr_median_depth.h"
#include "gsr_plane_median.h"
#include "gsr_plane_depth.h"

namespace {

// The median rule: an applied entry is taken while T > 0.5, then T = T (1 - t).  T, the taken value and its 1-based list position.
struct MedianPick {
    float T = 1.0f, med = 0.0f;
    int c = 0;

    // one entry of the walk; value() is evaluated for a taken entry only
    template <class Value>
    __device__ __forceinline__ void entry(float t, bool applied, int pos, Value value)
    {
        if (applied) {
            if (T > 0.5f) {
                med = value();
                c = pos;
            }
            T = T * (1.0f - t);
        }
    }
    // the walk's `open`: this lane's pixel may still change
    __device__ __forceinline__ bool open() const { return T > 0.5f; }
    __device__ __forceinline__ void store(const FrameWalk &walk, float *med_out, int32_t *contrib_out) const
    {
        if (walk.inside) {
            med_out[walk.pix] = med;
            contrib_out[walk.pix] = c;
        }
    }
};

__global__ __launch_bounds__(256) void median_depth_kernel(FrameK f, const float *__restrict__ invd, long long invd_stride, float *__restrict__ med_out,
                                                           int32_t *__restrict__ contrib_out)
{
    const FrameWalk walk(f);
    MedianPick pick;
    walk.run<2>(
        f, DepthFill{invd, invd_stride, nullptr},
        [&](const float4 &ra, const float4 &rb, float dx, float dy, float G, float t, bool applied, int pos) {
            pick.entry(t, applied, pos, [&] { return rb.w; });
        },
        [&] { return pick.open(); });
    pick.store(walk, med_out, contrib_out);
}

__global__ __launch_bounds__(256) void plane_median_kernel(FrameK f, const float *__restrict__ invd, long long invd_stride, const float *__restrict__ slopes,
                                                           float *__restrict__ med_out, int32_t *__restrict__ contrib_out)
{
    const FrameWalk walk(f);
    MedianPick pick;
    walk.run<3>(
        f, DepthFill{invd, invd_stride, slopes},
        [&](const float4 &ra, const float4 &rb, const float4 &rc, float dx, float dy, float G, float t, bool applied, int pos) {
            pick.entry(t, applied, pos, [&] {
                float mr;
                return plane_inv_depth(rb.w, rc.x, rc.y, dx, dy, mr);
            });
        },
        [&] { return pick.open(); });
    pick.store(walk, med_out, contrib_out);
}

// The chosen-entry scatter: the forward's geometry without its walk (workgroup = tile, wave = 8x8 block, lane = pixel).  Each lane
// with a chosen Gaussian gets its VALS values from values(id, pix, pix_x, pix_y, v) (v arrives as zeros); value k of Gaussian id is
// added to dst[id * stride + column + k], ValueTile's tail convention.
template <int VALS, class Values>
__device__ __forceinline__ void chosen_entry_scatter(const FrameK &f, const int32_t *__restrict__ contrib, float *__restrict__ dst, size_t stride, int column,
                                                     Values values)
{
    static_assert(2 * VALS <= 64, "a row is summed with two lanes");
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
    float v[VALS];
#pragma unroll
    for (int k = 0; k < VALS; ++k) v[k] = 0.0f;
    if (pix_x < f.W && pix_y < f.H) {
        const size_t pix = (size_t)pix_y * f.W + pix_x;
        const int c = std::min(std::max(contrib[pix], 0), (int)(end - start));
        if (c > 0) {
            id = f.point_list[start + c - 1]; // start + c - 1 < end <= D
            if ((long long)id >= f.N) id = -1;
        }
        if (id >= 0) values(id, pix, pix_x, pix_y, v);
    }
    // every lane follows the loop; a lane without a Gaussian, or with zeros for values, adds nothing (it matches no id, or holds zeros)
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
        if (lane < VALS && sum != 0.0f) atomicAdd(&dst[(size_t)cur * stride + column + lane], sum);
        wave_lds_sync(); // the rows are read before the next Gaussian's values overwrite them
        todo &= ~__builtin_amdgcn_ballot_w64(match);
    }
}

__global__ __launch_bounds__(256) void median_depth_backward_kernel(FrameK f, const float *__restrict__ g_in, const int32_t *__restrict__ contrib,
                                                                    float *__restrict__ acc)
{
    chosen_entry_scatter<1>(f, contrib, acc, 16, 11, [&](int id, size_t pix, int pix_x, int pix_y, float (&v)[1]) { v[0] = g_in[pix]; });
}

// S0, Sx, Sy: the Gaussian's row of dL_dplane_moments
__global__ __launch_bounds__(256) void plane_median_backward_kernel(FrameK f, const float *__restrict__ invd, long long invd_stride,
                                                                    const float *__restrict__ slopes, const float *__restrict__ g_in,
                                                                    const int32_t *__restrict__ contrib, float *__restrict__ dmom)
{
    chosen_entry_scatter<3>(f, contrib, dmom, 3, 0, [&](int id, size_t pix, int pix_x, int pix_y, float (&v)[3]) {
        // dx, dy as blend_forward_weight forms them, m as the forward has it: the clamp decision repeats bit for bit
        const float *pxy = f.xy + (size_t)id * f.xy_stride;
        const float dx = pxy[0] - (float)pix_x, dy = pxy[1] - (float)pix_y;
        float4 rb, rc;
        DepthFill{invd, invd_stride, slopes}(id, rb, rc);
        float mr;
        if (plane_inv_depth(rb.w, rc.x, rc.y, dx, dy, mr) == mr) { // not clamped
            const float g = g_in[pix];
            v[0] = g; v[1] = g * (-dx); v[2] = g * (-dy);
        }
    });
}

} // namespace

extern "C" int gsr_median_depth_forward(const GsrDistortionFrame *frame, float *median_inv_depth, int32_t *median_contrib, void *stream)
{
    const int rc = check_frame(frame, median_inv_depth, median_contrib);
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
    const int rc = check_frame(frame, dL_dmedian, median_contrib, accumulators);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (k.D == 0) return GSR_OK; // nothing was blended: nothing to add
    hipLaunchKernelGGL(median_depth_backward_kernel, dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, dL_dmedian, median_contrib, accumulators);
    return gsr_done();
}

extern "C" int gsr_pmed_forward(const GsrDistortionFrame *frame, const float *slopes, float *median_inv_depth, int32_t *median_contrib,
                                void *stream)
{
    const int rc = check_frame(frame, slopes, median_inv_depth, median_contrib);
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
    const int rc = check_frame(frame, slopes, dL_dmedian, median_contrib, dL_dplane_moments);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (k.D == 0) return GSR_OK; // nothing was blended: nothing to add
    hipLaunchKernelGGL(plane_median_backward_kernel, dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, frame->inv_depth,
                       (long long)frame->inv_depth_stride, slopes, dL_dmedian, median_contrib, dL_dplane_moments);
    return gsr_done();
}
