// densify_stats.hip -- screen-space densification statistics (include/gsr_densify_stats.h).
//
// What every 3DGS trainer other than the teaching reference densifies on: per Gaussian, the norm of the screen-space mean gradient
// summed over the views that saw it, the number of those views and its largest screen radius.  The gradient is already in the
// accumulator records the backward blend sums into (GradRec columns 3-4; columns 12-13 hold the AbsGS-style sums of magnitudes
// when the backward ran with GSR_BWD_ABSGRAD, blend_bwd_splat.hip ABS), so one streaming kernel per view reads 8 bytes of each
// record and 4 bytes of radii and issues three atomics per visible Gaussian.  The mark kernels are densify.hip's mark_kernel /
// prune_mark_kernel with the statistics in place of the one-view 3D gradient.
#include <math.h>

#include "gsr_densify_stats.h"
#include "gsr_internal.h"
#include "sh_stage.h"

namespace {

// One thread per Gaussian.  The record columns are read once per frame by this kernel and by nothing after it: non-temporal, like
// the other use-once streams (sh_stage.h).  The three read-modify-writes are atomics without return, so views on different
// streams may update one statistics set at the same time.
__global__ __launch_bounds__(256) void densify_stats_update_kernel(int64_t N, const int32_t *__restrict__ radii, const GradRec *__restrict__ acc,
                                                                   int col, float *__restrict__ grad_accum, int32_t *__restrict__ vis_count,
                                                                   int32_t *__restrict__ max_radii)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int32_t r = radii[i];
    if (!(r > 0)) return;
    const float gx = gsr_ld1<true>(&acc[i].f[col]), gy = gsr_ld1<true>(&acc[i].f[col + 1]);
    unsafeAtomicAdd(grad_accum + i, sqrtf(gx * gx + gy * gy));
    atomicAdd(vis_count + i, 1);
    atomicMax(max_radii + i, r);
}

// avg = grad_accum / max(vis_count, 1), non-finite -> 0; rows past the statistics (added by a clone since) have avg = 0
__device__ __forceinline__ float stats_avg(int64_t i, int64_t n_stats, const float *grad_accum, const int32_t *vis_count)
{
    if (i >= n_stats) return 0.0f;
    const int32_t c = vis_count[i];
    const float avg = grad_accum[i] / (float)(c > 1 ? c : 1);
    return isfinite(avg) ? avg : 0.0f;
}

__global__ __launch_bounds__(256) void densify_mark_stats_kernel(int64_t N, const float *__restrict__ scales, int64_t n_stats,
                                                                 const float *__restrict__ grad_accum, const int32_t *__restrict__ vis_count,
                                                                 float grad_threshold, float scale_threshold, int mode, int32_t *__restrict__ mask)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float avg = stats_avg(i, n_stats, grad_accum, vis_count);
    const float max_scale = fmaxf(fmaxf(scales[i * 3 + 0], scales[i * 3 + 1]), scales[i * 3 + 2]);
    const bool high_grad = avg >= grad_threshold;
    const bool size_ok = mode == GSR_MARK_SPLIT ? (max_scale > scale_threshold) : (max_scale <= scale_threshold);
    mask[i] = (high_grad && size_ok) ? 1 : 0;
}

__global__ __launch_bounds__(256) void prune_mark_stats_kernel(int64_t N, const float *__restrict__ opacities, const float *__restrict__ scales,
                                                               int64_t n_stats, const int32_t *__restrict__ max_radii, float opacity_threshold,
                                                               float max_screen, float max_world, int32_t *__restrict__ valid)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    bool keep = opacities[i] > opacity_threshold;
    if (max_screen > 0.0f && i < n_stats && (float)max_radii[i] > max_screen) keep = false;
    if (max_world > 0.0f) {
        const float max_scale = fmaxf(fmaxf(scales[i * 3 + 0], scales[i * 3 + 1]), scales[i * 3 + 2]);
        if (max_scale > max_world) keep = false;
    }
    valid[i] = keep ? 1 : 0;
}

unsigned blocks_for(int64_t threads) { return (unsigned)gsr_div_up(threads, 256); }
constexpr int64_t MAX_ROWS = (int64_t)1 << 27; // densify.hip's row limit

// GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN for a statistics set (N = 0 needs no arrays)
int check_stats(const GsrDensifyStats *st)
{
    if (!st) return GSR_E_NULL;
    if (st->N < 0 || st->N > MAX_ROWS) return GSR_E_DIMS;
    if (st->N > 0 && (!st->grad_accum || !st->vis_count || !st->max_radii)) return GSR_E_NULL;
    if (!gsr_aligned16(st->grad_accum) || !gsr_aligned16(st->vis_count) || !gsr_aligned16(st->max_radii)) return GSR_E_ALIGN;
    return GSR_OK;
}

} // namespace

extern "C" {

int gsr_densify_stats_update(const GsrDensifyStats *stats, const int32_t *radii, const void *ws, size_t ws_bytes, int32_t use_abs, void *stream)
{
    if (int rc = check_stats(stats)) return rc;
    const int64_t N = stats->N;
    if (N == 0) return GSR_OK;
    if (!radii) return GSR_E_NULL;
    if (!gsr_aligned16(radii) || !gsr_aligned16(ws)) return GSR_E_ALIGN;
    if (!ws || ws_bytes < gsr_backward_workspace_bytes(N, 0, 1, 1)) return GSR_E_WORKSPACE;
    const GradRec *acc = reinterpret_cast<const GradRec *>(static_cast<const char *>(ws) + gsr_backward_accumulators_offset(N));
    const int col = use_abs ? gsr_gradrec_slot(10) : gsr_gradrec_slot(3); // columns 12-13 or 3-4
    hipLaunchKernelGGL(densify_stats_update_kernel, dim3(blocks_for(N)), dim3(256), 0, (hipStream_t)stream, N, radii, acc, col, stats->grad_accum,
                       stats->vis_count, stats->max_radii);
    return gsr_done();
}

int gsr_densify_mark_stats(const GsrParams *params, const GsrDensifyStats *stats, float grad_threshold, float scene_extent, float percent_dense,
                           int mode, int32_t *mask, void *stream)
{
    if (!params) return GSR_E_NULL;
    if (int rc = check_stats(stats)) return rc;
    if (params->N < 0 || params->N > MAX_ROWS || stats->N > params->N || (mode != GSR_MARK_CLONE && mode != GSR_MARK_SPLIT)) return GSR_E_DIMS;
    if (params->N == 0) return GSR_OK;
    if (!params->scales || !mask) return GSR_E_NULL;
    const float scale_threshold = percent_dense * scene_extent; // float32 product, as gsr_densify_mark's
    hipLaunchKernelGGL(densify_mark_stats_kernel, dim3(blocks_for(params->N)), dim3(256), 0, (hipStream_t)stream, params->N, params->scales, stats->N,
                       stats->grad_accum, stats->vis_count, grad_threshold, scale_threshold, mode, mask);
    return gsr_done();
}

int gsr_prune_mark_stats(const GsrParams *params, const GsrDensifyStats *stats, float opacity_threshold, float max_screen_radius,
                         float max_world_scale, int32_t *valid, void *stream)
{
    if (!params) return GSR_E_NULL;
    if (int rc = check_stats(stats)) return rc;
    if (params->N < 0 || params->N > MAX_ROWS || stats->N > params->N) return GSR_E_DIMS;
    if (params->N == 0) return GSR_OK;
    if (!params->opacities || !params->scales || !valid) return GSR_E_NULL;
    hipLaunchKernelGGL(prune_mark_stats_kernel, dim3(blocks_for(params->N)), dim3(256), 0, (hipStream_t)stream, params->N, params->opacities,
                       params->scales, stats->N, stats->max_radii, opacity_threshold, max_screen_radius, max_world_scale, valid);
    return gsr_done();
}

} // extern "C"
