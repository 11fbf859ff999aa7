/*
 * gsr_densify_stats.h -- screen-space densification statistics of libgsr_hip.so, with optional absolute gradients.
 *
 * The reference trainer marks clone / split candidates from the 3D position gradient of the one view it rendered last
 * (gsr.h gsr_densify_mark).  The entry points here keep, per Gaussian and over every view since the last density-control call,
 *     grad_accum = sum over the views that saw it of |dL/dmean2D| = sqrt(gx^2 + gy^2)
 *     vis_count  = the number of those views (radii > 0)
 *     max_radii  = its largest screen radius in pixels (GsrGeom.radii)
 * and mark from grad_accum / vis_count.  gx, gy are columns 3-4 of the accumulator records the backward blend sums into
 * (gsr_backward_accumulators_offset; the dL_dmean2D of GsrGrads, in its convention: the factor 0.5 W / 0.5 H included).
 *
 * Absolute gradients (GSR_BWD_ABSGRAD).  dL/dmean2D of a Gaussian is a sum over (pixel, list entry) pairs, and the two sides of
 * a blurry splat contribute with opposite signs that cancel.  With the flag the backward blend also sums the MAGNITUDES of
 * exactly those terms,
 *     abs_x = sum |h (a dx + b dy)| 0.5 W        abs_y = sum |h (c dy + b dx)| 0.5 H        (h = dL/dG * G, conic a b c)
 * over the same pairs (the same `contributes` predicate, gradient passing the 0.99 alpha cap as the signed one does), into
 * columns 12-13 of the accumulator records.  abs >= |signed| up to float rounding.
 *
 * Contract
 *   - gsr_backward_flags / gsr_backward_blend_flags take the arguments of gsr_backward_aux / gsr_backward_blend_aux
 *     (gsr_aux_grads.h) and `flags`.  flags = 0 IS that call: the same kernels are launched.  Unknown bits give GSR_E_DIMS.
 *   - With GSR_BWD_ABSGRAD, columns 12-13 of the accumulator records hold the absolute sums; without it they are zero (cleared
 *     with the row, never written).  Every other output is what the unflagged call gives, up to float-atomic order.  The geometry
 *     half (gsr_backward_geom, gsr_backward_geom_aux) pairs with gsr_backward_blend_flags unchanged.
 *   - gsr_densify_stats_update follows a backward on the same `ws` and stream.  It reads the records at
 *     gsr_backward_accumulators_offset(N) and `radii` ([N], GsrGeom.radii) and, for radii[i] > 0, adds the norm to grad_accum[i],
 *     1 to vis_count[i] and raises max_radii[i] to radii[i].  These are device atomics: views rendered on different streams may
 *     update ONE statistics set concurrently; nothing else may write it meanwhile.
 *   - use_abs != 0 reads columns 12-13 instead of 3-4.  After a backward WITHOUT GSR_BWD_ABSGRAD that accumulates zeros: the
 *     library cannot see it, it is the caller's rule.  So is this: a capacity-mode frame (gsr_capacity.h) that overflowed must
 *     not be fed to gsr_densify_stats_update.
 *   - gsr_densify_mark_stats is gsr_densify_mark's rule on avg = grad_accum / max(vis_count, 1) (non-finite counts as 0) in place
 *     of the gradient norm.  params->N may exceed stats->N (rows a clone added): those rows have avg = 0.
 *   - gsr_prune_mark_stats: valid[i] = opacity_i > opacity_threshold
 *         && !(max_screen_radius > 0 && max_radii[i] > max_screen_radius) && !(max_world_scale > 0 && max(scale_i) > max_world_scale).
 *     A size term <= 0 is off.  Rows past stats->N have max_radii = 0.
 *   - No allocations, no host synchronisation.  N = 0 is fine (nothing is enqueued).
 *   - Errors, every one checked before anything is enqueued.  The backward pair: GSR_E_DIMS for unknown flags, then
 *     gsr_backward_aux's in its order.  The statistics calls: GSR_E_NULL, GSR_E_DIMS (N < 0 or too large, stats->N > params->N,
 *     an unknown mode), GSR_E_ALIGN (16 bytes: the three arrays, radii, ws), GSR_E_WORKSPACE (ws below
 *     gsr_backward_workspace_bytes(N, 0, 1, 1)).
 */
#ifndef GSR_DENSIFY_STATS_H
#define GSR_DENSIFY_STATS_H

#include "gsr_aux_grads.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_BWD_ABSGRAD 1u /* the backward blend also sums |terms of dL/dmean2D| into columns 12-13 of the accumulator records */

int gsr_backward_flags(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning,
                       const GsrImage *image, const GsrPixelGrads *pixel_grads, const GsrGrads *grads, float *dL_dinv_depths, void *ws,
                       size_t ws_bytes, uint32_t flags, void *stream);
int gsr_backward_blend_flags(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning,
                             const GsrImage *image, const GsrPixelGrads *pixel_grads, float *payload, void *ws, size_t ws_bytes,
                             uint32_t flags, void *stream);

typedef struct GsrDensifyStats {
    int64_t N;
    float *grad_accum;  /* [N] sum of |dL/dmean2D| over the views that saw the Gaussian */
    int32_t *vis_count; /* [N] number of those views */
    int32_t *max_radii; /* [N] largest screen radius, pixels */
} GsrDensifyStats;

int gsr_densify_stats_update(const GsrDensifyStats *stats, const int32_t *radii, const void *ws, size_t ws_bytes, int32_t use_abs,
                             void *stream);
int gsr_densify_mark_stats(const GsrParams *params, const GsrDensifyStats *stats, float grad_threshold, float scene_extent,
                           float percent_dense, int mode, int32_t *mask, void *stream);
int gsr_prune_mark_stats(const GsrParams *params, const GsrDensifyStats *stats, float opacity_threshold, float max_screen_radius,
                         float max_world_scale, int32_t *valid, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_DENSIFY_STATS_H */
