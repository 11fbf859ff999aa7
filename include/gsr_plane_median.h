/*
 * gsr_plane_median.h -- the ray-plane intersection depth under the median rule over the lists of a rendered frame, and its gradient,
 * in libgsr_hip.so: the depth RaDe-GS and GOF fuse.  gsr_median_depth.h chooses ONE Gaussian per pixel, the one at which the
 * transmittance falls through one half, and takes 1 / z of its centre; gsr_plane_depth.h (b) takes a flat Gaussian for a piece of its
 * plane and blends the inverse depth m_k(p) at which the pixel's own ray meets it.  This is the product of the two: the m_k(p) of the
 * one Gaussian the median rule chooses.  A stage of its own behind the forward, like both: the frame struct is gsr_distortion.h's,
 * the slopes are gsr_plane_slopes' (gsr_plane_depth.h (a)); no rasterizer kernel, struct or entry point changes, nothing is binned
 * or sorted again, and NO stage of the backward is added (see "Backward").
 *
 * Every float32 step is stated: products left to right, nothing contracted unless a fused multiply-add is named.
 *
 * Forward.  For pixel p the applied entries of its tile's list and their alphas are exactly those of gsr_median_depth.h (the same
 * float32 power expression, alpha = min(0.99, o exp(power)) with the forward's exp, the two skip tests, the walk up to n_contrib[p]).
 * With dx = x_k - p.x, dy = y_k - p.y as the forward forms them, invd = inv_depth[i_k * inv_depth_stride] and (gx, gy) = slopes[i_k],
 * from T = 1, med = 0, c = 0, per applied entry at 1-based list position pos, in list order:
 *
 *     mr = fma(-gx, dx, fma(-gy, dy, invd))
 *     m  = fmin(fmax(mr, invd * 0.25f), invd * 4.0f)       (gsr_plane_depth.h (b), GSR_PLANE_DEPTH_MAX_RATIO; the entry is CLAMPED
 *                                                           where m != mr)
 *     if T > 0.5f (T BEFORE this entry):   med = m,  c = pos
 *     T <- T * (1 - alpha)
 *
 *     plane_median_inv_depth[p] = med
 *     plane_median_contrib[p]   = c        n_contrib's convention: the 1-based position in the tile's list; 0 = no applied entry, med = 0
 *
 * Two facts follow.  c does not depend on the slopes: plane_median_contrib is bit for bit median_contrib of gsr_median_depth_forward
 * on the same frame.  At slopes (0, 0) mr = m = invd exactly, so med is bit for bit that call's median_inv_depth.  Every element of
 * both images is written; pixels without an applied entry, pixels of a tile without a list and every pixel of a frame with D = 0 are
 * 0 / 0.  Three registers per pixel, no atomics: the same frame gives the same bits every call, on every stream, with or without
 * block_masks.  A pixel is finished once T <= 0.5; the kernel leaves a tile's list after the first 256-entry batch behind which no
 * pixel of the tile is open, which changes nothing in the result.  The error of med against the exact plane is that of two fused
 * multiply-adds: at most 2 eps32 (|invd| + |gx dx| + |gy dy|), no sum over entries enters it.
 *
 * Backward.  The median is piecewise constant in everything but the chosen entry's m, and m = (n . r(p)) / (n . mu): its whole
 * dependence on the Gaussian travels through the three moments gsr_plane_slopes_backward consumes (gsr_plane_depth.h (c) / (d)), here
 * with weight 1 at the chosen entry instead of w.  With g = dL_dmedian[p], c = median_contrib[p] clipped to the tile's clipped
 * range, id = point_list[start(tile) + c - 1], dx, dy, mr and m recomputed by the forward's expressions (the clamp decision repeats
 * bit for bit), for every pixel with c > 0, id in [0, N) and m == mr:
 *
 *     dL_dplane_moments[id] += (g,  g * (-dx),  g * (-dy))
 *
 * A clamped entry is a constant and adds nothing.  On the fallback branch gsr_plane_slopes_backward makes -(invd^2 S0) of the row,
 * the centre median's gradient.  No accumulator column is touched: backward(), its stages and the camera gradient stay as they are,
 * and the moments go on through gsr_plane_slopes_backward and gsr_gaussian_normals_backward to the means and rotations.  The call
 * ADDS to dL_dplane_moments: THE CALLER CLEARS (or seeds) IT.  That is what lets this term and gsr_plane_depth_backward's share one
 * moments buffer -- everything behind the moments is linear in them.
 *
 * An 8x8 pixel block sums each of the three values over the pixels that chose the same Gaussian in gsr_median_depth.h's fixed order
 * -- from +0, pixels 0-31 in order (pixel q of a block is (q & 7, q >> 3)), pixels 32-63 in order, every other pixel of the block
 * counting as +0, then the two halves -- and adds each sum with one float atomic per (block, distinct Gaussian, value); a sum that
 * is zero is not added.  The last bits of a row that several blocks touch may differ from run to run.  Per element the float32
 * error is at most (n + 2) 2^-24 times the sum of the addends' magnitudes, n the element's number of addends: one rounding in dx (or
 * dy), one in the product, n - 1 in a sum of any order.  dL_dmedian must be finite.
 *
 * Every access is bounded as in gsr_features.h: a tile's range is clipped to [0, D], a pixel visits min(n_contrib[p], range length)
 * entries, median_contrib is clipped to the range, and an id outside [0, N) is skipped.  Stale or foreign buffers of the stated
 * sizes give wrong numbers, never an access out of bounds.  block_masks (optional, NULL is allowed) only let a wave pass over
 * entries that cannot reach its block; the backward does not read them.
 *
 * All pointers are device pointers.  slopes, median_inv_depth, median_contrib, dL_dmedian and dL_dplane_moments are 16-byte
 * aligned; the arrays of the frame are 4-byte aligned (xy, conic_opacity and inv_depth may be columns of a wider record: their row
 * strides are given in floats).  The caller owns every byte: the library allocates nothing, enqueues everything on `stream`, waits
 * for nothing and reads nothing back.  No workspace is needed.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL   frame, xy, conic_opacity, inv_depth, ranges, n_contrib or an array argument is NULL; point_list is NULL while D > 0.
 *     GSR_E_DIMS   W or H < 1 or > GSR_FEATURES_MAX_SIDE, N < 1 or > 2^31 - 1, D < 0 or > 2^30, xy_stride < 2, conic_opacity_stride < 4,
 *                  inv_depth_stride < 1.
 *     GSR_E_ALIGN  an array is not aligned as stated above.
 *     GSR_E_HIP    a launch failed.
 */
#ifndef GSR_PLANE_MEDIAN_H
#define GSR_PLANE_MEDIAN_H

#include "gsr.h"
#include "gsr_distortion.h"
#include "gsr_plane_depth.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two entry points are spelled gsr_pmed_* ("plane median"): the library's exported names that contain "plane" are exactly those
 * of gsr_plane_depth.h and those that contain "median" exactly those of gsr_median_depth.h, and both facts are held by tests. */

/* median_inv_depth[H][W] and median_contrib[H][W].  Every element of both is written.  With D = 0 both are zeros. */
int gsr_pmed_forward(const GsrDistortionFrame *frame, const float *slopes /* [N][2] */, float *median_inv_depth /* [H][W] */,
                     int32_t *median_contrib /* [H][W] */, void *stream);

/* ADDS (g, g (-dx), g (-dy)) of every pixel whose chosen entry is not clamped into dL_dplane_moments[N][3]: the caller clears.  With
 * D = 0 nothing is enqueued. */
int gsr_pmed_backward(const GsrDistortionFrame *frame, const float *slopes /* [N][2] */, const float *dL_dmedian /* [H][W] */,
                      const int32_t *median_contrib /* [H][W] */, float *dL_dplane_moments /* [N][3], ADDED to */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_PLANE_MEDIAN_H */
