/*
 * gsr_median_depth.h -- the median inverse depth over the lists of a rendered frame, and its gradient, in libgsr_hip.so: the depth
 * 2DGS, GOF, PGSR and RaDe-GS fuse bounded scenes from.  The forward's depth image is the EXPECTED inverse depth sum w m, which lies
 * inside a thick or semi-transparent layer of Gaussians; the median is the inverse depth of ONE Gaussian, the one at which the
 * transmittance falls through one half.  A stage of its own behind the forward and between the two halves of the backward, like
 * gsr_distortion.h, whose frame struct it takes as it is: no rasterizer kernel, struct or entry point changes, and nothing is
 * binned or sorted again.
 *
 * Definition.  For pixel p the applied entries of its tile's list and their alphas are exactly those of gsr_features.h: the same
 * float32 power expression, alpha = min(0.99, o exp(power)) with the forward's exp, the two skip tests (power > 0, alpha < 1/255)
 * and the walk up to n_contrib[p].  m_k is the inverse view depth of Gaussian i_k, inv_depth[i_k * inv_depth_stride], as in
 * gsr_distortion.h.
 *
 * Forward, per pixel, float32: T = 1, med = 0, c = 0, and per applied entry at 1-based list position pos, in list order:
 *
 *     if T > 0.5f (T BEFORE this entry):   med = m_k,  c = pos
 *     T <- T * (1 - alpha)
 *
 * 2DGS's rule: the result is the entry that takes T to at most one half, or the last applied entry if T never gets there.  A T of
 * exactly 0.5 closes the pixel: the strict > leaves the next entry out.  Then
 *
 *     median_inv_depth[p] = med     a copy of inv_depth[i_c * inv_depth_stride]: the same bits, no arithmetic applied
 *     median_contrib[p]   = c       n_contrib's convention: the 1-based position in the tile's list; 0 = no applied entry, med = 0
 *
 * Every element of both images is written.  Pixels without an applied entry, pixels of a tile without a list and every pixel of a
 * frame with D = 0 are 0 / 0.  No atomics: the same frame gives the same bits every call, on every stream, with or without
 * block_masks.  T is the float32 product the forward blend forms; where a prefix T_k lies within a few k eps32 of 0.5 another
 * evaluation of the same definition (float64, another exp) may lawfully choose the neighbouring entry.  A pixel is finished once
 * T <= 0.5; the kernel leaves a tile's list after the first 256-entry batch behind which no pixel of the tile is open, which changes
 * nothing in the result.
 *
 * Backward.  The median is piecewise constant in everything but the chosen Gaussian's inverse depth, so with g = dL_dmedian[p],
 * c = median_contrib[p] clipped to the tile's clipped range and id = point_list[start(tile) + c - 1]:
 *
 *     accumulators[id * 16 + 11] += g          (column 11 of the backward's 16-float records: dL/d(1/depth))
 *
 * for every pixel with c > 0 and id in [0, N), and no other column is touched.  An 8x8 pixel block sums g over the pixels that chose
 * the same Gaussian in a fixed order -- from +0, pixels 0-31 in order (pixel q of a block is (q & 7, q >> 3)), pixels 32-63 in
 * order, every other pixel of the block counting as +0, then the two halves -- and adds the sum with one float atomic per
 * (block, distinct Gaussian); a sum that is zero is not added.  The last bits of a row that several blocks touch may differ from run
 * to run.  The per-Gaussian half of the backward (gsr_backward_geom_aa, the AUX kernel) then carries column 11 on to the means, and
 * gsr_backward_camera_aa to the camera.  dL_dmedian must be finite.
 *
 * Every access is bounded as in gsr_features.h: a tile's range is clipped to [0, D], a pixel visits min(n_contrib[p], range length)
 * entries, median_contrib is clipped to the range, and an id outside [0, N) is skipped.  Stale or foreign buffers of the stated
 * sizes give wrong numbers, never an access out of bounds.  block_masks (optional, NULL is allowed) only let a wave pass over
 * entries that cannot reach its block; the backward does not read them.
 *
 * All pointers are device pointers.  median_inv_depth, median_contrib, dL_dmedian and accumulators are 16-byte aligned; the arrays
 * of the frame are 4-byte aligned (xy, conic_opacity and inv_depth may be columns of a wider record: their row strides are given in
 * floats).  The caller owns every byte: the library allocates nothing, enqueues everything on `stream`, waits for nothing and reads
 * nothing back.  No workspace is needed.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL   frame, xy, conic_opacity, inv_depth, ranges, n_contrib or an array argument is NULL; point_list is NULL while D > 0.
 *     GSR_E_DIMS   W or H < 1 or > GSR_FEATURES_MAX_SIDE, N < 1 or > 2^31 - 1, D < 0 or > 2^30, xy_stride < 2, conic_opacity_stride < 4,
 *                  inv_depth_stride < 1.
 *     GSR_E_ALIGN  an array is not aligned as stated above.
 *     GSR_E_HIP    a launch failed.
 */
#ifndef GSR_MEDIAN_DEPTH_H
#define GSR_MEDIAN_DEPTH_H

#include "gsr.h"
#include "gsr_distortion.h"

#ifdef __cplusplus
extern "C" {
#endif

/* median_inv_depth[H][W] and median_contrib[H][W].  Every element of both is written. */
int gsr_median_depth_forward(const GsrDistortionFrame *frame, float *median_inv_depth /* [H][W] */, int32_t *median_contrib /* [H][W] */,
                             void *stream);

/* Adds dL_dmedian[p] into column 11 of the accumulator record of the Gaussian each pixel chose. */
int gsr_median_depth_backward(const GsrDistortionFrame *frame, const float *dL_dmedian /* [H][W] */, const int32_t *median_contrib /* [H][W] */,
                              float *accumulators /* [N][16] */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_MEDIAN_DEPTH_H */
