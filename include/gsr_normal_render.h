/*
 * gsr_normal_render.h -- the normals of the Gaussians themselves, blended into an image over the lists of a rendered frame, and the
 * depth-normal consistency term of 2DGS, GOF, PGSR and RaDe-GS, in libgsr_hip.so.  A Gaussian's normal is the direction of its
 * shortest axis, turned to face the camera; the image N(p) = sum_k w_k(p) n[i_k] is blended with the weights the frame was drawn
 * with; the term holds N / |N| to the normals of the rendered depth (gsr_normals.h) and sends a gradient to BOTH sides.  The
 * gradient of the image depends on the pixel and the entry together, so it is a stage of its own between the two halves of the
 * backward, like gsr_distortion.h: no rasterizer kernel, struct or entry point changes, nothing is binned or sorted again.
 *
 * Every float32 step is stated: products left to right, nothing contracted unless a fused multiply-add is named.
 *
 * (a) gsr_gaussian_normals.  One thread per Gaussian i, from scales[i] = (sx, sy, sz), rotations[i] = q = (x, y, z, w) AS STORED
 * (not normalised), means[i] = p and the 16 floats of `viewmatrix` (HOST memory, row-vector convention p_view = [p, 1] @ V,
 * V[r][j] = viewmatrix[4 r + j]; V[:3,:3] is taken as a rotation, nothing is renormalised after it):
 *
 *   1. c* = the index of the smallest of (sx, sy, sz) by strict < in index order: c* = 0; if sy < s[c*] then 1; if sz < s[c*] then 2.
 *      Ties go to the lower index; exact on float32 inputs (a NaN scale is never smaller).
 *   2. a = column c* of the rotation matrix of csrc/sigma3d.h, the same expressions in the same order, with v = e_c*:
 *          cs = 2 * w * w - 1          cr = (y v2 - z v1, z v0 - x v2, x v1 - y v0)          d = ((x v0) + y v1) + z v2
 *          a[r] = (v[r] * cs + cr[r] * w * 2) + q[r] * d * 2
 *   3. l2 = (a0 a0 + a1 a1) + a2 a2.  If !(l2 >= GSR_NORMAL_RENDER_MIN_AXIS2 = 1e-24f), or if the stored quaternion is exactly
 *      (0, 0, 0, 0), the normal is (0, 0, 0) and the row's gradient in (b) is 0.  (The formula is not homogeneous in q: at the zero
 *      quaternion it gives a = -e_c*, the orientation of no rotation, so that case is named; a NaN quaternion fails the first test.)
 *      Otherwise s = sqrt(l2) (IEEE) and ah[r] = a[r] / s (IEEE division).
 *   4. n_c[j] = (ah0 V[0][j] + ah1 V[1][j]) + ah2 V[2][j],   p_v[j] = ((V[0][j] p0 + V[1][j] p1) + V[2][j] p2) + V[3][j]   (j = 0, 1, 2)
 *   5. t = (n_c0 p_v0 + n_c1 p_v1) + n_c2 p_v2,   sigma = t > 0 ? -1 : +1,   normals[i] = sigma n_c.
 *      The normal faces the camera, gsr_normals.h's convention: a fronto-parallel surface gives (0, 0, -1).
 *
 * (b) gsr_gaussian_normals_backward ADDS to dL_drot[i] the exact derivative of (a) with respect to the stored quaternion, c* and
 * sigma held constant (recomputed as above), from g = dL_dnormals[i]:
 *
 *          g_c = sigma g          g_w[r] = (V[r][0] g_c0 + V[r][1] g_c1) + V[r][2] g_c2
 *          e = (ah0 g_w0 + ah1 g_w1) + ah2 g_w2          g_a[r] = (g_w[r] - ah[r] * e) / s
 *          k = (x g_a0 + y g_a1) + z g_a2          X = e_c* x g_a = (v1 g_a2 - v2 g_a1, v2 g_a0 - v0 g_a2, v0 g_a1 - v1 g_a0)
 *          dq[r] = ((2 * w) * X[r] + (2 * q[c*]) * g_a[r]) + (2 * k) * v[r]          (r = 0, 1, 2: x, y, z)
 *          dw = (4 * w) * g_a[c*] + 2 * ((g_a0 cr0 + g_a1 cr1) + g_a2 cr2)
 *
 * One read-modify-write per Gaussian, no atomics.  It adds nothing to means, scales or the camera: c* and sigma are piecewise
 * constant in them, and the normal's DIRECT dependence on `viewmatrix` (step 4) is left out of the camera gradient (camera_grad
 * carries the screen-space columns of (d) only).
 *
 * (c) gsr_normal_render_forward.  The frame is a GsrFeaturesFrame; the applied entries k = 0 ... of a pixel and their weights
 * w_k = alpha_k T_k are exactly those of gsr_features.h (the same float32 power expression, alpha = min(0.99, o exp(power)) with
 * the forward's exp, the two skip tests, T <- T (1 - alpha) from T = 1, the walk up to n_contrib[p]).  From out[p] = (0, 0, 0), per
 * applied entry in list order, ONE fused multiply-add per channel:
 *
 *          out[p][c] <- fma(w_k, normals[i_k][c], out[p][c])
 *
 * which is bit for bit gsr_features_forward at C = 3.  Three running registers per pixel, no atomics: the same bits every call, on
 * every stream, with or without block_masks.  Every pixel is written; pixels without an applied entry, pixels of a tile without a
 * list and every pixel of a frame with D = 0 are (0, 0, 0).
 *
 * (d) gsr_normal_render_backward.  G = dL_dout[p], N = out[p] (the stored forward image, not recomputed).  Per pixel, once:
 *
 *          total = (G.x N.x + G.y N.y) + G.z N.z          P = 0, T = 1
 *
 * and per applied entry, in list order (Gexp = exp(power), o = opacity, dx = x_k - p.x, dy = y_k - p.y as in the forward,
 * n = normals[i_k]):
 *
 *          u  = (G.x n.x + G.y n.y) + G.z n.z
 *          w  = alpha * T
 *          P  <- P + w * u
 *          R  = total - P                      (the entries behind k)
 *          q  = T * u - R / (1 - alpha)        (IEEE division; dL/dalpha: the gradient passes the 0.99 cap)
 *          gd = Gexp * q
 *          h  = o * gd        hx = h * dx      hy = h * dy
 *          nine per-(pixel, entry) values:  hx, hy, hx * dx, hx * dy, hy * dy, gd, w * G.x, w * G.y, w * G.z
 *          T  <- T * (1 - alpha)
 *
 * The total-minus-prefix form keeps one pass; its stated limit is gsr_distortion.h's: R carries the rounding of the total,
 * eps32 |total|, which a back-to-front walk would not have at the last entries of a long list, so Gaussians seen only behind
 * saturated fronts carry a larger relative error in their small rows.
 *
 * An 8x8 pixel block sums each of the nine values over its pixels in gsr_distortion.h's fixed order -- pixels 0-31 in order (pixel q
 * of a block is (q & 7, q >> 3)), pixels 32-63 in order, then the two halves -- to S1, S2, Sxx, Sxy, Syy, Sop, Snx, Sny, Snz and ADDS
 * (a', b', c' = -a/2, -b, -c/2 the pre-scaled conic), with exactly that header's constants:
 *
 *     accumulators[i_k] column 3   (2 a' S1 + b' S2) * (0.5 W)                            dL_dmean2D x
 *                       column 4   (2 c' S2 + b' S1) * (0.5 H)                            dL_dmean2D y
 *                       column 6   -0.5 Sxx     column 7   -0.5 Sxy     column 9   -0.5 Syy      dL_dconic
 *                       column 10  Sop                                                    dL_dopacity (Gexp dL/dalpha)
 *     dL_dnormals[i_k]             (Snx, Sny, Snz)
 *
 * and touches no other accumulator column: 0-2 (colour), 5, 8, 11 (dL/d(1/depth)), 12-13 (the absolute gradients stay the colour,
 * depth and alpha terms' alone) and 14-15 are what the blend half left.  The call CLEARS dL_dnormals first, so rows that no pixel
 * used are exactly 0.  One float atomic per (block, applied entry, value): the last bits of a row that several blocks or tiles
 * touch may differ from run to run.  The per-Gaussian half of the backward (gsr_backward_geom_aa) then carries the six columns on
 * to the parameters, gsr_backward_camera_aa to the camera, and (b) carries dL_dnormals on to the rotations.
 *
 * (e) gsr_normal_consistency_loss.  Per pixel p, from Nimg[p] = N, the depth normal n_d[p] and valid[p] of gsr_normals_from_depth,
 * an optional weight image m (NULL: all ones) and c = (float)((double)weight / ((double)W * (double)H)):
 *
 *          L2 = (N.x N.x + N.y N.y) + N.z N.z
 *          the pixel COUNTS iff valid[p] != 0 and L2 >= GSR_NORMAL_RENDER_MIN_LENGTH * GSR_NORMAL_RENDER_MIN_LENGTH (float32; 1e-3f: a
 *          defined threshold, because 1 / |N| multiplies the gradient where a pixel's Gaussians face apart)
 *          s = sqrt(L2)       th[j] = N[j] / s       dot = (n_d.x th.x + n_d.y th.y) + n_d.z th.z
 *          term = m * (1 - dot)          km = c * m
 *          gN[p][j]  = -((km * (n_d[j] - th[j] * dot)) / s)          gnd[p][j] = -(km * th[j])
 *
 * gN and gnd are (0, 0, 0) at pixels that do not count.  sums[2] = (sum term, sum m) over the counted pixels: thread t of workgroup
 * b takes pixels (b + j B) 256 + t, j = 0, 1, ... (B = min(ceil(W H / 256), 2048) workgroups), adds its terms in that order in
 * double precision, and the totals go through csrc/fixed_sum.h's tree (wave butterfly, four wave sums pairwise, one record per
 * workgroup, the record walk, the same tree) and are rounded to float32 once: the same bits every call.  No atomics.  gN is the
 * gradient of c sums[0] with respect to the image of (c), gnd with respect to the depth normals:
 * gsr_normals_from_depth_backward(gnd) gives the two images the backward accepts.  `workspace`: gsr_normals_workspace_bytes(W, H)
 * bytes, 16-byte aligned (that header's workspace: the same buffer serves the call that follows).
 *
 * dL_dout, normals and dL_dnormals must be finite: anything else is outside the contract (no fault, but unspecified values).
 * Every walk is bounded as in gsr_features.h: a tile's range is clipped to [0, D], a pixel visits min(n_contrib[p], range length)
 * entries, and an id outside [0, N) is skipped.  Stale or foreign buffers of the stated sizes give wrong numbers, never an access
 * out of bounds.  block_masks (optional, NULL is allowed) only let a wave pass over entries that cannot reach its block.
 *
 * All array pointers are device pointers and 16-byte aligned, except: the arrays of the frame are 4-byte aligned (xy and
 * conic_opacity may be columns of a wider record: their row strides are given in floats), `sums` is 4-byte aligned, and
 * `viewmatrix` is a host pointer to 16 floats.  The caller owns every byte: the library allocates nothing, enqueues everything on
 * `stream`, waits for nothing and reads nothing back.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL       a required pointer is NULL (frame, xy, conic_opacity, ranges, n_contrib, an array argument, viewmatrix,
 *                      workspace; `m` may be NULL); point_list is NULL while D > 0.
 *     GSR_E_DIMS       (a), (b): N < 1 or > 2^31 - 1, a viewmatrix entry not finite.  (c), (d): W or H < 1 or > GSR_FEATURES_MAX_SIDE,
 *                      N < 1 or > 2^31 - 1, D < 0 or > 2^30, xy_stride < 2, conic_opacity_stride < 4.  (e): W, H < 1 or W H > 2^28,
 *                      weight not finite.
 *     GSR_E_ALIGN      an array is not aligned as stated above.
 *     GSR_E_WORKSPACE  (e): workspace_bytes < gsr_normals_workspace_bytes(W, H).
 *     GSR_E_HIP        a launch failed.
 */
#ifndef GSR_NORMAL_RENDER_H
#define GSR_NORMAL_RENDER_H

#include "gsr.h"
#include "gsr_features.h"
#include "gsr_normals.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_NORMAL_RENDER_MIN_AXIS2 1e-24f   /* (a): a shorter axis column (squared) gives the zero normal */
#define GSR_NORMAL_RENDER_MIN_LENGTH 1e-3f   /* (e): a shorter blended normal does not count */

/* normals[N][3] = the camera-facing unit normal of every Gaussian, in camera space.  Every element is written. */
int gsr_gaussian_normals(int64_t N, const float *scales /* [N][3] */, const float *rotations /* [N][4] */, const float *means /* [N][3] */,
                         const float *viewmatrix /* host, 16 */, float *normals /* [N][3] */, void *stream);

/* Adds the derivative of (a) with respect to the stored quaternion into dL_drot[N][4]. */
int gsr_gaussian_normals_backward(int64_t N, const float *scales, const float *rotations, const float *means, const float *viewmatrix /* host, 16 */,
                                  const float *dL_dnormals /* [N][3] */, float *dL_drot /* [N][4] */, void *stream);

/* out[H][W][3] = sum_k w_k(p) normals[i_k].  Every element is written. */
int gsr_normal_render_forward(const GsrFeaturesFrame *frame, const float *normals /* [N][3] */, float *out /* [H][W][3] */, void *stream);

/* Adds the screen-space gradient of sum_p dL_dout[p] . out[p] into columns 3, 4, 6, 7, 9 and 10 of accumulators[N][16] and writes
 * dL_dnormals[N][3] (cleared first). */
int gsr_normal_render_backward(const GsrFeaturesFrame *frame, const float *normals /* [N][3] */, const float *dL_dout /* [H][W][3] */,
                               const float *out /* [H][W][3] */, float *accumulators /* [N][16] */, float *dL_dnormals /* [N][3] */, void *stream);

/* sums[2] = (sum m (1 - n_d . N / |N|), sum m) over the counted pixels; gN, gnd [H][W][3]: the gradient of weight / (W H) * sums[0]. */
int gsr_normal_consistency_loss(const float *Nimg /* [H][W][3] */, const float *n_d /* [H][W][3] */, const float *valid /* [H][W] */,
                                const float *m /* [H][W] or NULL */, int32_t W, int32_t H, float weight, float *gN, float *gnd, float *sums,
                                void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_NORMAL_RENDER_H */
