/*
 * gsr_plane_depth.h -- the ray-plane intersection depth of PGSR, RaDe-GS and GOF over the lists of a rendered frame, and its
 * gradient, in libgsr_hip.so.  Every other depth of the library takes a Gaussian for a fronto-parallel card at 1 / z of its centre.
 * Here a flat Gaussian is a piece of its plane: with n its camera-space normal (gsr_normal_render.h (a)), mu = p_v its camera-space
 * centre and r(p) the ray of pixel p (gsr_normals.h: rx = ((2x + 1) / W - 1) tan_fovx, ry likewise, rz = 1) the inverse depth at
 * which the ray meets the plane is
 *
 *     m_k(p) = (n . r(p)) / (n . mu) = invd_k + gx_k (p.x - x_k) + gy_k (p.y - y_k)
 *     gx = n.x (2 tan_fovx / W) / (n . mu),     gy = n.y (2 tan_fovy / H) / (n . mu)
 *
 * affine in the pixel, exact, and 1 / z of the centre at the projected centre (x_k, y_k); x_k, y_k, invd_k are the staged xy and
 * 1 / depth a GsrDistortionFrame carries.  The image is out[p] = sum_k w_k(p) m_k(p), an inverse depth times coverage like the
 * forward's depth image.  Stages of their own behind the forward and between the two halves of the backward, like gsr_distortion.h
 * and gsr_normal_render.h: no rasterizer kernel, struct or entry point changes, nothing is binned or sorted again.
 *
 * Every float32 step is stated: products left to right, nothing contracted unless a fused multiply-add is named; every division and
 * square root is IEEE.
 *
 * (a) gsr_plane_slopes.  One thread per Gaussian i, from normals[i] = n (gsr_gaussian_normals' output), scales[i] = (s0, s1, s2),
 * means[i] = p, the 16 HOST floats of `viewmatrix` (V[r][j] = viewmatrix[4 r + j], row-vector convention), tan_fovx, tan_fovy, W, H:
 *
 *   1. p_v[j] = ((V[0][j] p0 + V[1][j] p1) + V[2][j] p2) + V[3][j]   (j = 0, 1, 2; gsr_normal_render.h step 4)
 *   2. t = (n0 p_v0 + n1 p_v1) + n2 p_v2
 *   3. l = sqrt((p_v0 p_v0 + p_v1 p_v1) + p_v2 p_v2)
 *   4. lo = fmin(fmin(s0, s1), s2),   mid = fmax(fmin(s0, s1), fmin(fmax(s0, s1), s2))      (the smallest and the middle scale)
 *   5. The Gaussian FALLS BACK, slopes[i] = (0, 0) exactly (it keeps its centre depth), if any of
 *          n0 == 0 and n1 == 0 and n2 == 0                              the zero normal
 *          !(p_v2 > GSR_PLANE_DEPTH_NEAR = 0.2f)                        not above the forward's near plane
 *          !(-t >= GSR_PLANE_DEPTH_MIN_COS * l)                         a grazing ray (MIN_COS = 0.1f; a NaN falls back)
 *          !(lo <= GSR_PLANE_DEPTH_MAX_FLATNESS * mid)                  not flat (MAX_FLATNESS = 0.5f): the normal of a round Gaussian
 *                                                                       is a tie-break of step 1 of gsr_normal_render.h, not a
 *                                                                       surface direction
 *   6. Otherwise kx = (2 * tan_fovx) / (float)W,  ky = (2 * tan_fovy) / (float)H,
 *          slopes[i] = ((n0 * kx) / t,  (n1 * ky) / t)
 *
 * Every decision of step 5 is the float32 comparison written there, so a float64 restatement that takes the decisions from the same
 * float32 values follows the same branch.  Every element of slopes is written.
 *
 * (b) gsr_plane_depth_forward.  The applied entries k = 0 ... of a pixel and their weights w_k = alpha_k T_k are exactly those of
 * gsr_features.h (the same float32 power expression, alpha = min(0.99, o exp(power)) with the forward's exp, the two skip tests,
 * T <- T (1 - alpha) from T = 1, the walk up to n_contrib[p]).  With dx = x_k - p.x, dy = y_k - p.y as the forward forms them,
 * invd = inv_depth[i_k * inv_depth_stride] and (gx, gy) = slopes[i_k], from out[p] = 0, per applied entry in list order:
 *
 *          m   = fma(-gx, dx, fma(-gy, dy, invd))
 *          m   <- fmin(fmax(m, invd * 0.25f), invd * 4.0f)        (GSR_PLANE_DEPTH_MAX_RATIO = 4: a plane seen near its horizon must
 *                                                                  not blend a zero or negative inverse depth; the entry is CLAMPED
 *                                                                  where this changes m)
 *          out[p] <- fma(w_k, m, out[p])
 *
 * One running register per pixel, no atomics: the same bits every call, on every stream, with or without block_masks.  Every pixel
 * is written; pixels without an applied entry, pixels of a tile without a list and every pixel of a frame with D = 0 are 0.  At
 * slopes (0, 0) m is invd exactly, so the image is bit for bit gsr_features_forward of the column invd at C = 1.
 *
 * (c) gsr_plane_depth_backward.  g = dL_dout[p], out[p] the stored forward image (not recomputed).  Per pixel, once:
 *
 *          total = g * out[p]          P = 0, T = 1
 *
 * and per applied entry, in list order (Gexp = exp(power), o = opacity, m as in (b), clamp included):
 *
 *          u  = g * m
 *          w  = alpha * T
 *          P  <- P + w * u
 *          R  = total - P                      (the entries behind k)
 *          q  = T * u - R / (1 - alpha)        (dL/dalpha: the gradient passes the 0.99 cap)
 *          gd = Gexp * q
 *          h  = o * gd        hx = h * dx      hy = h * dy
 *          wg = w * g
 *          nine per-(pixel, entry) values:  hx, hy, hx * dx, hx * dy, hy * dy, gd,  wg, wg * (-dx), wg * (-dy)
 *                                           (the last three are 0 for a clamped entry: it contributes through its weight only)
 *          T  <- T * (1 - alpha)
 *
 * the total-minus-prefix form of gsr_normal_render.h (d), with its stated limit.  An 8x8 pixel block sums each of the nine values
 * over its pixels in gsr_distortion.h's fixed order to S1, S2, Sxx, Sxy, Syy, Sop, S0, Sx, Sy and ADDS, with that header's constants,
 *
 *     accumulators[i_k] column 3   (2 a' S1 + b' S2) * (0.5 W)        column 4   (2 c' S2 + b' S1) * (0.5 H)
 *                       column 6   -0.5 Sxx     column 7   -0.5 Sxy     column 9   -0.5 Syy        column 10  Sop
 *     dL_dplane_moments[i_k]       (S0, Sx, Sy) = (sum w g, sum w g (p.x - x_k), sum w g (p.y - y_k))
 *
 * and touches no other accumulator column: column 11 (dL/d(1/depth)) stays the centre-depth terms' alone -- the dependence of m on
 * the Gaussian's centre travels through the moments and (d), not through the staged xy and 1 / depth.  The call CLEARS
 * dL_dplane_moments first.  One float atomic per (block, applied entry, value): the last bits of a row that several blocks or tiles
 * touch may differ from run to run.
 *
 * (d) gsr_plane_slopes_backward.  One thread per Gaussian, no atomics; p_v, t, the branch of step 5 and (gx, gy) are recomputed as
 * in (a) and the branch is held constant.  With (S0, Sx, Sy) = dL_dplane_moments[i], invd = 1 / p_v2, kx, ky as in step 6:
 *
 *          M = (invd * S0 + gx * Sx) + gy * Sy                                       (= sum_p w g m over the unclamped entries)
 *          R = ((p_v0 * invd) * S0 + kx * Sx,  (p_v1 * invd) * S0 + ky * Sy,  S0)    (= sum_p w g r(p))
 *          dL/dn[j]   = (R[j] - M * p_v[j]) / t
 *          dL/dp_v[j] = -((M * n[j]) / t)
 *     fallback branch:  dL/dn = (0, 0, 0),   dL/dp_v = (0, 0, -((invd * invd) * S0))   (invd = 0 where !(p_v2 > 0))
 *
 *          dL_dmean3D[i][r] += (V[r][0] dL/dp_v0 + V[r][1] dL/dp_v1) + V[r][2] dL/dp_v2        (ADDED: one read-modify-write)
 *          dL_dnormals[i]    = dL/dn                                                            (WRITTEN, every row)
 *
 * gsr_gaussian_normals_backward then carries dL_dnormals on to dL_drot (it adds; with the normal image's stage present its buffer
 * and this one are summed first, or the call is made twice).  The term's DIRECT dependence on `viewmatrix` (step 1, and the
 * normal's own) is left out of the camera gradient, as the normals' is: camera_grad carries the screen-space columns of (c) only.
 *
 * dL_dout, slopes, inv_depth, scales and means must be finite: anything else is outside the contract (no fault, but unspecified
 * values).  Every walk is bounded as in gsr_features.h: a tile's range is clipped to [0, D], a pixel visits min(n_contrib[p], range
 * length) entries, and an id outside [0, N) is skipped.  Stale or foreign buffers of the stated sizes give wrong numbers, never an
 * access out of bounds.  block_masks (optional, NULL is allowed) only let a wave pass over entries that cannot reach its block.
 *
 * All array pointers are device pointers and 16-byte aligned, except: the arrays of the frame are 4-byte aligned (xy,
 * conic_opacity and inv_depth may be columns of a wider record: their row strides are given in floats), and `viewmatrix` is a host
 * pointer to 16 floats.  The caller owns every byte: the library allocates nothing, enqueues everything on `stream`, waits for
 * nothing and reads nothing back.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL   a required pointer is NULL (frame, xy, conic_opacity, inv_depth, ranges, n_contrib, an array argument,
 *                  viewmatrix); point_list is NULL while D > 0.
 *     GSR_E_DIMS   (a), (d): N < 1 or > 2^31 - 1, a viewmatrix entry not finite, tan_fovx or tan_fovy not finite or <= 0, W or H < 1
 *                  or > GSR_FEATURES_MAX_SIDE.  (b), (c): W or H < 1 or > GSR_FEATURES_MAX_SIDE, N < 1 or > 2^31 - 1, D < 0 or > 2^30,
 *                  xy_stride < 2, conic_opacity_stride < 4, inv_depth_stride < 1.
 *     GSR_E_ALIGN  an array is not aligned as stated above.
 *     GSR_E_HIP    a launch failed.
 */
#ifndef GSR_PLANE_DEPTH_H
#define GSR_PLANE_DEPTH_H

#include "gsr.h"
#include "gsr_distortion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_PLANE_DEPTH_MIN_COS 0.1f        /* (a): -n . p_v / |p_v| below this is a grazing ray */
#define GSR_PLANE_DEPTH_MAX_FLATNESS 0.5f   /* (a): smallest scale / middle scale above this is not flat */
#define GSR_PLANE_DEPTH_NEAR 0.2f           /* (a): the forward's near plane */
#define GSR_PLANE_DEPTH_MAX_RATIO 4.0f      /* (b): m is held to [invd / 4, 4 invd] */

/* slopes[N][2] = (gx, gy), (0, 0) on the fallback branch.  Every element is written. */
int gsr_plane_slopes(int64_t N, const float *normals /* [N][3] */, const float *scales /* [N][3] */, const float *means /* [N][3] */,
                     const float *viewmatrix /* host, 16 */, float tan_fovx, float tan_fovy, int32_t W, int32_t H, float *slopes /* [N][2] */,
                     void *stream);

/* Adds the means' share of (d) into dL_dmean3D[N][3] and writes dL_dnormals[N][3]. */
int gsr_plane_slopes_backward(int64_t N, const float *normals, const float *scales, const float *means, const float *viewmatrix /* host, 16 */,
                              float tan_fovx, float tan_fovy, int32_t W, int32_t H, const float *dL_dplane_moments /* [N][3] */,
                              float *dL_dmean3D /* [N][3] */, float *dL_dnormals /* [N][3] */, void *stream);

/* out[H][W] = sum_k w_k(p) m_k(p).  Every element is written. */
int gsr_plane_depth_forward(const GsrDistortionFrame *frame, const float *slopes /* [N][2] */, float *out /* [H][W] */, void *stream);

/* Adds the screen-space gradient of sum_p dL_dout[p] out[p] into columns 3, 4, 6, 7, 9 and 10 of accumulators[N][16] and writes
 * dL_dplane_moments[N][3] (cleared first). */
int gsr_plane_depth_backward(const GsrDistortionFrame *frame, const float *slopes /* [N][2] */, const float *dL_dout /* [H][W] */,
                             const float *out /* [H][W] */, float *accumulators /* [N][16] */, float *dL_dplane_moments /* [N][3] */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_PLANE_DEPTH_H */
