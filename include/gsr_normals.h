/*
 * gsr_normals.h -- surface normals from the rendered depth in libgsr_hip.so, their exact gradient back to the two images the backward
 * accepts, and a cosine loss against a normal prior (a monocular normal network, a renderer's normal pass).  An image-space stage
 * beside gsr_aux_grads.h's losses and gsr_depth_corr.h: no rasterizer kernel, struct or entry point changes; the two gradient images
 * go where gsr_depth_loss_grad's and gsr_alpha_loss_grad's go (GsrPixelGrads.dL_dinv_depth and GsrPixelGrads.dL_dalpha).
 *
 * The function.  Dinv = the rendered expected inverse depth (GsrImage.inv_depth, sum_k w_k / z_k), T = GsrImage.final_T, both W x H
 * float32, row-major; tan_fovx, tan_fovy, W, H the camera's; alpha_min a threshold on the coverage.  Every step below is one float32
 * operation, rounded once, in the order written (no fused multiply-add):
 *     ray     rx = ((float)(2x + 1) / (float)W - 1) * tan_fovx,  ry = ((float)(2y + 1) / (float)H - 1) * tan_fovy,  rz = 1
 *             (the inverse of the forward's pixel convention: integer pixel coordinates are the sample positions)
 *     point   A = 1 - T.  The pixel is DEFINED iff A and Dinv are finite, A >= alpha_min and Dinv > 0.  Then z = A / Dinv (the
 *             harmonic-mean view depth of what was blended) and P = (z rx, z ry, z), in camera space.
 *     normal  a = P(x, y+1) - P(x, y-1),  b = P(x+1, y) - P(x-1, y),  N = a x b:
 *                 Nx = ay bz - az by      Ny = az bx - ax bz      Nz = ax by - ay bx
 *                 |N|^2 = (Nx Nx + Ny Ny) + Nz Nz,  |a|^2 and |b|^2 in the same order
 *             The pixel is VALID iff x-1, x+1, y-1, y+1 lie inside the image, the pixel and its four neighbours are defined, and
 *                 |N|^2 > GSR_NORMALS_MIN_NORM2 * (|a|^2 * |b|^2)   and   |N|^2 <= FLT_MAX
 *             (|N|^2 / (|a|^2 |b|^2) is the squared sine of the angle between the two differences: the test does not depend on the
 *             scene's scale).  Then n = N / sqrt(|N|^2), component by component.  A fronto-parallel surface gives (0, 0, -1): normals
 *             face the camera.  Every other pixel gets n = (0, 0, 0) and valid = 0.  No NaN or Inf comes out of finite input.
 * Validity is decided by exactly these float32 comparisons, so a float64 restatement that takes its decisions from the same float32
 * values marks the same pixels.
 *
 * The gradient (gsr_normals_from_depth_backward).  For g = dL/dn (H x W x 3) and the validity pattern held fixed, with
 *     u_p  = (g_p - n_p (n_p . g_p)) / |N_p|         (0 where p is not valid)
 *     c1_p = b_p x u_p = dL/da_p                     c2_p = u_p x a_p = dL/db_p
 * the gradient of the point of pixel q = (x, y) is GATHERED from its four neighbours, in this order,
 *     dL/dP(q) = ((c1(x, y-1) - c1(x, y+1)) + c2(x-1, y)) - c2(x+1, y)          (a neighbour outside the image contributes 0)
 *     dL/dz(q) = (rx dL/dPx + ry dL/dPy) + dL/dPz
 *     gD(q) = dL/dz (-z / Dinv)           gA(q) = dL/dz (1 / Dinv)
 * gA is the gradient with respect to A = 1 - T, the alpha image, not T.  The depth of a pixel reaches the normals of a radius-2
 * stencil.  Nothing is scattered: no float atomics, no host wait, the same bits every call whatever the workspace held, on any
 * stream.  gD and gA are +0 at pixels that are not defined and wherever no valid normal depends on the pixel.
 *
 * The loss (gsr_normals_loss_grad).  target = t (H x W x 3 float32, any length), R = an optional row-major 3 x 3 rotation in HOST
 * memory (NULL: identity; a world-space target passes the view rotation, a camera-space target in another axis convention a flip),
 * mask = m >= 0 (W x H, NULL: all ones).  In float32, in this order:
 *     s   = R t: s_i = (R_i0 tx + R_i1 ty) + R_i2 tz            |s|^2 = (sx sx + sy sy) + sz sz
 *     th  = s / sqrt(|s|^2); a pixel whose |s|^2 is 0 or not finite is not valid for the loss
 *     g   = -(weight m) th at valid pixels, 0 elsewhere
 *     loss_sum   = sum over valid pixels of m (1 - n . th)      weight_sum = sum over valid pixels of m
 *     gD, gA     = the gradient above of g: weight * d loss_sum / d Dinv and weight * d loss_sum / d A, bit for bit what
 *                  gsr_normals_from_depth_backward gives for that g
 * `weight` is applied as given (the Python wrapper passes weight / (W H), gsr_depth_loss_grad's normalisation).  The two sums are
 * float64 at every level (csrc/fixed_sum.h): a lane adds the terms of its pixels in ascending order, a workgroup leaves one partial
 * record per GSR_NORMALS_TILE_W x GSR_NORMALS_TILE_H tile it walks (at most GSR_NORMALS_MAX_BLOCKS workgroups), one finishing
 * workgroup adds the records in a fixed order and rounds each total to float32 once.
 *
 * Outputs (device memory, overwritten; nothing is accumulated across calls).  They must not overlap an input.
 *     normals_out  (H, W, 3)                valid_out  (H, W) float 0 / 1, or NULL
 *     gD, gA       (H, W) each; gsr_normals_loss_grad takes both NULL for the loss alone (one without the other is GSR_E_NULL)
 *     sums         2 floats: (loss_sum, weight_sum)
 * Images are 16-byte aligned, as in gsr.h; sums is 4-byte aligned.  workspace: device memory of at least
 * gsr_normals_workspace_bytes(W, H) bytes, 16-byte aligned, its contents undefined on entry and on return; one workspace serves one
 * call at a time.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL       a required pointer is NULL (everything but valid_out, R, mask, and gD and gA together).
 *     GSR_E_DIMS       W or H <= 0, W * H > 2^28, a tangent not finite or <= 0, alpha_min or weight not finite.
 *     GSR_E_ALIGN      an image or the workspace not 16-byte aligned, sums not 4-byte aligned.
 *     GSR_E_WORKSPACE  workspace_bytes < gsr_normals_workspace_bytes(W, H).
 *     GSR_E_HIP        a launch failed.
 */
#ifndef GSR_NORMALS_H
#define GSR_NORMALS_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_NORMALS_MIN_NORM2 1e-12f     /* |N|^2 at or below this fraction of |a|^2 |b|^2 is no normal: the differences are parallel to 1e-6 rad */
#define GSR_NORMALS_ALPHA_MIN 0.5f       /* the default alpha_min of the Python surface */
#define GSR_NORMALS_TILE_W 32            /* pixels a workgroup takes at a time: a 32 x 8 tile, one pixel per thread, a 2-pixel halo */
#define GSR_NORMALS_TILE_H 8             /* (the loss leaves one partial record per workgroup, a workgroup walks whole tiles) */
#define GSR_NORMALS_MAX_BLOCKS 2048      /* workgroups of the loss at most (= partial records); larger images take several tiles each */
#define GSR_NORMALS_RECORD_BYTES 16      /* one partial record: 2 float64 sums */
#define GSR_NORMALS_SUMS_FLOATS 2        /* sums = (loss_sum, weight_sum) */

/* Bytes of workspace the two gradient calls need for a W x H image (0 if W or H <= 0 or W * H > 2^28): the partial records. */
size_t gsr_normals_workspace_bytes(int32_t W, int32_t H);

int gsr_normals_from_depth(const float *Dinv, const float *final_T, float tan_fovx, float tan_fovy, int32_t W, int32_t H, float alpha_min,
                           float *normals_out, float *valid_out /* may be NULL */, void *stream);

int gsr_normals_from_depth_backward(const float *Dinv, const float *final_T, float tan_fovx, float tan_fovy, int32_t W, int32_t H, float alpha_min,
                                    const float *dL_dnormals, float *gD, float *gA, void *workspace, size_t workspace_bytes, void *stream);

int gsr_normals_loss_grad(const float *Dinv, const float *final_T, const float *target, const float *R /* host[9] or NULL: identity */,
                          const float *mask /* may be NULL */, float tan_fovx, float tan_fovy, int32_t W, int32_t H, float alpha_min, float weight,
                          float *gD /* NULL with gA: loss only */, float *gA, float *sums /* device[2], overwritten */, void *workspace,
                          size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_NORMALS_H */
