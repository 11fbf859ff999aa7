/*
 * gsr_antialias.h -- antialiased rendering of libgsr_hip.so: the opacity compensation of the screen-space blur, forward and backward.
 *
 * The classic forward adds h = 0.3 px^2 to the diagonal of every projected covariance and leaves the opacity alone, so a Gaussian
 * much smaller than a pixel is drawn as a 0.55-pixel blob at full opacity.  The antialiased mode (Mip-Splatting's 2D filter; the
 * `antialiasing` of the Inria rasterizer) keeps that blob's integral: with (a0, b, c0) the projected covariance before the blur and
 * a = a0 + h, c = c0 + h after it,
 *     det0 = a0 c0 - b^2        det1 = a c - b^2        rho = sqrt(max(0.000025, det0 / det1))        (0 < rho <= 1)
 *     effective opacity = opacity * rho
 * Radius, tile rectangle, conic, depth, colour, the sort and the blend are those of the classic mode; the blend kernels read the
 * effective opacity where they read the raw one (column 5 of the blend record, conic_opacity[3]).
 *
 * The mode is selected by one extra argument, `aa_scale`: a caller-owned array of N floats, 16-byte aligned.  The forward writes
 * rho there per Gaussian (0 for culled ones, as every per-Gaussian output); the backward reads it.
 *
 * Contract
 *   - aa_scale == NULL IS the classic call: gsr_forward_count_aa, gsr_forward_capacity_aa, gsr_backward_aa, gsr_backward_geom_aa and
 *     gsr_backward_camera_aa then launch the kernels of gsr_forward_count, gsr_forward_capacity (gsr_capacity.h), gsr_backward_flags
 *     (gsr_densify_stats.h), gsr_backward_geom_aux (gsr_aux_grads.h) and gsr_backward_camera (gsr_camera_grads.h).
 *   - gsr_forward_count_aa / gsr_forward_capacity_aa: the arguments of their namesakes plus aa_scale (out).  They store opacity * rho
 *     in the blend record and in conic_opacity[3].  gsr_forward_render follows gsr_forward_count_aa unchanged.
 *   - gsr_backward_aa: the arguments of gsr_backward_flags plus aa_scale (in, the forward's).  gsr_backward_geom_aa: those of
 *     gsr_backward_geom_aux plus it.  The blend half of an antialiased frame is gsr_backward_blend_flags, unchanged: it leaves
 *     g = dL/d(effective opacity) in column 10 of the accumulator records.  The per-Gaussian half then writes
 *     dL_dopacity = aa_scale * g and adds opacity * g * d(rho)/d(a, b, c) to the cotangent of the blurred covariance before it is
 *     chained to dL_dmean3D, dL_dscale and dL_drot; with k = 1 / (2 rho det1^2) where det0 / det1 > 0.000025 and k = 0 on the floor,
 *         d rho / d a =  k h (c c0 + b^2)      d rho / d c =  k h (a a0 + b^2)      d rho / d b = -k 2 b h (a + c0)
 *     (b the one parameter that fills both off-diagonal entries), evaluated at the backward's own (a, b, c) as its conic derivative
 *     is.  It reads scene->opacity, which the classic per-Gaussian half does not.
 *   - gsr_backward_camera_aa: gsr_backward_camera plus aa_scale (in).  The same term joins the camera gradient, at the forward's
 *     (a, b, c).  No float atomics: the sum stays bitwise reproducible.
 *   - Every other output is what the classic call gives for a scene whose opacity is opacity * aa_scale.
 *   - No allocation; no host synchronisation beyond that of the namesake.  N = 0 is fine (aa_scale is not looked at).
 *   - Errors, every one checked before anything is enqueued, in the namesake's order: aa_scale's alignment is checked with the
 *     namesake's other alignments (GSR_E_ALIGN), i.e. after its GSR_E_NULL / GSR_E_DIMS checks and before GSR_E_OVERFLOW (backward) and
 *     GSR_E_WORKSPACE.  gsr_backward_camera_aa: GSR_E_NULL (scene, camera, scene->opacity with the other scene arrays), GSR_E_DIMS,
 *     GSR_E_NULL (dL_dcamera, geom, geom->radii, geom->clamped_state), GSR_E_ALIGN, GSR_E_WORKSPACE.
 *   - Nothing else changes: gsr.h, its structs, GSR_ABI_VERSION, workspace sizes and every existing entry point are as before.
 */
#ifndef GSR_ANTIALIAS_H
#define GSR_ANTIALIAS_H

#include "gsr_camera_grads.h"
#include "gsr_capacity.h"
#include "gsr_densify_stats.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_AA_BLUR 0.3f           /* h: what the forward adds to the diagonal of the projected covariance */
#define GSR_AA_RATIO_FLOOR 0.000025f /* the floor under det0 / det1 */

int gsr_forward_count_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, void *geom_ws, size_t geom_ws_bytes,
                         int64_t *num_rendered, float *aa_scale, void *stream);
int gsr_forward_capacity_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning,
                            const GsrImage *image, void *geom_ws, size_t geom_ws_bytes, void *bin_ws, size_t bin_ws_bytes,
                            int64_t shape_hint, float *aa_scale, void *stream);
int gsr_backward_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning,
                    const GsrImage *image, const GsrPixelGrads *pixel_grads, const GsrGrads *grads, float *dL_dinv_depths, void *ws,
                    size_t ws_bytes, uint32_t flags, const float *aa_scale, void *stream);
int gsr_backward_geom_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrGrads *grads,
                         float *dL_dinv_depths, void *ws, size_t ws_bytes, const float *aa_scale, void *stream);
int gsr_backward_camera_aa(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, float *dL_dcamera, const void *ws,
                           size_t ws_bytes, void *scratch, size_t scratch_bytes, const float *aa_scale, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_ANTIALIAS_H */
