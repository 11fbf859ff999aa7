/*
 * gsr_camera_grads.h -- gradients of libgsr_hip.so's loss with respect to the camera: dL/dview, dL/dproj, dL/dcampos.
 *
 * gsr_backward treats the camera as a constant.  gsr_backward_camera takes the screen-space gradients that a backward left in its
 * workspace and chains them to the three camera inputs of the forward, each taken as independent (the caller who builds proj
 * from view, or campos from view, composes the three itself):
 *     dL_dcamera[0..15]   dL/dview, row-major, in the row-vector convention of the kernels: p_view = [p, 1] @ view
 *     dL_dcamera[16..31]  dL/dproj, row-major, for the full projection passed as GsrCamera.proj: p_hom = [p, 1] @ proj
 *     dL_dcamera[32..34]  dL/dcampos
 *     dL_dcamera[35]      0
 * This is the true derivative of the forward (preprocess and blend) at the given inputs, not a reference-compatible quirk
 * set like gsr_backward's: the 2D mean through p_hom.xy / (p_hom.w + 1e-7), the conic through the forward's
 * Sigma2D = J W Sigma3D W^T J^T (W = view[0:3, 0:3], with the derivative of the 1.3 tan(fov) clamp in J, the 0.3 blur and
 * 1/det^2), 1/depth through view column 2 when the aux backward (gsr_aux_grads.h) left dL/dinvd, and the colour of unclamped
 * channels through dir = normalize(mean - campos).  Sigma3D is GsrGeom.cov3D, or is recomputed from the scene with its
 * scale_modifier when cov3D is NULL; d(colour)/d(dir) is GsrGeom.sh_dir_grad when given, else formed from scene->sh.
 * Culled Gaussians (radius 0) contribute nothing; radii, tile rectangles and the sort order get no gradient.  The colour
 * gradients the blend backward accumulates pass the forward's 0.99 alpha cap as gsr_backward's do.
 *
 * Contract
 *   - Call it after gsr_backward, gsr_backward_aux, or gsr_backward_blend[_aux] (with or without the geom half), with the same
 *     scene, camera, geom and workspace `ws`, on the same stream.  It reads the accumulator records that call left
 *     (gsr_backward_accumulators_offset) and writes nothing but dL_dcamera and `scratch`.
 *   - dL_dcamera: 36 device floats, 16-byte aligned, overwritten (the caller clears nothing).
 *   - scratch: at least gsr_backward_camera_scratch_bytes(N) bytes of device memory, 16-byte aligned (may be NULL when that is 0).
 *   - The sum over Gaussians is bitwise reproducible: the same inputs give the same bits, with no float atomics.
 *   - No allocation and no host synchronisation.  N = 0, D = 0 and frames where every Gaussian is culled give zeros.
 *   - Errors, every one checked before anything is enqueued: GSR_E_NULL, GSR_E_DIMS (as gsr_backward), GSR_E_NULL (dL_dcamera,
 *     geom, geom->radii, geom->clamped_state), GSR_E_ALIGN, GSR_E_WORKSPACE (ws or scratch missing or too small).
 *   - Nothing else changes: gsr.h, its structs, workspace sizes and every existing entry point are as before.
 */
#ifndef GSR_CAMERA_GRADS_H
#define GSR_CAMERA_GRADS_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_CAMERA_GRAD_FLOATS 36

size_t gsr_backward_camera_scratch_bytes(int64_t N);
int gsr_backward_camera(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, float *dL_dcamera, const void *ws,
                        size_t ws_bytes, void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_CAMERA_GRADS_H */
