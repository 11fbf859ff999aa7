/*
 * gsr_aux_grads.h -- backward of libgsr_hip.so through the inverse-depth and alpha images, and their L1 losses.
 *
 * The forward renders two images besides colour (gsr.h GsrImage): the expected inverse depth Dinv = sum_k alpha_k T_k invd_k
 * (GsrImage.inv_depth, invd_k = 1 / the view depth of Gaussian k) and, implicitly, the alpha image A = 1 - final_T.  gsr_backward
 * takes a gradient for the colour image only.  The entry points here take all three:
 *     gD = dL/dDinv (H x W), gA = dL/dA (H x W), next to dL_dpixels (H x W x 3).
 * Per list entry the blend backward then uses
 *     c_k . dpix + gD invd_k        in place of c_k . dpix,
 *     T_final (bg . dpix - gA)      in place of the background term T_final (bg . dpix)   (dA/dalpha_k = T_final / (1 - alpha_k)),
 * and accumulates dL/dinvd_k = sum over pixels of alpha_k T_k gD.  The per-Gaussian half adds the true derivative of invd = 1/z
 * through the view depth z = view[2] m0 + view[6] m1 + view[10] m2 + view[14]:
 *     dL_dmean3D += -invd^2 dL/dinvd (view[2], view[6], view[10])        (visible Gaussians)
 * beside the reference's own mean terms (not through its dt transform, so without that transform's view[j][3] offset).  The
 * screen-space part -- dL/dalpha into mean2D, conic and opacity -- flows on as the colour image's does.
 *
 * Contract
 *   - gsr_backward_aux, gsr_backward_blend_aux and gsr_backward_geom_aux take the arguments of gsr_backward,
 *     gsr_backward_blend and gsr_backward_geom, with dL_dpixels replaced by a GsrPixelGrads.  The dL_dpixels rules are those
 *     of gsr_backward; here it may be NULL (no colour gradient).
 *   - At least one of the three pixel gradients is non-NULL.  dL_dinv_depth and dL_dalpha are W x H floats, row-major,
 *     16-byte aligned; a NULL one counts as zeros.
 *   - dL_dinv_depth needs records that carry 1/depth: GsrGeom.blend_records (the forward's own), or GsrGeom.depths for the
 *     re-pack from xy / conic_opacity / rgb.  Records re-packed without depths carry invd = 0, so dL_dinv_depth with neither is
 *     GSR_E_NULL rather than a silent zero gradient.
 *   - dL_dinv_depths (optional, [N] floats): dL/dinvd per Gaussian.  It is also column 11 of the accumulator records in the
 *     backward workspace (gsr_backward_accumulators_offset), as dL_dcolor / dL_dmean2D / dL_dconic are columns 0-9.
 *   - D == 0 gives zero blend gradients, as gsr_backward does.  A capacity-mode frame (gsr_capacity.h) is handled as in
 *     gsr_backward: binning->D is the forward's shape hint.
 *   - The halves pair up as gsr_backward_blend / gsr_backward_geom do, and an aux half pairs only with an aux half:
 *     gsr_backward_geom_aux reads the dL/dinvd that gsr_backward_blend_aux left in the workspace.
 *   - gsr_backward_aux with dL_dinv_depth = dL_dalpha = NULL is gsr_backward, bit for bit (the same kernels run).
 *   - Errors, every one checked before anything is enqueued, in gsr_backward's order: GSR_E_DIMS, GSR_E_NULL, GSR_E_ALIGN,
 *     GSR_E_OVERFLOW (binning->D), GSR_E_WORKSPACE.
 *
 * Losses (no host sync; loss_sum is a device float, overwritten):
 *   gsr_depth_loss_grad:  loss_sum = sum |r - t| mask,  grad = weight mask sign(r - t)  with r = rendered (W x H)
 *   gsr_alpha_loss_grad:  the same with r = 1 - final_T (the alpha image is not made first)
 *   sign(0) = +1 as in gsr_l1_loss_grad.  mask may be NULL (all ones) and so may grad (the loss only).  loss_sum over the
 *   pixels is what gsr_depth_loss sums; divide by W H for the reference's mean.  Errors: GSR_E_NULL, GSR_E_DIMS.
 */
#ifndef GSR_AUX_GRADS_H
#define GSR_AUX_GRADS_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct GsrPixelGrads {
    const float *dL_dpixels;    /* H x W x 3 or NULL */
    const float *dL_dinv_depth; /* H x W or NULL: dL / d(GsrImage.inv_depth) */
    const float *dL_dalpha;     /* H x W or NULL: dL / d(1 - GsrImage.final_T) */
} GsrPixelGrads;

int gsr_backward_aux(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning,
                     const GsrImage *image, const GsrPixelGrads *pixel_grads, const GsrGrads *grads, float *dL_dinv_depths, void *ws,
                     size_t ws_bytes, void *stream);
int gsr_backward_blend_aux(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrBinning *binning,
                           const GsrImage *image, const GsrPixelGrads *pixel_grads, float *payload, void *ws, size_t ws_bytes, void *stream);
int gsr_backward_geom_aux(const GsrScene *scene, const GsrCamera *camera, const GsrGeom *geom, const GsrGrads *grads,
                          float *dL_dinv_depths, void *ws, size_t ws_bytes, void *stream);

int gsr_depth_loss_grad(const float *rendered, const float *target, const float *mask, float *grad, float *loss_sum, int32_t W,
                        int32_t H, float weight, void *stream);
int gsr_alpha_loss_grad(const float *final_T, const float *target_alpha, const float *mask, float *grad, float *loss_sum, int32_t W,
                        int32_t H, float weight, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_AUX_GRADS_H */
