/*
 * gsr_depth_corr.h -- a Pearson-correlation depth loss in libgsr_hip.so, for depth priors that are known only up to a scale and a
 * shift per image (monocular depth maps): loss = 1 - rho(rendered inverse depth, target), its exact pixel gradient, and the
 * least-squares map of the target onto the render.  An image-space stage beside gsr_aux_grads.h's masked L1 (gsr_depth_loss_grad):
 * no rasterizer kernel, struct or entry point changes; the gradient goes where gsr_depth_loss_grad's goes (GsrPixelGrads.dL_dinv_depth).
 *
 * The function.  r = the rendered inverse depth (GsrImage.inv_depth), t = the target (any relative depth), m = weights >= 0 (NULL:
 * all ones), all W x H float32, row-major.  With
 *     M  = sum m              mu_r = sum m r / M                 mu_t = sum m t / M
 *     Vr = sum m (r - mu_r)^2 / M      Vt = sum m (t - mu_t)^2 / M      C = sum m (r - mu_r)(t - mu_t) / M
 * the call computes
 *     rho    = C / sqrt(Vr Vt)
 *     loss   = 1 - rho
 *     grad_i = -weight m_i / (M sqrt(Vr Vt)) [ (t_i - mu_t) - (C / Vr)(r_i - mu_r) ]          (= weight dloss/dr_i, exactly)
 *     fit    = (rho, s, b, M),  s = C / Vt,  b = mu_r - s mu_t       (the least-squares map of the target onto the render: r ~ s t + b)
 * loss and gradient do not change under t -> a t + b with a > 0 (a < 0 turns loss into 2 - loss), nor under a shift or a positive
 * scaling of r: sum grad_i = 0 and sum grad_i r_i = 0.
 *
 * Degenerate input.  The frame is degenerate when M == 0, or Vr <= GSR_DEPTH_CORR_MIN_REL_VAR * (sum m r^2 / M), or the same test
 * fails for t: a 1-pixel image, an all-zero mask, a render that is all background (r = 0), a constant target.  Then rho := 0:
 * loss = 1, grad is all +0 and fit = (0, 0, 0, M).  No NaN comes out of finite input.
 *
 * Arithmetic.  The six sums (sum m, m r, m t, m r^2, m t^2, m r t) are float64 at every level: a lane adds its pixels in ascending
 * order (4 consecutive pixels per round, rounds GSR_DEPTH_CORR_MAX_BLOCKS * GSR_DEPTH_CORR_BLOCK_PIXELS pixels apart), a wave adds
 * its 64 lanes in a butterfly, a workgroup its 4 waves, and leaves one partial record in the workspace; a launch of one workgroup
 * adds the records -- each thread every 256th in ascending order, then the same butterfly -- and forms the moments, the test above,
 * rho, loss and fit in float64, each rounded to float32 once.  The gradient pass forms (t_i - mu_t) and (r_i - mu_r) in float64
 * against the float64 means and rounds the finished product once.  No float atomics and no host wait: two calls on the same inputs
 * give the same bits in grad, loss and fit.
 *
 * Outputs (device memory, overwritten; nothing is accumulated across calls):
 *     grad   (H, W), or NULL for the loss and the fit alone.  It must not overlap an input.
 *     loss   1 float: 1 - rho.
 *     fit    4 floats (rho, s, b, M), or NULL.
 *
 * Images are 16-byte aligned, as in gsr.h; loss and fit are 4-byte aligned: a row of a (V, 4) tensor qualifies.  workspace: device
 * memory of at least gsr_depth_corr_workspace_bytes(W, H) bytes, 16-byte aligned, its contents undefined on entry and on return; one
 * workspace serves one call at a time.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL       rendered, target, loss or workspace is NULL.
 *     GSR_E_DIMS       W or H <= 0, W * H > 2^28, weight not finite.
 *     GSR_E_ALIGN      an image or the workspace not 16-byte aligned, loss or fit not 4-byte aligned.
 *     GSR_E_WORKSPACE  workspace_bytes < gsr_depth_corr_workspace_bytes(W, H).
 *     GSR_E_HIP        a launch failed.
 */
#ifndef GSR_DEPTH_CORR_H
#define GSR_DEPTH_CORR_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_DEPTH_CORR_FIT_FLOATS 4       /* fit = (rho, s, b, M) */
#define GSR_DEPTH_CORR_BLOCK_PIXELS 1024  /* pixels a workgroup takes per round: 256 threads x 4 pixels */
#define GSR_DEPTH_CORR_MAX_BLOCKS 1024    /* workgroups of the sums at most (= partial records); larger images take several rounds */
#define GSR_DEPTH_CORR_RECORD_BYTES 64    /* one partial record: 6 float64 sums, 2 of padding */
#define GSR_DEPTH_CORR_MIN_REL_VAR 1e-12  /* a variance at or below this fraction of the mean square is no variance: the frame is degenerate */

/* Bytes of workspace gsr_depth_corr_loss_grad needs for a W x H image (0 if W or H <= 0 or W * H > 2^28): the partial records and
 * one more record that carries the moments from the finishing launch to the gradient pass. */
size_t gsr_depth_corr_workspace_bytes(int32_t W, int32_t H);

int gsr_depth_corr_loss_grad(const float *rendered, const float *target, const float *mask /* may be NULL */,
                             float *grad /* may be NULL: loss only */, float *loss /* device[1], overwritten with 1 - rho */,
                             float *fit /* device[4] or NULL */, int32_t W, int32_t H, float weight, void *workspace, size_t workspace_bytes,
                             void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_DEPTH_CORR_H */
