/*
 * gsr_weighted_loss.h -- per-pixel loss weights for the colour loss in libgsr_hip.so: the weighted twins of gsr_l1_loss_grad
 * (gsr.h) and gsr_l1_dssim_loss_grad (gsr_loss.h).  What the weights are for: people walking through a capture, the photographer's
 * shadow, sky, a turntable, the object masks that ship with many datasets.
 *
 * The function.  m is an (H, W) float32 image, m >= 0 and finite, and M = sum_p m_p.  S_c(p), alpha, beta, gamma, w, Wp and the
 * two windows are exactly those of gsr_loss.h: the window sums run over all pixels of the image, whatever their weight.  The weight
 * multiplies the loss map, not the images:
 *     l1_sum   = sum_p m_p sum_c |x - y|
 *     ssim_sum = sum_p m_p (1/3) sum_c S_c(p)
 *     L        = (1 - lambda) l1_sum / (3 M) + lambda (1 - ssim_sum / M)
 *     pixel_grad(q, c) = (1 - lambda) / (3 M) m_q sign(x - y)                                        [sign(0) = +1]
 *                      - lambda / (3 M) [ (w*(m alpha))(q) + 2 x_q (w*(m beta))(q) + y_q (w*(m gamma))(q) ]
 * When M = 0 both sums are 0 and pixel_grad is all zeros: no division by zero reaches an output.
 * Negative, NaN or infinite weights are the caller's error: nothing here looks for them, and the outputs are then undefined.
 *
 * What follows from it:
 *   - m = 1 everywhere gives the L and the gradient of gsr_l1_dssim_loss_grad (one more rounding of the scale factor);
 *   - k m for m changes neither L nor the gradient (for k a power of two not a bit of it; l1_sum and ssim_sum scale by k);
 *   - a pixel whose whole 11 x 11 neighbourhood has weight 0 gets a gradient of exactly 0;
 *   - a weight-0 pixel within 5 pixels of a weighted one still receives SSIM gradient, through that neighbour's window.
 * So a region is fully excluded only by a mask grown by the window radius, 5 pixels: with weights that are 0 on a region and
 * within 5 pixels of it, all outputs are bit for bit those of any other target content inside the region.
 *
 * weight_total is M as a single float IN DEVICE MEMORY, read by the kernels: a caller with a static mask computes it once per
 * view with gsr_weight_total and pays no extra launch per step.  The kernels form 1 / M themselves (0 when M = 0).
 *
 * Outputs (device memory, overwritten; nothing is accumulated across calls): the sums as above, single device floats (4-byte
 * aligned: any slot of a float array); pixel_grad (H, W, 3), or NULL for the sums alone.  Every sum is reduced per workgroup and
 * then in a fixed order, without float atomics, so two calls on the same inputs give the same bits in every output.  Nothing
 * in a call waits on the device.
 *
 * Arrays are packed float32 and 16-byte aligned: rendered, target, pixel_grad (H, W, 3); weight (H, W).  Each workspace is device
 * memory of at least the stated size, 16-byte aligned, its contents undefined on entry and on return; one workspace serves one
 * call at a time.  gsr_weighted_l1_loss_grad keeps one partial sum per workgroup, as gsr_weight_total does, and takes a workspace
 * of the same size, gsr_weight_total_workspace_bytes(W, H).
 *
 * Errors, checked in this order before anything is enqueued: GSR_E_NULL (any pointer but pixel_grad NULL), GSR_E_DIMS (W or
 * H <= 0, W * H > 2^28, scale negative or not finite, lambda_dssim outside [0, 1] or NaN, an unknown window), GSR_E_ALIGN (an
 * array or workspace pointer not 16-byte aligned, a single-float pointer not 4-byte aligned), GSR_E_WORKSPACE (workspace_bytes
 * below the stated size), then GSR_E_HIP (a launch failed).
 */
#ifndef GSR_WEIGHTED_LOSS_H
#define GSR_WEIGHTED_LOSS_H

#include "gsr_loss.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace gsr_weight_total and gsr_weighted_l1_loss_grad need for a W x H image (0 if W or H <= 0 or W * H > 2^28). */
size_t gsr_weight_total_workspace_bytes(int32_t W, int32_t H);

/* *total = M = the sum of weight (H, W). */
int gsr_weight_total(const float *weight, int32_t W, int32_t H, float *total /* device, overwritten */, void *workspace,
                     size_t workspace_bytes, void *stream);

/* The weighted twin of gsr_l1_loss_grad: *loss_sum = l1_sum above, pixel_grad = scale / (3 M) m sign(x - y). */
int gsr_weighted_l1_loss_grad(const float *rendered, const float *target, const float *weight, const float *weight_total /* device */,
                              float *pixel_grad /* may be NULL */, float *loss_sum /* device, overwritten */, int32_t W, int32_t H,
                              float scale, void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of workspace gsr_weighted_l1_dssim_loss_grad needs for a W x H image (0 if W or H <= 0 or W * H > 2^28). */
size_t gsr_weighted_dssim_workspace_bytes(int32_t W, int32_t H);

/* The weighted twin of gsr_l1_dssim_loss_grad.  For lambda_dssim = 0 pixel_grad is gsr_weighted_l1_loss_grad's with scale = 1,
 * bit for bit. */
int gsr_weighted_l1_dssim_loss_grad(const float *rendered, const float *target, const float *weight, const float *weight_total /* device */,
                                    float *pixel_grad /* may be NULL */, float *l1_sum, float *ssim_sum /* device, overwritten */, int32_t W,
                                    int32_t H, float lambda_dssim, int32_t window, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_WEIGHTED_LOSS_H */
