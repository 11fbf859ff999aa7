/*
 * gsr_loss.h -- the training loss of standard 3DGS in libgsr_hip.so: L = (1 - lambda) * L1 + lambda * (1 - SSIM), with its
 * pixel gradient.
 *
 * The reference's compute_image_gradients (loss.py:217-244) takes a lambda_dssim but leaves the SSIM gradient as a TODO
 * (loss.py:243), and its trainer keeps the SSIM term commented out (train.py:968-972); gsr_l1_loss_grad (gsr.h) reproduces
 * that surface.  This entry point completes it.
 *
 * The function.  For channel c at pixel p = (i, j) of a W x H image the window is the 11 x 11 window clipped to the image and
 * renormalised by its own weight sum, as the reference's ssim_kernel does (loss.py:76-100).  Tap q weighs w(|qx-i|) w(|qy-j|)
 * and Wp = Sx(i) Sy(j), Sx(i) = sum of w(|qx-i|) over the columns qx of the window inside the image (Sy likewise):
 *     m1 = sum w x / Wp,  m2 = sum w y / Wp,  e11 = sum w x^2 / Wp,  e22 = sum w y^2 / Wp,  e12 = sum w x y / Wp
 *     A = 2 m1 m2 + C1,  B = 2 (e12 - m1 m2) + C2,  C = m1^2 + m2^2 + C1,  D = (e11 - m1^2) + (e22 - m2^2) + C2
 *     S = A B / (C D),   SSIM = (1 / (3 H W)) sum_p sum_c S_c(p),   C1 = 0.01^2,  C2 = 0.03^2
 * x is the rendered image, y the target (a constant).  Two windows:
 *     GSR_SSIM_WINDOW_REFERENCE  w(d) = exp(-(d-5)^2 / 4.5): the weights gsr_ssim applies (quirk Q21: the rim weighs most).
 *                                With it, *ssim_sum equals gsr_ssim's sum up to float32 summation order.
 *     GSR_SSIM_WINDOW_GAUSSIAN   w(d) = exp(-d^2 / 4.5): the centred sigma = 1.5 window standard 3DGS trains with, under the
 *                                same border rule.  This is NOT the zero-padded convolution some codebases use: near the
 *                                border the window shrinks and is renormalised, it is not filled with zeros.
 *
 * The gradient.  With alpha = dS/dm1 / Wp, beta = dS/de11 / Wp, gamma = dS/de12 / Wp per channel and pixel,
 *     dS/dm1 = S (2 m2/A - 2 m2/B - 2 m1/C + 2 m1/D),   dS/de11 = -S / D,   dS/de12 = 2 S / B
 *     dSSIM/dx_q = (1 / (3 H W)) [ (w*alpha)(q) + 2 x_q (w*beta)(q) + y_q (w*gamma)(q) ]
 * where (w*a)(q) = sum over the pixels p inside the image of w(|px-qx|) w(|py-qy|) a(p): the same separable window applied
 * the other way.  Then
 *     pixel_grad = (1 - lambda) / (3 H W) * sign(x - y) - lambda * dSSIM/dx,    sign(0) = +1 as in gsr_l1_loss_grad.
 * For lambda = 0 pixel_grad is gsr_l1_loss_grad's with l1_weight = 1 / (3 H W), bit for bit.
 *
 * Outputs (device memory, overwritten; nothing is accumulated across calls):
 *     *l1_sum   = sum over pixels and channels of |x - y|                     mean L1 = l1_sum / (3 H W)
 *     *ssim_sum = sum over pixels of the channel mean of S (as gsr_ssim)     SSIM    = ssim_sum / (H W)
 *     pixel_grad (H, W, 3) as above, or NULL for the two sums alone.
 * The sums are reduced per workgroup and then in a fixed order, without atomics, so two calls on the same inputs give the same
 * bits in all three outputs.  Nothing in the call waits on the device.
 *
 * Arrays are packed (H, W, 3) float32 and 16-byte aligned, as in gsr.h; l1_sum and ssim_sum are single device floats (4-byte
 * aligned: any slot of a float array, such as a trainer's loss curve).
 * workspace: device memory of at least gsr_dssim_workspace_bytes(W, H) bytes, 16-byte aligned, its contents undefined on
 * entry and on return; one workspace serves one call at a time.
 *
 * Errors, all checked before anything is enqueued: GSR_E_NULL (rendered, target, l1_sum, ssim_sum or workspace NULL),
 * GSR_E_DIMS (W or H <= 0, W * H > 2^28, lambda_dssim outside [0, 1] or NaN, an unknown window), GSR_E_ALIGN (an array
 * or workspace pointer not 16-byte aligned, a sum pointer not 4-byte aligned), GSR_E_WORKSPACE (workspace_bytes <
 * gsr_dssim_workspace_bytes(W, H)), GSR_E_HIP (a launch failed).
 */
#ifndef GSR_LOSS_H
#define GSR_LOSS_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_SSIM_WINDOW_REFERENCE 0
#define GSR_SSIM_WINDOW_GAUSSIAN 1

/* Bytes of workspace gsr_l1_dssim_loss_grad needs for a W x H image (0 if W or H <= 0 or W * H > 2^28). */
size_t gsr_dssim_workspace_bytes(int32_t W, int32_t H);

int gsr_l1_dssim_loss_grad(const float *rendered, const float *target, float *pixel_grad /* may be NULL */, float *l1_sum,
                           float *ssim_sum /* device, overwritten */, int32_t W, int32_t H, float lambda_dssim, int32_t window,
                           void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_LOSS_H */
