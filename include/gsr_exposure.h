/*
 * gsr_exposure.h -- per-view exposure compensation in libgsr_hip.so: a learned affine colour transform per training image, applied
 * to the render before the loss (the "exposure" of hierarchical 3DGS, now in the standard 3DGS trainer), its backward, and the
 * Adam step of its 12 numbers.  An image-space stage beside gsr_loss.h: no rasterizer kernel, struct or entry point changes.
 *
 * The function.  E is 12 float32, row-major (4, 3): rows 0-2 are A, row 3 is b (E[3 i + j] = A[i][j], E[9 + j] = b_j).  For a
 * pixel with colour row vector c = (c_0, c_1, c_2):
 *     c'_j = ((c_0 A[0][j] + c_1 A[1][j]) + c_2 A[2][j]) + b_j          c' = c A + b;  identity: A = I, b = 0
 * which is 3DGS's matmul(image.permute(1, 2, 0), exposure[:3, :3]) + exposure[:3, 3].  There is no clamp.  The sum is evaluated in
 * float32 in exactly the order written (i = 0, 1, 2, then + b_j), no fused multiply-add.  With E = identity the output is the
 * input bit for bit for every finite input except -0, which comes back as +0 (x * 1 + 0 + 0 + 0; a non-finite channel makes
 * its pixel's other channels NaN, inf * 0).
 *
 * The backward.  Given g = dL/dc' of shape (H, W, 3):
 *     dL/dc_i     = (A[i][0] g_0 + A[i][1] g_1) + A[i][2] g_2
 *     dL/dA[i][j] = sum over pixels of c_i g_j
 *     dL/db_j     = sum over pixels of g_j
 * dL_dE has the layout of E.  The 12 sums: a thread sums its pixels in ascending order (4 consecutive pixels per round, rounds
 * GSR_EXPOSURE_MAX_BLOCKS * GSR_EXPOSURE_BLOCK_PIXELS pixels apart), a wave adds its 64 lanes in a butterfly, a workgroup its
 * 4 waves, and leaves one partial record in the workspace; a second launch of one workgroup adds the records -- each thread
 * every 256th in ascending order, then the same butterfly.  No float atomics: two calls on the same inputs give the same bits
 * in dL_drendered and dL_dE.
 *
 * The Adam step (gsr_exposure_adam), on each of the 12 elements, in float32:
 *     m = beta1 m + (1 - beta1) g,   v = beta2 v + (1 - beta2) (g g)
 *     E = E - lr * ((m / (1 - beta1^step)) / (sqrt(v / (1 - beta2^step)) + eps))
 * step >= 1 is the number of this step (the first is 1); the two bias corrections are formed on the host in float32.  Nothing in
 * any of these calls waits on the device.
 *
 * Outputs (device memory, overwritten; nothing is accumulated across calls):
 *     out           (H, W, 3) the corrected image; may be `rendered` itself (in place).
 *     dL_drendered  (H, W, 3), or NULL for dL_dE alone; may be `dL_dout` itself (in place).  It must not overlap an input otherwise.
 *     dL_dE         12 floats.
 *     E, m, v       12 floats each, updated in place by gsr_exposure_adam.
 *
 * Images are packed (H, W, 3) float32 and 16-byte aligned, as in gsr.h.  The 12-float arrays (E, dL_dE, m, v) are 4-byte
 * aligned: a row of a (V, 12) tensor qualifies.  workspace: device memory of at least gsr_exposure_workspace_bytes(W, H) bytes,
 * 16-byte aligned, its contents undefined on entry and on return; one workspace serves one call at a time.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL       a required pointer is NULL (every pointer except dL_drendered).
 *     GSR_E_DIMS       W or H <= 0, W * H > 2^28; gsr_exposure_adam: step < 1, lr negative or not finite, beta1 or beta2 outside
 *                      [0, 1) or NaN, eps not positive or not finite.
 *     GSR_E_ALIGN      an image or the workspace not 16-byte aligned, a 12-float array not 4-byte aligned.
 *     GSR_E_WORKSPACE  workspace_bytes < gsr_exposure_workspace_bytes(W, H).
 *     GSR_E_HIP        a launch failed.
 */
#ifndef GSR_EXPOSURE_H
#define GSR_EXPOSURE_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_EXPOSURE_FLOATS 12          /* E, dL_dE, m, v */
#define GSR_EXPOSURE_BLOCK_PIXELS 1024  /* pixels a workgroup of the image kernels takes per round: 256 threads x 4 pixels */
#define GSR_EXPOSURE_MAX_BLOCKS 1024    /* workgroups of the backward at most (= partial records); larger images take several rounds */
#define GSR_EXPOSURE_RECORD_BYTES 64    /* one partial record: 12 sums, 4 floats of padding */

/* Bytes of workspace gsr_exposure_backward needs for a W x H image (0 if W or H <= 0 or W * H > 2^28). */
size_t gsr_exposure_workspace_bytes(int32_t W, int32_t H);

int gsr_exposure_apply(const float *rendered, const float *E /* device[12] */, float *out /* may equal rendered */, int32_t W, int32_t H,
                       void *stream);

int gsr_exposure_backward(const float *rendered, const float *E /* device[12] */, const float *dL_dout,
                          float *dL_drendered /* may equal dL_dout; may be NULL */, float *dL_dE /* device[12], overwritten */, int32_t W,
                          int32_t H, void *workspace, size_t workspace_bytes, void *stream);

int gsr_exposure_adam(float *E, const float *dL_dE, float *m, float *v /* device[12] each */, float lr, float beta1, float beta2, float eps,
                      int32_t step /* >= 1 */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_EXPOSURE_H */
