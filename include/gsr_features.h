/*
 * gsr_features.h -- N-channel feature rendering over the lists of a rendered frame, with its gradient, in libgsr_hip.so: any
 * per-Gaussian quantity (a normal, a segmentation logit, a distilled 2D feature, a statistic, an id as a palette colour) blended
 * into an image with the weights of a frame the rasterizer has already drawn, and the transposed sum that carries an image-space
 * gradient back onto the per-Gaussian rows.  A stage of its own behind the forward: no rasterizer kernel, struct or entry point
 * changes, and nothing is binned or sorted again.
 *
 * Inputs:
 *
 * - A frame: the buffers of one forward call, of any rasterize mode, with or without the 3D filter.  Capacity mode is allowed once
 *   the caller has checked the rendered count, as for the backward (D is then the capacity).
 * - A feature array F: float32 [N][C], row-major, 1 <= C <= GSR_FEATURES_MAX_CHANNELS (64).
 *
 * For pixel p = (x, y) in tile t, visit entries k = 0 ... n_contrib[p] - 1 of the tile's list, i_k = point_list[ranges[t].start + k],
 * in list order:
 *
 * - d = xy[i_k] - p.
 * - power is the float32 expression of blend_fwd.hip:307: pre-scaled conic (a' = -a/2, b' = -b, c' = -c/2),
 *   (a' dx dx + c' dy dy) + b' dx dy, every product left to right, nothing contracted.
 * - alpha = min(0.99, o * exp(power)), with the forward's exp (v_exp_f32 of power * log2 e).
 * - The entry is skipped when power > 0 or alpha < 1/255.
 * - Otherwise w = alpha * T, then T <- T * (1 - alpha), with T starting at 1.
 *
 * Outputs:
 *
 * - out[p][c] = sum over k of w_k F[i_k][c], summed front to back: one float32 fused multiply-add per term, in list order.
 * - Nothing past n_contrib[p] is visited.  The saturation decision is the forward's and is not taken again.
 * - No background is added.  final_T is in the caller's hands.
 * - Pixels of a tile without a list are 0 (quirk Q10's behaviour); so is every pixel of a frame with D = 0.
 * - Backward: dL_dF[i][c] = sum over p of w_i(p) G[p][c], where G is dL_dout, [H][W][C].  The array is written by the call, not
 *   added to.  Rows of Gaussians that no pixel used are exactly 0.
 * - The gradient is with respect to the features only.  Geometry is a constant of the call.
 *
 * Reproducibility.  The forward uses no atomics: the same frame and F give the same bits every call, on every stream, with or
 * without block_masks.  The backward sums the 64 pixels of an 8x8 block in a fixed order on chip and adds each block's row to
 * dL_dF with float atomics: the last bits of a row that several blocks or tiles touch may differ from run to run.
 *
 * F and G must be finite: anything else is outside the contract (no fault, but unspecified values).
 *
 * Every walk is bounded: a tile's range is clipped to [0, D], a pixel visits min(n_contrib[p], range length) entries, and an id
 * outside [0, N) is skipped.  Stale or foreign buffers of the stated sizes give wrong numbers, never an access out of bounds.
 *
 * block_masks (optional, NULL is allowed): the forward blend's per-entry 8x4-block hit masks (GsrBinning.block_masks), D bytes.
 * They only let a wave pass over entries that cannot reach alpha >= 1/255 inside its block: they are conservative and defined up to
 * each tile's saturation point, which the walk never passes, so no output depends on them.
 *
 * All pointers are device pointers.  features, out, dL_dout and dL_dF are 16-byte aligned; the arrays of the frame are 4-byte
 * aligned (xy and conic_opacity may be columns of a wider record: their row strides are given in floats).  The caller owns every
 * byte: the library allocates nothing, enqueues everything on `stream`, waits for nothing and reads nothing back.  No workspace is
 * needed, so there is no gsr_features_workspace_bytes and no GSR_E_WORKSPACE.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL   frame, xy, conic_opacity, ranges, n_contrib or an array argument is NULL; point_list is NULL while D > 0.
 *     GSR_E_DIMS   W or H < 1 or > GSR_FEATURES_MAX_SIDE, N < 1 or > 2^31 - 1, D < 0 or > 2^30, xy_stride < 2, conic_opacity_stride < 4,
 *                  C < 1 or C > GSR_FEATURES_MAX_CHANNELS.
 *     GSR_E_ALIGN  an array is not aligned as stated above.
 *     GSR_E_HIP    a launch failed.
 */
#ifndef GSR_FEATURES_H
#define GSR_FEATURES_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_FEATURES_MAX_CHANNELS 64
#define GSR_FEATURES_MAX_SIDE 32768

typedef struct GsrFeaturesFrame {
    int32_t W, H;                /* image size; tiles are 16 x 16, row-major, ceil(W / 16) per row */
    int64_t N;                   /* Gaussians of the frame */
    int64_t D;                   /* entries of point_list (capacity mode: the capacity) */
    const float *xy;             /* pixel position of Gaussian i at xy[i * xy_stride + {0, 1}] */
    int64_t xy_stride;           /* in floats: 2 for a packed [N][2] array, 16 for the column view of the blend records */
    const float *conic_opacity;  /* conic a, b, c and opacity of Gaussian i at conic_opacity[i * conic_opacity_stride + {0 .. 3}] */
    int64_t conic_opacity_stride; /* in floats: 4 packed, 16 for the record view */
    const int32_t *point_list;   /* [D] Gaussian ids, tile by tile, front to back */
    const int32_t *ranges;       /* [tiles][2]: start and end of each tile's list */
    const int32_t *n_contrib;    /* [H][W]: 1-based list position of each pixel's last contributor */
    const uint8_t *block_masks;  /* [D] or NULL: see above */
} GsrFeaturesFrame;

/* out[H][W][C] = the blend of features[N][C] under the frame's weights.  Every element of out is written. */
int gsr_features_forward(const GsrFeaturesFrame *frame, int32_t C, const float *features /* [N][C] */, float *out /* [H][W][C] */,
                         void *stream);

/* dL_dF[N][C] = the transposed sum of dL_dout[H][W][C].  Every element of dL_dF is written. */
int gsr_features_backward(const GsrFeaturesFrame *frame, int32_t C, const float *dL_dout /* [H][W][C] */, float *dL_dF /* [N][C] */,
                          void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_FEATURES_H */
