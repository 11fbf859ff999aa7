/*
 * gsr_distortion.h -- the depth-distortion regulariser over the lists of a rendered frame, and its gradient, in libgsr_hip.so: the
 * term 2DGS, GOF, PGSR and RaDe-GS train with before they extract a mesh.  It pulls the Gaussians a ray crosses onto one surface.
 * A stage of its own behind the forward and between the two halves of the backward: no rasterizer kernel, struct or entry point
 * changes, and nothing is binned or sorted again.
 *
 * Definition.  For pixel p the applied entries k = 0 ... of its tile's list and their weights w_k = alpha_k T_k are exactly those of
 * gsr_features.h: the same float32 power expression, alpha = min(0.99, o exp(power)) with the forward's exp, the two skip tests
 * (power > 0, alpha < 1/255), T <- T (1 - alpha) from T = 1, and the walk up to n_contrib[p].  m_k is the INVERSE view depth of
 * Gaussian i_k, inv_depth[i_k * inv_depth_stride]: column 9 of the blend records (stride 16) or a packed array of 1 / depths.
 * Inverse depth rather than 2DGS's near/far mapping: it is bounded, it needs no parameters, and it is what the forward's depth
 * image already blends.
 *
 *     Dist(p) = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2  =  A S,      A = sum w,  mu = sum w m / A,  S = sum w (m - mu)^2
 *
 * the squared, ordered-pair form of 2DGS's rasterizer.
 *
 * Forward, per pixel, float32, every product left to right, nothing contracted; A = mu = S = 0 and T = 1 before the first entry,
 * and per applied entry, in list order:
 *
 *     w  = alpha * T          T <- T * (1 - alpha)
 *     A' = A + w
 *     d  = m - mu
 *     r  = w / A'             (IEEE division)
 *     S  <- S + ((A * r) * d) * d        (A: the value BEFORE this entry)
 *     mu <- mu + r * d
 *     A  <- A'
 *
 * then dist[p] = A * S and moments[p] = (A, mu, S, 0).  A running weighted mean and central moment, not A M2 - M1^2: with depths
 * within a relative 1 / kappa of each other the running form errs by a few eps32 kappa of the value, the moment form by kappa times
 * more.  moments[p][0] is bit for bit gsr_features_forward of a column of ones.  Pixels without an applied entry, pixels of a tile
 * without a list and every pixel of a frame with D = 0 are (0, 0, 0, 0), dist 0.  No atomics: the same frame gives the same bits
 * every call, on every stream, with or without block_masks.
 *
 * Backward.  g = dL_ddist[p]; A, mu, S are read from `moments` (the forward's, not recomputed).  With
 *
 *     dL/dw_k = g (A (m_k - mu)^2 + S),   dL/dm_k += 2 g w_k A (m_k - mu),   sum_k w_k dL/dw_k = 2 g A S
 *     dL/dalpha_k = T_k dL/dw_k - (sum_{j>k} w_j dL/dw_j) / (1 - alpha_k)
 *
 * the walk is again front to back, and the suffix sum is formed as the stored total minus the running prefix.  Per pixel, once:
 *
 *     gA = g * A          total = 2 * (gA * S)          P = 0, T = 1
 *
 * and per applied entry, in list order (G = exp(power), o = opacity, dx = x_k - p.x, dy = y_k - p.y as in the forward):
 *
 *     w  = alpha * T
 *     d  = m - mu
 *     u  = (((A * d) * d) + S) * g
 *     P  <- P + w * u
 *     R  = total - P                      (the entries behind k)
 *     q  = T * u - R / (1 - alpha)        (IEEE division; dL/dalpha: the gradient passes the 0.99 cap)
 *     gd = G * q                          (the opacity term)
 *     h  = o * gd        hx = h * dx      hy = h * dy
 *     seven per-(pixel, entry) values:  hx, hy, hx * dx, hx * dy, hy * dy, gd, ((2 * gA) * w) * d
 *     T  <- T * (1 - alpha)
 *
 * The total-minus-prefix form keeps one pass; its price is that R carries the rounding of the total, eps32 |2 g A S|, which a
 * back-to-front walk would not have at the last entries of a long list.
 *
 * An 8x8 pixel block sums each of the seven values over its pixels in a fixed order -- pixels 0-31 in order (pixel q of a block is
 * (q & 7, q >> 3)), pixels 32-63 in order, then the two halves -- to S1, S2, Sxx, Sxy, Syy, Sop, Sdm, and ADDS to the accumulator
 * row of Gaussian i_k (the backward's 16-float records at gsr_backward_accumulators_offset; a', b', c' = -a/2, -b, -c/2 the
 * pre-scaled conic):
 *
 *     column 3   (2 a' S1 + b' S2) * (0.5 W)        = -(a S1 + b S2) 0.5 W       dL_dmean2D x
 *     column 4   (2 c' S2 + b' S1) * (0.5 H)                                      dL_dmean2D y
 *     column 6   -0.5 Sxx     column 7   -0.5 Sxy  (b as stored: half)     column 9   -0.5 Syy      dL_dconic
 *     column 10  Sop                                                              dL_dopacity (G dL/dalpha)
 *     column 11  Sdm                                                              dL/d(1/depth)
 *
 * and touches no other column: 0-2 (colour), 5, 8, 12-13 (the absolute gradients stay the colour, depth and alpha terms' alone) and
 * 14-15 are what the blend half left.  One float atomic per (block, applied entry, column): the last bits of a row that several
 * blocks or tiles touch may differ from run to run.  The per-Gaussian half of the backward (gsr_backward_geom_aa, the AUX kernel)
 * then carries the seven columns on to the parameters, and gsr_backward_camera_aa to the camera.
 *
 * dL_ddist and inv_depth must be finite: anything else is outside the contract (no fault, but unspecified values).
 *
 * Every walk is bounded as in gsr_features.h: a tile's range is clipped to [0, D], a pixel visits min(n_contrib[p], range length)
 * entries, and an id outside [0, N) is skipped.  Stale or foreign buffers of the stated sizes give wrong numbers, never an access
 * out of bounds.  block_masks (optional, NULL is allowed) only let a wave pass over entries that cannot reach its block.
 *
 * All pointers are device pointers.  dist, moments, dL_ddist and accumulators are 16-byte aligned; the arrays of the frame are
 * 4-byte aligned (xy, conic_opacity and inv_depth may be columns of a wider record: their row strides are given in floats).  The
 * caller owns every byte: the library allocates nothing, enqueues everything on `stream`, waits for nothing and reads nothing back.
 * No workspace is needed.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL   frame, xy, conic_opacity, inv_depth, ranges, n_contrib or an array argument is NULL; point_list is NULL while D > 0.
 *     GSR_E_DIMS   W or H < 1 or > GSR_FEATURES_MAX_SIDE, N < 1 or > 2^31 - 1, D < 0 or > 2^30, xy_stride < 2, conic_opacity_stride < 4,
 *                  inv_depth_stride < 1.
 *     GSR_E_ALIGN  an array is not aligned as stated above.
 *     GSR_E_HIP    a launch failed.
 */
#ifndef GSR_DISTORTION_H
#define GSR_DISTORTION_H

#include "gsr.h"
#include "gsr_features.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct GsrDistortionFrame {
    int32_t W, H;                /* image size; tiles are 16 x 16, row-major, ceil(W / 16) per row */
    int64_t N;                   /* Gaussians of the frame */
    int64_t D;                   /* entries of point_list (capacity mode: the capacity) */
    const float *xy;             /* pixel position of Gaussian i at xy[i * xy_stride + {0, 1}] */
    int64_t xy_stride;           /* in floats: 2 packed, 16 for the column view of the blend records */
    const float *conic_opacity;  /* conic a, b, c and opacity of Gaussian i at conic_opacity[i * conic_opacity_stride + {0 .. 3}] */
    int64_t conic_opacity_stride; /* in floats: 4 packed, 16 for the record view */
    const int32_t *point_list;   /* [D] Gaussian ids, tile by tile, front to back */
    const int32_t *ranges;       /* [tiles][2]: start and end of each tile's list */
    const int32_t *n_contrib;    /* [H][W]: 1-based list position of each pixel's last contributor */
    const uint8_t *block_masks;  /* [D] or NULL: the forward blend's per-entry block hit masks */
    const float *inv_depth;      /* 1 / view depth of Gaussian i at inv_depth[i * inv_depth_stride] */
    int64_t inv_depth_stride;    /* in floats: 1 packed, 16 for column 9 of the blend records */
} GsrDistortionFrame;

/* dist[H][W] = A S and moments[H][W][4] = (A, mu, S, 0).  Every element of both is written. */
int gsr_distortion_forward(const GsrDistortionFrame *frame, float *dist /* [H][W] */, float *moments /* [H][W][4] */, void *stream);

/* Adds the gradient of sum_p dL_ddist[p] Dist(p) into columns 3, 4, 6, 7, 9, 10 and 11 of accumulators[N][16]. */
int gsr_distortion_backward(const GsrDistortionFrame *frame, const float *dL_ddist /* [H][W] */, const float *moments /* [H][W][4] */,
                            float *accumulators /* [N][16] */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_DISTORTION_H */
