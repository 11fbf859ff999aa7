/*
 * gsr_knn.h -- exact 3-nearest-neighbour distances of a point cloud in libgsr_hip.so: what a 3DGS trainer needs to start from SfM
 * points (or from random ones), each Gaussian's scale being the root of the mean squared distance to its three nearest neighbours.
 * A stage of its own in front of training: no rasterizer kernel, struct or entry point changes.
 *
 * The result is defined exactly.  For point i and every other index j != i
 *     d2(i, j) = (dx * dx + dy * dy) + dz * dz,   dx = x_i - x_j, dy = y_i - y_j, dz = z_i - z_j,
 * every operation in float32, in that order, nothing contracted.  A point at the position of i is a neighbour at distance 0.  The
 * candidates of i are ordered by (d2, j): ties go to the lower index.  With k = min(GSR_KNN_K, N - 1)
 *     nn_index[3 i .. 3 i + k)   the first k candidates in that order, the entries from k on are -1;
 *     mean_dist2[i]            = ((d2_0 + d2_1) + d2_2) / 3 in float32 (k = 2: (d2_0 + d2_1) / 2; k = 1: d2_0; N = 1: 0).
 * The spatial structure inside (a Morton order cut into blocks of GSR_KNN_BLOCK_POINTS points, each with its bounding box) only
 * prunes: a block is skipped when the float32 lower bound of its box, evaluated by the same expression, is strictly greater than
 * the third-best distance so far.  Float32 subtraction, multiplication and the addition of non-negative terms are monotone, so that
 * bound is never above the d2 of a point in the box, and the strict test keeps the ties by index.  The output therefore does not
 * depend on the order in which candidates are met, on the workspace's earlier contents or on the stream: the same points give the
 * same bits every call.
 *
 * Coordinates must be finite, and so must every d2: anything else is outside the contract (no fault, but unspecified values).
 *
 * All pointers are device pointers, 16-byte aligned.  The caller owns every byte: the library allocates nothing, enqueues everything
 * on `stream`, waits for nothing and reads nothing back -- the bounding box is reduced and consumed on the device, so a call may sit
 * in a stream behind the kernels that write `points`.  workspace: at least gsr_knn_workspace_bytes(N) bytes, contents undefined on
 * entry and on return; one workspace serves one call at a time.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL       points, mean_dist2 or ws is NULL (nn_index may be NULL: distances only).
 *     GSR_E_DIMS       N < 1 or N > GSR_KNN_MAX_POINTS.
 *     GSR_E_ALIGN      an array or the workspace is not 16-byte aligned.
 *     GSR_E_WORKSPACE  ws_bytes < gsr_knn_workspace_bytes(N).
 *     GSR_E_HIP        a launch failed.
 */
#ifndef GSR_KNN_H
#define GSR_KNN_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_KNN_K 3
#define GSR_KNN_BLOCK_POINTS 256 /* points per search block: one workgroup's queries, and one staged block of candidates */
#define GSR_KNN_MAX_POINTS (1 << 27)

/* Bytes of workspace gsr_knn needs for N points; 0 for N < 1 or N > GSR_KNN_MAX_POINTS.  With A(x) = x rounded up to a multiple of
 * 256, nb = ceil(N / 256) search blocks, sb = ceil(N / 1024) sort chunks and h = 256 sb histogram entries:
 *     A(32 * 1025)                     the bounding box: 1024 partial records and the box itself
 *   + 2 A(8 N)                         the (Morton code << 32 | id) items and their ping-pong partner
 *   + 2 A(4 h) + A(4 (ceil(h / 1024) + 4))   a radix pass's histogram, its exclusive scan and the scan's scratch
 *   + A(16 N)                          the points in sorted order as (x, y, z, id)
 *   + A(32 nb)                         the blocks' bounding boxes */
size_t gsr_knn_workspace_bytes(int64_t N);

int gsr_knn(int64_t N, const float *points /* [N*3] */, float *mean_dist2 /* [N] */, int32_t *nn_index /* [N*3] or NULL */, void *ws,
            size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_KNN_H */
