/*
 * gsr_mesh_eval.h -- what judging an extracted mesh against a ground-truth surface needs in libgsr_hip.so: points sampled on a
 * triangle mesh by area, and the exact nearest neighbour of every point of one set in another set.  Accuracy, completeness (the two
 * halves of the Chamfer distance) and the F-score are sums over those distances (3dgs-native_amd/mesh_eval.py).  A stage of its own
 * behind training and extraction: no rasterizer kernel, struct or entry point changes.
 *
 * ---- gsr_nearest ----
 * The result is defined exactly.  For query q and reference j
 *     d2(q, j) = (dx * dx + dy * dy) + dz * dz,   dx = q.x - r_j.x, dy = q.y - r_j.y, dz = q.z - r_j.z,
 * every operation in float32, in that order, nothing contracted (gsr_knn.h's expression).  The candidates of q are the references
 * with d2(q, j) <= max_dist2 (max_dist2 = +inf: all of them), ordered by (d2, j): ties go to the lower reference index.  Then
 *     dist2[q] = d2 of the first candidate,  index[q] = its j;      without a candidate  dist2[q] = +inf, index[q] = -1.
 * The spatial structure inside (both sets in Morton order under their common bounding box, cut into blocks of
 * GSR_NEAREST_BLOCK_POINTS points, each with its box) only prunes: a block of references is skipped when the float32 lower bound of
 * its box, evaluated by the same expression, is strictly greater than the best distance so far, which starts at max_dist2.  Float32
 * subtraction, multiplication and the addition of non-negative terms are monotone, so the bound is never above the d2 of a point
 * in the box, and the strict test keeps the ties by index.  The output therefore does not depend on the order in which candidates
 * are met, on the workspace's earlier contents or on the stream: the same inputs give the same bits every call.
 *
 * Coordinates must be finite, and so must every d2: anything else is outside the contract (no fault, but unspecified values).
 *
 * ---- gsr_surface_sample_count / gsr_surface_sample_emit ----
 * Area-weighted random points on a triangle soup tri[T][3][3] (vertex a, b, c of each triangle, x y z of each vertex), in two
 * phases like the mesh extraction of gsr_tsdf.h: count, one host read of S = offsets[T] by the caller, emit.  Every step is one
 * rounded float32 operation in the stated order, nothing contracted, so the result is the same bits on every call.
 *
 * The random numbers are a counter-based hash, all in uint32 (wrapping):
 *     mix(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *     h(seed, t, k) = mix(mix(seed ^ t * 0x9E3779B9) ^ k * 0x85EBCA6B)
 *     u(seed, t, k) = (float)(h >> 8) * 2^-24                                 in [0, 1), exact
 * The count of triangle t:
 *     e1 = b - a,  e2 = c - a                                                   per component
 *     nx = e1.y * e2.z - e1.z * e2.y,  ny = e1.z * e2.x - e1.x * e2.z,  nz = e1.x * e2.y - e1.y * e2.x
 *     area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz)                          correctly rounded sqrt
 *     x = min(area * density, 2^20)   (GSR_SURFACE_SAMPLE_MAX_PER_TRIANGLE)
 *     count = (int)floor(x) + (u(seed, t, 0xFFFFFFFF) < x - floor(x) ? 1 : 0)   stochastic rounding: the expected count is x
 *     count = 0 when area is not finite (a NaN or infinite vertex, an overflow).
 * offsets[t] = count[0] + ... + count[t - 1], offsets[T] = S, int32.  The caller guarantees S < 2^31 (sum(area) * density + T bounds
 * it); beyond that the offsets wrap and emit writes unspecified points, inside its bounds.
 * Sample j = 0 .. count - 1 of triangle t is point offsets[t] + j (triangle order, then j):
 *     r1 = u(seed, t, 2 j),  r2 = u(seed, t, 2 j + 1);   if r1 + r2 > 1:  r1 = 1 - r1, r2 = 1 - r2
 *     p = (a + r1 * e1) + r2 * e2                                               per component
 *     points[offsets[t] + j] = p,  tri_index[offsets[t] + j] = t.
 * Emit writes only the samples whose global index is below S_capacity (and below S): a capacity that is too small loses the tail
 * and cannot fault.  `seed` and `tri` must be the ones of the count call.
 *
 * ---- both ----
 * All pointers are device pointers, 16-byte aligned.  The caller owns every byte: the library allocates nothing, enqueues everything
 * on `stream`, waits for nothing and reads nothing back.  A workspace's contents are undefined on entry and on return; one
 * workspace serves one call at a time.
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL       a required pointer is NULL (index and tri_index may be NULL).
 *     GSR_E_DIMS       gsr_nearest: M or N < 1 or > GSR_NEAREST_MAX_POINTS; max_dist2 negative or NaN (+inf is allowed).
 *                      sampling: T < 1 or T > GSR_SURFACE_SAMPLE_MAX_TRIANGLES; density not positive and finite;
 *                      S_capacity < 1 or > GSR_SURFACE_SAMPLE_MAX_SAMPLES.
 *     GSR_E_ALIGN      an array or the workspace is not 16-byte aligned.
 *     GSR_E_WORKSPACE  ws_bytes is below the stated size.
 *     GSR_E_HIP        a launch failed.
 */
#ifndef GSR_MESH_EVAL_H
#define GSR_MESH_EVAL_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_NEAREST_BLOCK_POINTS 256 /* points per search block: one workgroup's queries, and one staged block of references */
#define GSR_NEAREST_MAX_POINTS (1 << 27)
#define GSR_SURFACE_SAMPLE_MAX_TRIANGLES (1 << 27)
#define GSR_SURFACE_SAMPLE_MAX_SAMPLES (1 << 27)
#define GSR_SURFACE_SAMPLE_MAX_PER_TRIANGLE (1 << 20)

/* Bytes of workspace gsr_nearest needs for M queries and N references; 0 when either is < 1 or > GSR_NEAREST_MAX_POINTS.  With
 * A(x) = x rounded up to a multiple of 256, P(X) = 2 A(8 X) + A(16 X) + A(32 ceil(X / 256)) (a set's Morton items with their
 * ping-pong partner, its points in sorted order as (x, y, z, id), its blocks' boxes), L = max(M, N) and h = 256 ceil(L / 1024)
 * histogram entries of a radix pass:
 *     A(32 * 2049)                              the bounding box: 1024 partial records per set and the common box
 *   + P(M) + P(N)
 *   + 2 A(4 h) + A(4 (ceil(h / 1024) + 4))      a radix pass's histogram, its exclusive scan and the scan's scratch (shared) */
size_t gsr_nearest_workspace_bytes(int64_t M, int64_t N);

int gsr_nearest(int64_t M, const float *queries /* [M*3] */, int64_t N, const float *refs /* [N*3] */, float max_dist2,
                float *dist2 /* [M] */, int32_t *index /* [M] or NULL */, void *ws, size_t ws_bytes, void *stream);

/* Bytes of workspace gsr_surface_sample_count needs for T triangles; 0 for T < 1 or T > GSR_SURFACE_SAMPLE_MAX_TRIANGLES:
 *     A(4 (T + 1)) + A(4 (ceil((T + 1) / 1024) + 4))      the counts and the scan's scratch */
size_t gsr_surface_sample_workspace_bytes(int64_t T);

int gsr_surface_sample_count(int64_t T, const float *tri /* [T*9] */, float density, uint32_t seed,
                          int32_t *offsets /* [T+1], exclusive; offsets[T] = S */, void *ws, size_t ws_bytes, void *stream);

int gsr_surface_sample_emit(int64_t T, const float *tri /* [T*9] */, const int32_t *offsets /* [T+1] */, uint32_t seed, int64_t S_capacity,
                         float *points /* [S_capacity*3] */, int32_t *tri_index /* [S_capacity] or NULL */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_MESH_EVAL_H */
