/*
 * gsr_tsdf.h -- TSDF fusion of rendered depth (and colour) into a dense volume, and triangle-mesh extraction from it by marching
 * tetrahedra, in libgsr_hip.so.  A stage of its own behind the forward: it reads depth images (tsdf.depth_from_buffers gives them from
 * the forward's inverse depth and final_T) and changes no rasterizer kernel, struct or entry point.
 *
 * All pointers are device pointers unless marked host.  The library allocates nothing, enqueues everything on `stream`, waits for
 * nothing and reads nothing back.  No kernel uses atomics: the same bits every call, on any stream, whatever the outputs and the
 * workspace held before.  Every step below is one float32 operation, rounded once, in the order written (no fused multiply-add;
 * divisions are correctly rounded).
 *
 * The volume (GsrTsdfVolume).  Gx x Gy x Gz voxels, 1 <= G <= GSR_TSDF_MAX_DIM per axis, Gx Gy Gz <= GSR_TSDF_MAX_VOXELS.  origin =
 * o, the world position of the CENTRE of voxel (0, 0, 0); voxel_size = s > 0.  tsdf[Gz][Gy][Gx] and weight[Gz][Gy][Gx] float32,
 * color[Gz][Gy][Gx][3] float32 or NULL.  The linear index of voxel (x, y, z) is (z Gy + y) Gx + x.  gsr_tsdf_reset writes tsdf = 1,
 * weight = 0, color = 0.  A volume must be reset before it is first integrated.
 *
 * Integration (gsr_tsdf_integrate).  `views`: a HOST array of V >= 1 GsrTsdfView records: depth z[H][W] (view depth along the camera's
 * +z; 0 means "no measurement"), color [H][W][3] or NULL, `view` = world_to_camera as 16 floats in row-vector form (p = [X, 1] . V,
 * V_rc = view[4 r + c], the translation in row 3 -- gsr.h's GsrCamera.view), tan_fovx, tan_fovy, W, H and the observation weight
 * w_obs > 0.  Every voxel takes the views in the order given.  For the voxel (ix, iy, iz):
 *     X_c  = o_c + s * (float)i_c                                                     (c = x, y, z)
 *     p_x  = ((X_x V00 + X_y V10) + X_z V20) + V30,  p_y with V01 V11 V21 V31,  p_z with V02 V12 V22 V32
 *     skip the view unless p_z > 0 and p_z is finite
 *     u    = ((p_x / (p_z * tan_fovx) + 1) * (float)W - 1) * 0.5                      v likewise with p_y, tan_fovy, H
 *            (the forward's pixel convention; gsr_normals.h states its inverse)
 *     fu   = floorf(u + 0.5f); skip unless 0 <= fu and fu < (float)W, compared in float (a NaN fails); x = (int)fu.  fv, y likewise.
 *     d    = z[y][x]; skip unless d is finite, d > 0 and d <= depth_max
 *     sdf  = d - p_z; skip if sdf < -trunc;  t = fminf(1, sdf / trunc)
 *     w0   = weight,  w1 = w0 + w_obs,  tsdf = (tsdf * w0 + t * w_obs) / w1
 *     if the view and the volume both have colour, per channel: color = (color * w0 + c[y][x] * w_obs) / w1
 *     weight = fminf(w1, w_max)
 * The views reach the kernel BY VALUE, in launches of at most GSR_TSDF_VIEWS_PER_LAUNCH views (the kernel-argument area bounds it);
 * nothing is staged through device memory.  A thread keeps its voxel's state in registers over the views of a launch: the volume is
 * read and written once per launch, not once per view.  The update is sequential float32 in view order, so the result is the same
 * bits however a sequence of views is split into calls.  The kernel prunes nothing by block: every voxel runs the steps above.
 *
 * gsr_tsdf_depth gives the depth image the integrator reads from the forward's two images: Dinv = GsrImage.inv_depth, T =
 * GsrImage.final_T (W x H float32).  A = 1 - T; the pixel is DEFINED iff A and Dinv are finite, A >= alpha_min and Dinv > 0 -- exactly
 * gsr_normals.h's rule -- and then z = A / Dinv; every other pixel gets 0, "no measurement".
 *
 * Extraction by marching tetrahedra (gsr_mesh_count, gsr_mesh_emit).  No case table beyond what is stated here.
 *   Cells.   Cell (ix, iy, iz), 0 <= i_c < G_c - 1, linear index (iz (Gy - 1) + iy) (Gx - 1) + ix, has the corners
 *            (ix + dx, iy + dy, iz + dz), corner code k = dx + 2 dy + 4 dz.  It is ACTIVE iff all eight corners have weight >=
 *            min_weight (min_weight > 0).  A corner is INSIDE iff tsdf < 0: the iso-value is 0 and a corner at exactly 0 is outside.
 *   Tetrahedra.  An active cell is cut into the six Kuhn tetrahedra: for the permutations (a, b, c) of the axes (0, 1, 2) in
 *            lexicographic order -- 012, 021, 102, 120, 201, 210, tetrahedron 0 to 5 -- the corners with the codes
 *                c0 = 0,  c1 = 1 << a,  c2 = c1 | (1 << b),  c3 = 7.
 *            sigma = the sign of the permutation: + - - + + -.
 *   Edges and vertices.  The edge between tetrahedron corners m < n runs from the grid point P (code c_m) to Q (code c_n), along the
 *            direction with the bits c_n ^ c_m: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) are directions 0 to 6.  A
 *            crossed edge (one end inside, one outside) gives, with a = tsdf(P), b = tsdf(Q):
 *                t     = a / (a - b)
 *                x_c   = (o_c + s * (float)P_c) + t * (s * (float)dir_c)
 *                col_c = (1 - t) * col(P)_c + t * col(Q)_c                 ((1 - t) * col(P) first, then t * col(Q), then the sum)
 *                key   = (int64)(linear voxel index of P) * 7 + direction
 *            always from P to Q, so every tetrahedron and cell that shares the edge produces the same bits and the same key.
 *   Triangles.  With the inside corners of the tetrahedron as a set:
 *            one corner L on one side, three on the other: with (j, k, l) = (1,2,3) (0,3,2) (3,0,1) (2,1,0) for L = 0 1 2 3, the
 *                triangle (e_Lj, e_Lk, e_Ll); its last two vertices are exchanged iff (sigma < 0) != (L is outside).
 *            two and two: inside {i < j}, outside {k < l}: the quad (e_ik, e_il, e_jl, e_jk); it is taken in the reverse cyclic
 *                order (e_ik, e_jk, e_jl, e_il) iff (sigma < 0) != ({i, j} is {0, 2} or {1, 3}).  The cyclic order is rotated to start
 *                at the vertex with the smallest key, q0 q1 q2 q3, and split into (q0, q1, q2) and (q0, q2, q3).
 *            Every triangle is thereby wound so that (v1 - v0) x (v2 - v0) points towards positive tsdf, which is free space.
 *   Degenerate triangles.  A corner whose tsdf is exactly 0 is outside and puts the vertices of all its crossed edges on itself:
 *            zero-area triangles occur then, and are emitted like any other triangle (welding by key keeps the mesh closed).
 *   Output order.  Triangles come out by ascending linear cell index, then by tetrahedron, then by triangle: the same arrays every call.
 *
 * gsr_mesh_count walks the cells in workgroups of GSR_MESH_GROUP_CELLS consecutive cells, leaves each workgroup's exclusive triangle
 * offset in the workspace and the total in *total (a device int64).  gsr_mesh_emit, on the volume, min_weight and workspace of a
 * count, writes vertices[T][3][3], colors[T][3][3] (or NULL; zeros for a volume without colour) and keys[T][3] (int64) for the
 * triangles below the caller's capacity T_cap, and nothing at or past T_cap.  workspace: device memory of at least
 * gsr_mesh_workspace_bytes(Gx, Gy, Gz) bytes, 16-byte aligned, undefined on entry to the count:
 *     groups = max(1, ceil((Gx - 1)(Gy - 1)(Gz - 1) / GSR_MESH_GROUP_CELLS))
 *     bytes  = align256(4 * groups) + align256(8 * ceil(groups / GSR_MESH_SCAN_GROUPS))
 *
 * Errors, all checked before anything is enqueued, in this order:
 *     GSR_E_NULL       volume, tsdf, weight, views, a view's depth, workspace, total, vertices, keys, Dinv, final_T or z_out is NULL.
 *     GSR_E_DIMS       a G outside 1 .. GSR_TSDF_MAX_DIM, Gx Gy Gz > GSR_TSDF_MAX_VOXELS, origin not finite, voxel_size not finite or
 *                      <= 0; V < 1, a view's W or H <= 0 or > GSR_TSDF_MAX_SIDE or W H > 2^28, a tangent or w_obs not finite or <= 0, a matrix entry not
 *                      finite; trunc not finite or <= 0; depth_max, w_max or min_weight NaN or <= 0 (+Inf is allowed); T_cap < 0;
 *                      alpha_min not finite.
 *     GSR_E_ALIGN      an array, an image or the workspace not 16-byte aligned, total not 8-byte aligned.
 *     GSR_E_WORKSPACE  workspace_bytes < gsr_mesh_workspace_bytes(Gx, Gy, Gz).
 *     GSR_E_HIP        a launch failed.
 */
#ifndef GSR_TSDF_H
#define GSR_TSDF_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_TSDF_MAX_DIM 2048            /* voxels per axis at most */
#define GSR_TSDF_MAX_VOXELS 2147483648   /* Gx Gy Gz at most: 2^31 */
#define GSR_TSDF_MAX_SIDE 16777216        /* W and H of a view at most: 2^24, so that (float)W and (float)H are exact */
#define GSR_TSDF_VIEWS_PER_LAUNCH 16     /* views one launch takes by value: 16 records of 104 bytes in the kernel-argument area */
#define GSR_MESH_GROUP_CELLS 256         /* consecutive cells per workgroup of the count and the emit: one offset each */
#define GSR_MESH_SCAN_GROUPS 1024        /* workgroup counts one scan workgroup takes */
#define GSR_MESH_DIRECTIONS 7            /* key = linear index of P * 7 + direction */

typedef struct GsrTsdfVolume {
    int32_t Gx, Gy, Gz;
    float voxel_size;
    float origin[3];     /* world position of the centre of voxel (0, 0, 0) */
    int32_t pad;
    float *tsdf;         /* [Gz][Gy][Gx] */
    float *weight;       /* [Gz][Gy][Gx] */
    float *color;        /* [Gz][Gy][Gx][3], or NULL */
} GsrTsdfVolume;

typedef struct GsrTsdfView {
    const float *depth;  /* [H][W] view depth; 0 = no measurement */
    const float *color;  /* [H][W][3], or NULL */
    float view[16];      /* world_to_camera, row-vector form, translation in row 3 */
    float tan_fovx, tan_fovy;
    int32_t W, H;
    float w_obs;         /* > 0 */
    int32_t pad;
} GsrTsdfView;           /* 104 bytes */

/* Bytes of workspace gsr_mesh_count and gsr_mesh_emit need (0 if the dimensions are refused). */
size_t gsr_mesh_workspace_bytes(int32_t Gx, int32_t Gy, int32_t Gz);

int gsr_tsdf_reset(const GsrTsdfVolume *volume /* host */, void *stream);

int gsr_tsdf_integrate(const GsrTsdfVolume *volume /* host */, int32_t V, const GsrTsdfView *views /* host[V] */, float trunc, float depth_max,
                       float w_max, void *stream);

int gsr_tsdf_depth(const float *Dinv, const float *final_T, int32_t W, int32_t H, float alpha_min, float *z_out /* [H][W] */, void *stream);

int gsr_mesh_count(const GsrTsdfVolume *volume /* host */, float min_weight, void *workspace, size_t workspace_bytes,
                   int64_t *total /* device, overwritten */, void *stream);

int gsr_mesh_emit(const GsrTsdfVolume *volume /* host */, float min_weight, const void *workspace, size_t workspace_bytes, int64_t T_cap,
                  float *vertices /* [T_cap][3][3] */, float *colors /* [T_cap][3][3] or NULL */, int64_t *keys /* [T_cap][3] */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_TSDF_H */
