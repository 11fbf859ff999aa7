/*
 * gsr_filter3d.h -- the 3D smoothing filter of Mip-Splatting for libgsr_hip.so: a lower bound on every Gaussian's world-space size,
 * set by what the training views could resolve, as a map on (scales, opacity) with its transpose.
 *
 * gsr_antialias.h is the screen-space half of Mip-Splatting (the opacity compensation of the 0.3 px^2 blur).  This is the other
 * half.  Nothing stops training from shrinking a Gaussian below the sampling interval of every camera that ever saw it; such a
 * Gaussian dilates or erodes as soon as the view zooms in or out.  The filter convolves each Gaussian with an isotropic Gaussian of
 * standard deviation filter_3d[i] (scene units) and keeps its integral.
 *
 * Sampling rate.  A view is 16 floats of view matrix as stored, a focal length in pixels, W and H (GsrFilterView).  With
 * p_view = (p, 1) * view under the row-vector convention of the forward (rows accumulated in ascending order, quirk Q3 inherited),
 * view v SEES Gaussian i when
 *     p_view.z > 0.2      |p_view.x / p_view.z * focal| <= 1.15 * W / 2      |p_view.y / p_view.z * focal| <= 1.15 * H / 2
 * (Mip-Splatting's 15 % margin about the image centre; the kernel tests |p_view.x| * focal <= (1.15 * W / 2) * p_view.z, the same
 * statement without the division), and then
 *     nu_i = max over seeing views of focal_v / z_v
 * A Gaussian that no view sees takes the smallest nu among those that were seen (Mip-Splatting's distance[~valid] =
 * distance[valid].max(), generalised to views of different focal lengths); if nothing is seen at all, V = 0 included, the filter
 * is 0.  filter_3d[i] = sqrt(variance) / nu_i, variance = 0.2 by default.  With one focal length this is Mip-Splatting's
 * compute_3D_filter.
 *
 * The map, with f = filter_3d[i] and k = x, y, z:
 *     s'_k = sqrt(s_k^2 + f^2)      r_k = |s_k| / s'_k      opacity' = opacity * (r_x r_y r_z)
 * f == 0 is an exact pass-through: bits are copied and nothing divides by s'.  The rasterizer runs on (s', opacity'); scale_modifier
 * applies after the filter.  Scales and opacities are raw (no activations, quirk Q5), which is what makes the map closed-form.
 *
 * Its transpose, given g_s' (3 floats) and g_o' = the backward's dL/d(s', opacity'):
 *     dL/dopacity = g_o' r_x r_y r_z
 *     dL/ds_k     = g_s'_k s_k / s'_k + g_o' opacity sign(s_k) (prod over j != k of r_j) f^2 / s'_k^3        (sign(0) = 0)
 * with no division by s_k; f == 0 is a pass-through.
 *
 * Contract
 *   - Caller-owned memory only: no allocation, no host synchronisation, everything is enqueued on `stream`.  Every array is 16-byte
 *     aligned.  `views` is DEVICE memory, V records of 80 bytes.
 *   - Arguments are checked before anything is enqueued, in this order: GSR_E_NULL (an array of a call with N > 0; `views` with
 *     V > 0), GSR_E_DIMS (N < 0 or N > 2^31 - 1, V < 0, variance not positive and finite), then N = 0 returns GSR_OK and enqueues
 *     nothing, GSR_E_ALIGN, GSR_E_WORKSPACE (ws NULL or smaller than gsr_filter3d_workspace_bytes(N)).
 *   - gsr_filter3d_from_views: V = 0 writes zeros.  filter_3d is a pure function of the inputs: max and min do not depend on
 *     order, so it is bitwise reproducible and bitwise equal on every rank of a data-parallel run; no collective is needed.  Two
 *     launches behind a 4-byte clear of ws: one lane per Gaussian loops over the views (wave-uniform records, read once per wave)
 *     and leaves nu, or 0, in filter_3d; the smallest positive nu is reduced as uint bits (positive floats order like their bit
 *     patterns), per wave and then with at most one vector atomic per wave into ws (a wave whose minimum cannot lower the word it
 *     has just read skips it: the word only falls, so nothing is lost); the second launch substitutes the unseen Gaussians and
 *     converts nu to filter_3d.  An unseen Gaussian therefore carries exactly the bits of the largest seen filter_3d.
 *   - gsr_filter3d_apply: scales_out / opacity_out may be scales / opacity (every lane reads its rows before it writes them).
 *   - gsr_filter3d_backward may run in place: dL_dscale == dL_dscale_f and dL_dopacity == dL_dopacity_f; a gradient arena's
 *     segments qualify.  scales, opacity and filter_3d are the RAW parameters and the filter the forward used.
 *   - sqrt and division are the correctly rounded ones and no expression is contracted (-ffp-contract=off).
 *   - Nothing else changes: gsr.h, its structs, GSR_ABI_VERSION, workspace sizes and every existing entry point are as before.
 */
#ifndef GSR_FILTER3D_H
#define GSR_FILTER3D_H

#include "gsr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct GsrFilterView {
    float view[16]; /* the view matrix as stored (GsrCamera.view) */
    float focal;    /* pixels (GsrCamera.focal_x) */
    int32_t W, H;
    int32_t pad;
} GsrFilterView; /* 80 bytes */

#define GSR_FILTER3D_VARIANCE 0.2f /* the default variance: filter_3d = sqrt(variance) / nu */
#define GSR_FILTER3D_MARGIN 0.15f  /* a view sees what projects within (1 + margin) half-images of its centre */
#define GSR_FILTER3D_NEAR 0.2f     /* ... and lies farther than this in front of it */

size_t gsr_filter3d_workspace_bytes(int64_t N);
int gsr_filter3d_from_views(int64_t N, const float *means, int32_t V, const GsrFilterView *views /* device [V] */, float variance,
                            float *filter_3d /* [N] out */, void *ws, size_t ws_bytes, void *stream);
int gsr_filter3d_apply(int64_t N, const float *scales, const float *opacity, const float *filter_3d, float *scales_out,
                       float *opacity_out, void *stream);
int gsr_filter3d_backward(int64_t N, const float *scales, const float *opacity, const float *filter_3d, const float *dL_dscale_f,
                          const float *dL_dopacity_f, float *dL_dscale, float *dL_dopacity, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_FILTER3D_H */
