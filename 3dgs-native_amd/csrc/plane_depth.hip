// plane_depth.hip -- the ray-plane intersection depth over a frame's lists, its gradient into the backward's accumulator records, and
// the per-Gaussian slopes with their gradient (include/gsr_plane_depth.h), for gfx950.
//
// plane_slopes_kernel<BWD>: one thread per Gaussian, the header's steps (a) and (d) word for word; the view matrix travels as a
// kernel argument.
//
// plane_depth_kernel<BWD> is normal_render.hip's walk with another third word: frame_walk.h's FrameWalk stages the tile's list in
// 48-byte records, 1 / depth in the spare float of the second word (as distortion.hip has it) and the two slopes in the third.
//   - forward: two fused multiply-adds and a clamp per entry for m, one more for the running image: one register per lane.
//   - backward: that file's ValueTile<9, 3> with u = g m: the same 27 rows, the same two-lanes-per-row flush, the same 43 KB of LDS
//     per workgroup; the last three values go to the Gaussian's row of dL_dplane_moments instead of dL_dnormals.
#include <math.h>

#include "frame_walk.h"
#include "gsr_plane_depth.h"

namespace {

constexpr int SLOTS = 3;     // entries per flush of the backward (normal_render.hip's choice, for its reasons)
constexpr int VALS = 9;      // S1, S2, Sxx, Sxy, Syy, Sop, S0, Sx, Sy: the last three are the Gaussian's row of dL_dplane_moments
typedef ValueTile<VALS, SLOTS> Tile;

struct ViewK {
    float v[16];
};

// ---- (a), (d): one thread per Gaussian ----
// BWD: `in` is dL_dplane_moments [N][3], `out` dL_dmean3D [N][3] (added to), `out2` dL_dnormals [N][3]; else `out` is slopes [N][2].
template <bool BWD>
__global__ __launch_bounds__(256) void plane_slopes_kernel(long long N, const float *__restrict__ normals, const float *__restrict__ scales,
                                                           const float *__restrict__ means, ViewK V, float tan_fovx, float tan_fovy, int W, int H,
                                                           const float *__restrict__ in, float *__restrict__ out, float *__restrict__ out2)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float n[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    const float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
    const float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    float pv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) pv[j] = ((V.v[j] * p[0] + V.v[4 + j] * p[1]) + V.v[8 + j] * p[2]) + V.v[12 + j];
    const float t = (n[0] * pv[0] + n[1] * pv[1]) + n[2] * pv[2];
    const float l = __fsqrt_rn((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2]);
    const float lo = fminf(fminf(s[0], s[1]), s[2]);
    const float mid = fmaxf(fminf(s[0], s[1]), fminf(fmaxf(s[0], s[1]), s[2]));
    const bool fallback = (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) || !(pv[2] > GSR_PLANE_DEPTH_NEAR) || !(-t >= GSR_PLANE_DEPTH_MIN_COS * l) ||
                          !(lo <= GSR_PLANE_DEPTH_MAX_FLATNESS * mid);
    const float kx = __fdiv_rn(2.0f * tan_fovx, (float)W), ky = __fdiv_rn(2.0f * tan_fovy, (float)H);
    const float td = fallback ? 1.0f : t; // the divisions below are not taken on the fallback branch: keep them finite
    const float gx = __fdiv_rn(n[0] * kx, td), gy = __fdiv_rn(n[1] * ky, td);
    if (!BWD) {
        *reinterpret_cast<float2 *>(out + 2 * i) = fallback ? make_float2(0.0f, 0.0f) : make_float2(gx, gy);
        return;
    }
    const float S0 = in[3 * i], Sx = in[3 * i + 1], Sy = in[3 * i + 2];
    const float invd = pv[2] > 0.0f ? __fdiv_rn(1.0f, pv[2]) : 0.0f;
    float dn[3] = {0.0f, 0.0f, 0.0f}, dp[3] = {0.0f, 0.0f, -((invd * invd) * S0)};
    if (!fallback) {
        const float M = (invd * S0 + gx * Sx) + gy * Sy;
        const float R[3] = {(pv[0] * invd) * S0 + kx * Sx, (pv[1] * invd) * S0 + ky * Sy, S0};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dn[j] = __fdiv_rn(R[j] - M * pv[j], t);
            dp[j] = -__fdiv_rn(M * n[j], t);
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        out[3 * i + r] += (V.v[4 * r] * dp[0] + V.v[4 * r + 1] * dp[1]) + V.v[4 * r + 2] * dp[2];
        out2[3 * i + r] = dn[r];
    }
}

// ---- (b), (c): the list walk ----
// BWD: `g_in` is dL_dout [H][W], `img` the stored forward image (read), `acc` the accumulator records, `dmom` dL_dplane_moments [N][3]
// (cleared by the caller); else `img` is written.
template <bool BWD>
__global__ __launch_bounds__(256) void plane_depth_kernel(FrameK f, const float *__restrict__ invd, long long invd_stride, const float *__restrict__ slopes,
                                                          const float *__restrict__ g_in, float *img, float *__restrict__ acc, float *__restrict__ dmom)
{
    __shared__ Tile::V<BWD> s_v; // the value tile: the backward's alone
    __shared__ Tile::Red s_red;
    __shared__ Tile::Con s_con;
    const FrameWalk walk(f);
    const bool inside = walk.inside;
    const size_t pix = walk.pix;

    float o = 0.0f;                              // forward: the running image
    float g = 0.0f, total = 0.0f, P = 0.0f;
    if (BWD && inside && walk.nc > 0) {
        g = g_in[pix];
        total = g * img[pix];
    }
    Tile tile(s_v[BWD ? walk.wv : 0], s_red[walk.wv], s_con[walk.wv], walk, f, acc, dmom, 3, 0);

    float T = 1.0f;
    walk.run<3>(
        f, DepthFill{invd, invd_stride, slopes},
        [&](const float4 &ra, const float4 &rb, const float4 &rc, float dx, float dy, float G, float t, bool applied) {
            float mr;
            const float m = plane_inv_depth(rb.w, rc.x, rc.y, dx, dy, mr);
            if (BWD) {
                if (__builtin_amdgcn_ballot_w64(applied) != 0ull) {
                    float v[VALS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (applied) {
                        const float u = g * m;
                        const float w = t * T;
                        P = P + w * u;
                        const float R = total - P;
                        const float om = 1.0f - t;
                        const float q = T * u - R / om;
                        const float gd = G * q;
                        const float h = rb.y * gd;
                        const float hx = h * dx, hy = h * dy;
                        v[0] = hx; v[1] = hy; v[2] = hx * dx; v[3] = hx * dy; v[4] = hy * dy; v[5] = gd;
                        if (m == mr) { // not clamped
                            const float wg = w * g;
                            v[6] = wg; v[7] = wg * (-dx); v[8] = wg * (-dy);
                        }
                        T = T * om;
                    }
                    tile.file(v, ra, rb);
                }
            } else if (applied) {
                const float w = t * T;
                T = T * (1.0f - t);
                o = __builtin_fmaf(w, m, o);
            }
        });
    if (BWD) {
        tile.finish();
    } else if (inside) {
        img[pix] = o;
    }
}

int check_gaussians(int64_t N, const float *normals, const float *scales, const float *means, const float *view, float tan_fovx, float tan_fovy,
                    int32_t W, int32_t H, const void *a, const void *b, const void *c)
{
    if (!normals || !scales || !means || !view || !a || !b || !c) return GSR_E_NULL;
    if (N < 1 || N > 0x7FFFFFFFll) return GSR_E_DIMS;
    for (int k = 0; k < 16; ++k)
        if (!isfinite(view[k])) return GSR_E_DIMS;
    if (!isfinite(tan_fovx) || !isfinite(tan_fovy) || !(tan_fovx > 0.0f) || !(tan_fovy > 0.0f)) return GSR_E_DIMS;
    if (W < 1 || H < 1 || W > GSR_FEATURES_MAX_SIDE || H > GSR_FEATURES_MAX_SIDE) return GSR_E_DIMS;
    if (!all_aligned16(normals, scales, means, a, b, c)) return GSR_E_ALIGN;
    return GSR_OK;
}

ViewK view_k(const float *view)
{
    ViewK v;
    for (int k = 0; k < 16; ++k) v.v[k] = view[k];
    return v;
}

} // namespace

extern "C" int gsr_plane_slopes(int64_t N, const float *normals, const float *scales, const float *means, const float *viewmatrix, float tan_fovx,
                                float tan_fovy, int32_t W, int32_t H, float *slopes, void *stream)
{
    const int rc = check_gaussians(N, normals, scales, means, viewmatrix, tan_fovx, tan_fovy, W, H, slopes, slopes, slopes);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL((plane_slopes_kernel<false>), dim3((unsigned)gsr_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, (long long)N, normals, scales,
                       means, view_k(viewmatrix), tan_fovx, tan_fovy, (int)W, (int)H, nullptr, slopes, nullptr);
    return gsr_done();
}

extern "C" int gsr_plane_slopes_backward(int64_t N, const float *normals, const float *scales, const float *means, const float *viewmatrix,
                                         float tan_fovx, float tan_fovy, int32_t W, int32_t H, const float *dL_dplane_moments, float *dL_dmean3D,
                                         float *dL_dnormals, void *stream)
{
    const int rc = check_gaussians(N, normals, scales, means, viewmatrix, tan_fovx, tan_fovy, W, H, dL_dplane_moments, dL_dmean3D, dL_dnormals);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL((plane_slopes_kernel<true>), dim3((unsigned)gsr_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, (long long)N, normals, scales,
                       means, view_k(viewmatrix), tan_fovx, tan_fovy, (int)W, (int)H, dL_dplane_moments, dL_dmean3D, dL_dnormals);
    return gsr_done();
}

extern "C" int gsr_plane_depth_forward(const GsrDistortionFrame *frame, const float *slopes, float *out, void *stream)
{
    const int rc = check_frame(frame, slopes, out);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    // a frame with D = 0 walks nothing: every pixel is written as 0
    hipLaunchKernelGGL((plane_depth_kernel<false>), dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, frame->inv_depth,
                       (long long)frame->inv_depth_stride, slopes, nullptr, out, nullptr, nullptr);
    return gsr_done();
}

extern "C" int gsr_plane_depth_backward(const GsrDistortionFrame *frame, const float *slopes, const float *dL_dout, const float *out, float *accumulators,
                                        float *dL_dplane_moments, void *stream)
{
    const int rc = check_frame(frame, slopes, dL_dout, out, accumulators, dL_dplane_moments);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (hipMemsetAsync(dL_dplane_moments, 0, sizeof(float) * 3 * (size_t)k.N, (hipStream_t)stream) != hipSuccess) return GSR_E_HIP;
    if (k.D == 0) return gsr_done(); // nothing was blended: nothing to add
    hipLaunchKernelGGL((plane_depth_kernel<true>), dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, frame->inv_depth,
                       (long long)frame->inv_depth_stride, slopes, dL_dout, const_cast<float *>(out), accumulators, dL_dplane_moments);
    return gsr_done();
}
