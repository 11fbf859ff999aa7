// dssim.hip -- L = (1 - lambda) L1 + lambda (1 - SSIM) and its pixel gradient (include/gsr_loss.h has the formulas).
//
// Two passes over 32 x 16 pixel tiles, 256 threads each ("D-SSIM loss"):
//   dssim_stats_kernel    stages a channel of both images with a 5-pixel halo in LDS, forms the five window sums separably
//                         (11 horizontal taps into LDS, then 11 vertical taps), and from them S, the L1 term and the per-pixel
//                         adjoint weights alpha / beta / gamma, pre-scaled by lambda / (3 H W), into three planes per channel of
//                         the workspace.  Each workgroup leaves its L1 and SSIM partial sums in the workspace.
//   dssim_adjoint_kernel  convolves alpha / beta / gamma with the same separable window and writes pixel_grad.
//   dssim_finish_kernel   one workgroup adds the partial sums in a fixed order into the two caller words.
// The other join, one kernel that recomputes alpha / beta / gamma on a 5-pixel halo of its tile instead of the 9-float-per-pixel
// workspace, measured 109 against 71 us per call at 800 x 800 (profiles/dssim_kernels/ab_join.txt) and was removed.
#include <math.h>

#include "dssim_window.h"
#include "gsr_loss.h"

namespace {

// ---- pass 1: window statistics of the tile, S, L1, and alpha / beta / gamma into the workspace planes ----
__global__ __launch_bounds__(NT) void dssim_stats_kernel(const float *__restrict__ rendered, const float *__restrict__ target,
                                                         float *__restrict__ planes, float2 *__restrict__ part, int W, int H, DssimW k,
                                                         float kscale, int want_grad)
{
    constexpr int SW = TX + 2 * RAD, SH = TY + 2 * RAD, P = 2;
    __shared__ float s_x[SW * SH], s_y[SW * SH], s_h[5 * SH * TX];
    __shared__ float s_red[8];
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
    const int u = threadIdx.x & (TX - 1), v0 = (threadIdx.x / TX) * P;   // this thread's two output pixels (u, v0), (u, v0 + 1)
    const int gx = tx0 + u;
    const size_t HW = (size_t)H * W;
    float inv_wp[P];
    {
        const float sx = border_sum(k, gx, W);
#pragma unroll
        for (int p = 0; p < P; ++p) inv_wp[p] = 1.0f / (sx * border_sum(k, ty0 + v0 + p, H));
    }
    float l1 = 0.0f, ss = 0.0f;
    for (int c = 0; c < 3; ++c) {
        stage<SW, SH>(rendered, 3, c, tx0 - RAD, ty0 - RAD, W, H, s_x);
        stage<SW, SH>(target, 3, c, tx0 - RAD, ty0 - RAD, W, H, s_y);
        __syncthreads();
        hsum_stats<SW, SH, 2>(s_x, s_y, s_h, k);
        __syncthreads();
        float acc[5][P];
        vsum<5, TX, SH, P>(s_h, u, v0, k, acc);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int gy = ty0 + v0 + p;
            if (gx >= W || gy >= H) continue;
            const float s[5] = {acc[0][p], acc[1][p], acc[2][p], acc[3][p], acc[4][p]};
            float al, be, ga;
            ss += ssim_terms(s, inv_wp[p], kscale, al, be, ga);
            const int li = (v0 + p + RAD) * SW + u + RAD;
            l1 += fabsf(s_x[li] - s_y[li]);
            if (want_grad) {
                const size_t g = (size_t)gy * W + gx;
                planes[(3 * c + 0) * HW + g] = al;
                planes[(3 * c + 1) * HW + g] = be;
                planes[(3 * c + 2) * HW + g] = ga;
            }
        }
        __syncthreads();   // s_x / s_y / s_h are restaged for the next channel
    }
    block_partials(l1, ss / 3.0f, part, s_red);
}

// ---- pass 2: (w * alpha) + 2 x (w * beta) + y (w * gamma), combined with the L1 sign term into pixel_grad ----
__global__ __launch_bounds__(NT) void dssim_adjoint_kernel(const float *__restrict__ rendered, const float *__restrict__ target,
                                                           const float *__restrict__ planes, float *__restrict__ pixel_grad, int W, int H,
                                                           DssimW k, float l1w)
{
    constexpr int SW = TX + 2 * RAD, SH = TY + 2 * RAD, P = 2;
    __shared__ float s_a[3 * SW * SH], s_h[3 * SH * TX];
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
    const int u = threadIdx.x & (TX - 1), v0 = (threadIdx.x / TX) * P;
    const int gx = tx0 + u;
    const size_t HW = (size_t)H * W;
    float g[P][3] = {};
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int q = 0; q < 3; ++q) stage<SW, SH>(planes + (3 * c + q) * HW, 1, 0, tx0 - RAD, ty0 - RAD, W, H, s_a + q * SW * SH);
        __syncthreads();
        hsum3<SW, SH, 2>(s_a, s_h, k);
        __syncthreads();
        float acc[3][P];
        vsum<3, TX, SH, P>(s_h, u, v0, k, acc);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int gy = ty0 + v0 + p;
            if (gx >= W || gy >= H) continue;
            const size_t i = 3 * ((size_t)gy * W + gx) + c;
            const float x = rendered[i], y = target[i];
            const float adj = fmaf(y, acc[2][p], fmaf(2.0f * x, acc[1][p], acc[0][p]));
            g[p][c] = l1w * (x - y < 0.0f ? -1.0f : 1.0f) - adj;
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int gy = ty0 + v0 + p;
        if (gx >= W || gy >= H) continue;
        float *o = pixel_grad + 3 * ((size_t)gy * W + gx);
        o[0] = g[p][0]; o[1] = g[p][1]; o[2] = g[p][2];
    }
}

// ---- the two sums: one workgroup adds the per-workgroup partials in a fixed order ----
__global__ __launch_bounds__(NT) void dssim_finish_kernel(const float2 *__restrict__ part, int n, float *__restrict__ l1_sum,
                                                          float *__restrict__ ssim_sum)
{
    __shared__ float s_red[8];
    float l1 = 0.0f, ss = 0.0f;
    for (int i = threadIdx.x; i < n; i += NT) {
        const float2 v = part[i];
        l1 += v.x;
        ss += v.y;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        l1 += __shfl_xor(l1, d, 64);
        ss += __shfl_xor(ss, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_red[threadIdx.x >> 6] = l1;
        s_red[4 + (threadIdx.x >> 6)] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *l1_sum = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        *ssim_sum = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
    }
}

} // namespace

extern "C" {

size_t gsr_dssim_workspace_bytes(int32_t W, int32_t H)
{
    return dssim_workspace_bytes(W, H);
}

int gsr_l1_dssim_loss_grad(const float *rendered, const float *target, float *pixel_grad, float *l1_sum, float *ssim_sum, int32_t W, int32_t H,
                           float lambda_dssim, int32_t window, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rendered || !target || !l1_sum || !ssim_sum || !workspace) return GSR_E_NULL;
    if (W <= 0 || H <= 0 || (int64_t)W * H > MAX_PIXELS || !(lambda_dssim >= 0.0f && lambda_dssim <= 1.0f) ||
        (window != GSR_SSIM_WINDOW_REFERENCE && window != GSR_SSIM_WINDOW_GAUSSIAN))
        return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(target) || !gsr_aligned16(pixel_grad) || !gsr_aligned16(workspace)) return GSR_E_ALIGN;
    if (((uintptr_t)l1_sum & 3u) || ((uintptr_t)ssim_sum & 3u)) return GSR_E_ALIGN;   // single floats: any slot of a float curve
    if (workspace_bytes < gsr_dssim_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    const DssimW k = window_taps(window == GSR_SSIM_WINDOW_REFERENCE);
    const double n = 3.0 * (double)W * (double)H;
    const float l1w = (float)((1.0 - (double)lambda_dssim) / n), kscale = (float)((double)lambda_dssim / n);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)gsr_div_up(W, TX), (unsigned)gsr_div_up(H, TY));
    float2 *part = reinterpret_cast<float2 *>(workspace);
    float *planes = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + partial_bytes(W, H));
    hipLaunchKernelGGL(dssim_stats_kernel, grid, dim3(NT), 0, s, rendered, target, planes, part, W, H, k, kscale, pixel_grad != nullptr);
    if (pixel_grad) hipLaunchKernelGGL(dssim_adjoint_kernel, grid, dim3(NT), 0, s, rendered, target, planes, pixel_grad, W, H, k, l1w);
    hipLaunchKernelGGL(dssim_finish_kernel, dim3(1), dim3(NT), 0, s, part, (int)(grid.x * grid.y), l1_sum, ssim_sum);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_E_HIP;
}

} // extern "C"
