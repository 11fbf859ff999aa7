// dssim.hip -- L = (1 - lambda) L1 + lambda (1 - SSIM) and its pixel gradient (include/gsr_loss.h has the formulas), and the same
// colour loss under per-pixel weights m (include/gsr_weighted_loss.h).
//
// Two passes over 32 x 16 pixel tiles, 256 threads each ("D-SSIM loss"), each one kernel in two instantiations:
//   dssim_stats_kernel    stages a channel of both images with a 5-pixel halo in LDS, forms the five window sums separably
//                         (11 horizontal taps into LDS, then 11 vertical taps), and from them S, the L1 term and the per-pixel
//                         adjoint weights alpha / beta / gamma, pre-scaled by lambda / (3 H W), into three planes per channel of
//                         the workspace.  Each workgroup leaves its L1 and SSIM partial sums in the workspace.
//   dssim_adjoint_kernel  convolves alpha / beta / gamma with the same separable window and writes pixel_grad.
// WEIGHTED adds one coalesced read of m at the output pixel (no halo: the weight multiplies the loss map, not the images): the
// planes hold m alpha, m beta, m gamma scaled by lambda / (3 M), the partials m |x - y| and m S, and the sign term is times m.  Its
// two pointers (weight, weight_total) are a parameter pack behind `target`, empty in the plain kernels, which take their scales from
// the host and do no arithmetic for any of this.
//   weight_sum_kernel     M = sum of m, flat over the image: one partial per workgroup.
//   weighted_l1_kernel    m |x - y| and scale / (3 M) m sign(x - y), four pixels per thread; partials likewise.
// Every sum is a fixed-order sum with pairwise wave sums, finished by gsr_finish_kernel ("The fixed-order sum").
// M arrives as a device float: every kernel that scales by it forms 1 / (3 M) itself, 0 when M = 0, so an all-zero mask gives zeros.
// A zero weight gives +0 whatever the sign of x - y, so what a masked region holds never shows in the bits of the gradient.
// The other join, one kernel that recomputes alpha / beta / gamma on a 5-pixel halo of its tile instead of the 9-float-per-pixel
// workspace, measured 109 against 71 us per call at 800 x 800 (profiles/dssim_kernels/ab_join.txt) and was removed.
#include <float.h>
#include <math.h>

#include "dssim_window.h"
#include "fixed_sum.h"
#include "gsr_loss.h"
#include "gsr_weighted_loss.h"

namespace {

constexpr int SUM_BLOCK_PIXELS = 4 * NT;   // the flat kernels: four pixels per thread and round
constexpr int MAX_SUM_BLOCKS = 512;        // two workgroups per CU, grid stride, as gsr_l1_loss_grad

__device__ __forceinline__ float inv_3m(const float *weight_total)
{
    const float M = *weight_total;
    return M > 0.0f ? 1.0f / (3.0f * M) : 0.0f;
}

// w sign(d) with sign(0) = +1, and +0 for w = 0
__device__ __forceinline__ float signed_weight(float w, float d) { return (d < 0.0f && w > 0.0f) ? -w : w; }

// ---- M: flat over the H * W weights, a float4 per lane ----
__global__ __launch_bounds__(NT) void weight_sum_kernel(const float *__restrict__ weight, float *__restrict__ part, int64_t n)
{
    __shared__ float s_red[GSR_SUM_WAVES][1];
    float acc = 0.0f;
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
        const float4 m = reinterpret_cast<const float4 *>(weight)[i];
        acc += (m.x + m.y) + (m.z + m.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) acc += weight[(n4 << 2) + threadIdx.x];   // tail (< 4 pixels)
    const GsrBlockSums<float, 1> b = gsr_block_sum<NT>(acc, s_red);
    if (threadIdx.x == 0) part[blockIdx.x] = b.pairwise(0);
}

// ---- weighted L1: four pixels per thread (one float4 of weights, three of each image) ----
__global__ __launch_bounds__(NT) void weighted_l1_kernel(const float *__restrict__ rendered, const float *__restrict__ target,
                                                         const float *__restrict__ weight, const float *__restrict__ weight_total,
                                                         float *__restrict__ pixel_grad, float *__restrict__ part, int64_t n, float scale)
{
    __shared__ float s_red[GSR_SUM_WAVES][1];
    const float c = scale * inv_3m(weight_total);
    float acc = 0.0f;
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
        const float4 m4 = reinterpret_cast<const float4 *>(weight)[i];
        const float m[4] = {m4.x, m4.y, m4.z, m4.w};
        float d[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4 r = reinterpret_cast<const float4 *>(rendered)[3 * i + q];
            const float4 t = reinterpret_cast<const float4 *>(target)[3 * i + q];
            d[4 * q + 0] = r.x - t.x; d[4 * q + 1] = r.y - t.y; d[4 * q + 2] = r.z - t.z; d[4 * q + 3] = r.w - t.w;
        }
        float g[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            const float mp = m[e / 3];
            acc += mp * fabsf(d[e]);
            g[e] = signed_weight(c * mp, d[e]);
        }
        if (pixel_grad) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                reinterpret_cast<float4 *>(pixel_grad)[3 * i + q] = make_float4(g[4 * q + 0], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {   // tail (< 4 pixels)
        const int64_t p = (n4 << 2) + threadIdx.x;
        const float mp = weight[p];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float d = rendered[3 * p + ch] - target[3 * p + ch];
            acc += mp * fabsf(d);
            if (pixel_grad) pixel_grad[3 * p + ch] = signed_weight(c * mp, d);
        }
    }
    const GsrBlockSums<float, 1> b = gsr_block_sum<NT>(acc, s_red);
    if (threadIdx.x == 0) part[blockIdx.x] = b.pairwise(0);
}

// ---- pass 1: window statistics of the tile, S, L1, and alpha / beta / gamma into the workspace planes ----
// `scale`: kscale = lambda / (3 H W) from the host; WEIGHTED: lambda, and the kernel forms kscale = lambda / (3 M)
template <bool WEIGHTED = false, class... Wt>
__global__ __launch_bounds__(NT) void dssim_stats_kernel(const float *__restrict__ rendered, const float *__restrict__ target, Wt... wt,
                                                         float *__restrict__ planes, float2 *__restrict__ part, int W, int H, DssimW k,
                                                         float scale, int want_grad)
{
    static_assert(sizeof...(Wt) == (WEIGHTED ? 2 : 0), "weight and weight_total, in the weighted kernel only");
    constexpr int SW = TX + 2 * RAD, SH = TY + 2 * RAD, P = 2;
    __shared__ float s_x[SW * SH], s_y[SW * SH], s_h[5 * SH * TX];
    __shared__ float s_red[2][GSR_SUM_WAVES];
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
    const int u = threadIdx.x & (TX - 1), v0 = (threadIdx.x / TX) * P;   // this thread's two output pixels (u, v0), (u, v0 + 1)
    const int gx = tx0 + u;
    const size_t HW = (size_t)H * W;
    float kscale = scale, inv_wp[P], m[P];   // m: the weights of the two pixels, WEIGHTED only
    const float *weight = nullptr;
    if constexpr (WEIGHTED) {
        const float *const w[] = {wt...};
        weight = w[0], kscale = scale * inv_3m(w[1]);
    }
    {
        const float sx = border_sum(k, gx, W);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int gy = ty0 + v0 + p;
            inv_wp[p] = 1.0f / (sx * border_sum(k, gy, H));
            if constexpr (WEIGHTED) m[p] = (gx < W && gy < H) ? weight[(size_t)gy * W + gx] : 0.0f;
        }
    }
    float sums[2] = {};   // L1, SSIM
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
            float S = ssim_terms(s, inv_wp[p], kscale, al, be, ga);
            if constexpr (WEIGHTED) S = m[p] * S;
            sums[1] += S;
            const int li = (v0 + p + RAD) * SW + u + RAD;
            float ad = fabsf(s_x[li] - s_y[li]);
            if constexpr (WEIGHTED) ad = m[p] * ad;
            sums[0] += ad;
            if (want_grad) {
                if constexpr (WEIGHTED) al = m[p] * al, be = m[p] * be, ga = m[p] * ga;
                const size_t g = (size_t)gy * W + gx;
                planes[(3 * c + 0) * HW + g] = al;
                planes[(3 * c + 1) * HW + g] = be;
                planes[(3 * c + 2) * HW + g] = ga;
            }
        }
        __syncthreads();   // s_x / s_y / s_h are restaged for the next channel
    }
    sums[1] /= 3.0f;
    const auto b = gsr_block_sums<NT>(sums, s_red);
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = make_float2(b.pairwise(0), b.pairwise(1));
}

// ---- pass 2: (w * alpha) + 2 x (w * beta) + y (w * gamma), combined with the L1 sign term into pixel_grad ----
// `l1w`: (1 - lambda) / (3 H W) from the host; WEIGHTED: 1 - lambda, and the sign term is times m / (3 M)
template <bool WEIGHTED = false, class... Wt>
__global__ __launch_bounds__(NT) void dssim_adjoint_kernel(const float *__restrict__ rendered, const float *__restrict__ target, Wt... wt,
                                                           const float *__restrict__ planes, float *__restrict__ pixel_grad, int W, int H,
                                                           DssimW k, float l1w)
{
    static_assert(sizeof...(Wt) == (WEIGHTED ? 2 : 0), "weight and weight_total, in the weighted kernel only");
    constexpr int SW = TX + 2 * RAD, SH = TY + 2 * RAD, P = 2;
    __shared__ float s_a[3 * SW * SH], s_h[3 * SH * TX];
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
    const int u = threadIdx.x & (TX - 1), v0 = (threadIdx.x / TX) * P;
    const int gx = tx0 + u;
    const size_t HW = (size_t)H * W;
    float l1m[P];   // l1w m / (3 M) at the two pixels, WEIGHTED only
    if constexpr (WEIGHTED) {
        const float *const w[] = {wt...};
        const float l1c = l1w * inv_3m(w[1]);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int gy = ty0 + v0 + p;
            l1m[p] = (gx < W && gy < H) ? l1c * w[0][(size_t)gy * W + gx] : 0.0f;
        }
    }
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
            if constexpr (WEIGHTED) g[p][c] = signed_weight(l1m[p], x - y) - adj;
            else g[p][c] = l1w * (x - y < 0.0f ? -1.0f : 1.0f) - adj;
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

bool window_ok(int32_t window) { return window == GSR_SSIM_WINDOW_REFERENCE || window == GSR_SSIM_WINDOW_GAUSSIAN; }
unsigned sum_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, gsr_record_count(n, SUM_BLOCK_PIXELS, MAX_SUM_BLOCKS)); }

// the launches of both D-SSIM entry points behind their checks; weight == NULL: the plain kernels, scales from the host
int dssim_launch(const float *rendered, const float *target, const float *weight, const float *weight_total, float *pixel_grad, float *l1_sum,
                 float *ssim_sum, int32_t W, int32_t H, float lambda_dssim, int32_t window, void *workspace, hipStream_t s)
{
    const DssimW k = window_taps(window == GSR_SSIM_WINDOW_REFERENCE);
    const dim3 grid((unsigned)gsr_div_up(W, TX), (unsigned)gsr_div_up(H, TY));
    float2 *part = reinterpret_cast<float2 *>(workspace);
    float *planes = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + partial_bytes(W, H));
    const int want_grad = pixel_grad != nullptr;
    if (weight) {
        using Wp = const float *__restrict__;   // the pack's two types: the weights are only read, as every other input
        hipLaunchKernelGGL((dssim_stats_kernel<true, Wp, Wp>), grid, dim3(NT), 0, s, rendered, target, weight, weight_total, planes, part, W, H, k,
                           lambda_dssim, want_grad);
        if (pixel_grad)
            hipLaunchKernelGGL((dssim_adjoint_kernel<true, Wp, Wp>), grid, dim3(NT), 0, s, rendered, target, weight, weight_total,
                               (const float *)planes, pixel_grad, W, H, k, 1.0f - lambda_dssim);
    } else {
        const double n = 3.0 * (double)W * (double)H;
        const float l1w = (float)((1.0 - (double)lambda_dssim) / n), kscale = (float)((double)lambda_dssim / n);
        hipLaunchKernelGGL(dssim_stats_kernel<false>, grid, dim3(NT), 0, s, rendered, target, planes, part, W, H, k, kscale, want_grad);
        if (pixel_grad)
            hipLaunchKernelGGL(dssim_adjoint_kernel<false>, grid, dim3(NT), 0, s, rendered, target, (const float *)planes, pixel_grad, W, H, k, l1w);
    }
    hipLaunchKernelGGL((gsr_finish_kernel<2, 2, 2>), dim3(1), dim3(NT), 0, s, reinterpret_cast<const float *>(part), (int)(grid.x * grid.y),
                       GsrSumOut<2>{{l1_sum, ssim_sum}});
    return gsr_done();
}

} // namespace

extern "C" {

size_t gsr_dssim_workspace_bytes(int32_t W, int32_t H) { return dssim_workspace_bytes(W, H); }

int gsr_l1_dssim_loss_grad(const float *rendered, const float *target, float *pixel_grad, float *l1_sum, float *ssim_sum, int32_t W, int32_t H,
                           float lambda_dssim, int32_t window, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rendered || !target || !l1_sum || !ssim_sum || !workspace) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H) || !(lambda_dssim >= 0.0f && lambda_dssim <= 1.0f) || !window_ok(window)) return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(target) || !gsr_aligned16(pixel_grad) || !gsr_aligned16(workspace)) return GSR_E_ALIGN;
    if (!gsr_aligned4(l1_sum) || !gsr_aligned4(ssim_sum)) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_dssim_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    return dssim_launch(rendered, target, nullptr, nullptr, pixel_grad, l1_sum, ssim_sum, W, H, lambda_dssim, window, workspace, (hipStream_t)stream);
}

size_t gsr_weight_total_workspace_bytes(int32_t W, int32_t H)
{
    return gsr_image_dims_ok(W, H) ? gsr_align(sizeof(float) * sum_blocks((int64_t)W * H)) : 0;
}

int gsr_weight_total(const float *weight, int32_t W, int32_t H, float *total, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!weight || !total || !workspace) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H)) return GSR_E_DIMS;
    if (!gsr_aligned16(weight) || !gsr_aligned16(workspace) || !gsr_aligned4(total)) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_weight_total_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)W * H;
    const unsigned blocks = sum_blocks(n);
    float *part = reinterpret_cast<float *>(workspace);
    hipLaunchKernelGGL(weight_sum_kernel, dim3(blocks), dim3(NT), 0, s, weight, part, n);
    hipLaunchKernelGGL((gsr_finish_kernel<1, 1, 1>), dim3(1), dim3(NT), 0, s, (const float *)part, (int)blocks, GsrSumOut<1>{{total}});
    return gsr_done();
}

int gsr_weighted_l1_loss_grad(const float *rendered, const float *target, const float *weight, const float *weight_total, float *pixel_grad,
                              float *loss_sum, int32_t W, int32_t H, float scale, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rendered || !target || !weight || !weight_total || !loss_sum || !workspace) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H) || !(scale >= 0.0f && scale <= FLT_MAX)) return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(target) || !gsr_aligned16(weight) || !gsr_aligned16(pixel_grad) || !gsr_aligned16(workspace))
        return GSR_E_ALIGN;
    if (!gsr_aligned4(weight_total) || !gsr_aligned4(loss_sum)) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_weight_total_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)W * H;
    const unsigned blocks = sum_blocks(n);
    float *part = reinterpret_cast<float *>(workspace);
    hipLaunchKernelGGL(weighted_l1_kernel, dim3(blocks), dim3(NT), 0, s, rendered, target, weight, weight_total, pixel_grad, part, n, scale);
    hipLaunchKernelGGL((gsr_finish_kernel<1, 1, 1>), dim3(1), dim3(NT), 0, s, (const float *)part, (int)blocks, GsrSumOut<1>{{loss_sum}});
    return gsr_done();
}

size_t gsr_weighted_dssim_workspace_bytes(int32_t W, int32_t H) { return dssim_workspace_bytes(W, H); }

int gsr_weighted_l1_dssim_loss_grad(const float *rendered, const float *target, const float *weight, const float *weight_total, float *pixel_grad,
                                    float *l1_sum, float *ssim_sum, int32_t W, int32_t H, float lambda_dssim, int32_t window, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (!rendered || !target || !weight || !weight_total || !l1_sum || !ssim_sum || !workspace) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H) || !(lambda_dssim >= 0.0f && lambda_dssim <= 1.0f) || !window_ok(window)) return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(target) || !gsr_aligned16(weight) || !gsr_aligned16(pixel_grad) || !gsr_aligned16(workspace))
        return GSR_E_ALIGN;
    if (!gsr_aligned4(weight_total) || !gsr_aligned4(l1_sum) || !gsr_aligned4(ssim_sum)) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_weighted_dssim_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    return dssim_launch(rendered, target, weight, weight_total, pixel_grad, l1_sum, ssim_sum, W, H, lambda_dssim, window, workspace,
                        (hipStream_t)stream);
}

} // extern "C"
