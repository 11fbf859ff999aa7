// dssim_weighted.hip -- the colour loss under per-pixel weights m (include/gsr_weighted_loss.h has the formulas): the weighted twins
// of train_ops.hip's L1 kernel and of dssim.hip's three passes, over the same window code (dssim_window.h), tiles and LDS.
//   weight_sum_kernel            M = sum of m: one partial per workgroup, then weighted_finish_kernel<1>.
//   weighted_l1_kernel           m |x - y| and scale / (3 M) m sign(x - y), four pixels per thread; partials and finish likewise.
//   dssim_weighted_stats_kernel  dssim_stats_kernel plus one coalesced read of m at the output pixel (no halo: the weight multiplies
//                                the loss map, not the images): the planes hold m alpha, m beta, m gamma scaled by lambda / (3 M),
//                                the partials m |x - y| and m S.
//   dssim_weighted_adjoint_kernel  dssim_adjoint_kernel with the sign term times m_q.
//   weighted_finish_kernel<2>    the two sums, as dssim_finish_kernel.
// M arrives as a device float: every kernel that scales by it forms 1 / (3 M) itself, 0 when M = 0, so an all-zero mask gives zeros.
// A zero weight gives +0 whatever the sign of x - y, so what a masked region holds never shows in the bits of the gradient.
#include <float.h>
#include <math.h>

#include "dssim_window.h"
#include "gsr_weighted_loss.h"

namespace {

constexpr int MAX_SUM_BLOCKS = 512;   // two workgroups per CU, grid stride, as gsr_l1_loss_grad

__device__ __forceinline__ float inv_3m(const float *__restrict__ weight_total)
{
    const float M = *weight_total;
    return M > 0.0f ? 1.0f / (3.0f * M) : 0.0f;
}

// w sign(d) with sign(0) = +1, and +0 for w = 0
__device__ __forceinline__ float signed_weight(float w, float d) { return (d < 0.0f && w > 0.0f) ? -w : w; }

// workgroup sum of one per-thread value into part[blockIdx.x] (fixed order)
__device__ __forceinline__ void block_partial(float acc, float *__restrict__ part, float *s_red)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// ---- M: flat over the H * W weights, a float4 per lane ----
__global__ __launch_bounds__(NT) void weight_sum_kernel(const float *__restrict__ weight, float *__restrict__ part, int64_t n)
{
    __shared__ float s_red[4];
    float acc = 0.0f;
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
        const float4 m = reinterpret_cast<const float4 *>(weight)[i];
        acc += (m.x + m.y) + (m.z + m.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) acc += weight[(n4 << 2) + threadIdx.x];   // tail (< 4 pixels)
    block_partial(acc, part, s_red);
}

// ---- weighted L1: four pixels per thread (one float4 of weights, three of each image) ----
__global__ __launch_bounds__(NT) void weighted_l1_kernel(const float *__restrict__ rendered, const float *__restrict__ target,
                                                         const float *__restrict__ weight, const float *__restrict__ weight_total,
                                                         float *__restrict__ pixel_grad, float *__restrict__ part, int64_t n, float scale)
{
    __shared__ float s_red[4];
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
    block_partial(acc, part, s_red);
}

// ---- pass 1: dssim_stats_kernel with the loss map weighted ----
__global__ __launch_bounds__(NT) void dssim_weighted_stats_kernel(const float *__restrict__ rendered, const float *__restrict__ target,
                                                                  const float *__restrict__ weight, const float *__restrict__ weight_total,
                                                                  float *__restrict__ planes, float2 *__restrict__ part, int W, int H, DssimW k,
                                                                  float lambda, int want_grad)
{
    constexpr int SW = TX + 2 * RAD, SH = TY + 2 * RAD, P = 2;
    __shared__ float s_x[SW * SH], s_y[SW * SH], s_h[5 * SH * TX];
    __shared__ float s_red[8];
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
    const int u = threadIdx.x & (TX - 1), v0 = (threadIdx.x / TX) * P;   // this thread's two output pixels (u, v0), (u, v0 + 1)
    const int gx = tx0 + u;
    const size_t HW = (size_t)H * W;
    const float kscale = lambda * inv_3m(weight_total);
    float inv_wp[P], m[P];
    {
        const float sx = border_sum(k, gx, W);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int gy = ty0 + v0 + p;
            inv_wp[p] = 1.0f / (sx * border_sum(k, gy, H));
            m[p] = (gx < W && gy < H) ? weight[(size_t)gy * W + gx] : 0.0f;
        }
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
            ss += m[p] * ssim_terms(s, inv_wp[p], kscale, al, be, ga);
            const int li = (v0 + p + RAD) * SW + u + RAD;
            l1 += m[p] * fabsf(s_x[li] - s_y[li]);
            if (want_grad) {
                const size_t g = (size_t)gy * W + gx;
                planes[(3 * c + 0) * HW + g] = m[p] * al;
                planes[(3 * c + 1) * HW + g] = m[p] * be;
                planes[(3 * c + 2) * HW + g] = m[p] * ga;
            }
        }
        __syncthreads();   // s_x / s_y / s_h are restaged for the next channel
    }
    block_partials(l1, ss / 3.0f, part, s_red);
}

// ---- pass 2: dssim_adjoint_kernel with the sign term times m_q ----
__global__ __launch_bounds__(NT) void dssim_weighted_adjoint_kernel(const float *__restrict__ rendered, const float *__restrict__ target,
                                                                    const float *__restrict__ weight, const float *__restrict__ weight_total,
                                                                    const float *__restrict__ planes, float *__restrict__ pixel_grad, int W,
                                                                    int H, DssimW k, float l1_scale)
{
    constexpr int SW = TX + 2 * RAD, SH = TY + 2 * RAD, P = 2;
    __shared__ float s_a[3 * SW * SH], s_h[3 * SH * TX];
    const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
    const int u = threadIdx.x & (TX - 1), v0 = (threadIdx.x / TX) * P;
    const int gx = tx0 + u;
    const size_t HW = (size_t)H * W;
    const float l1c = l1_scale * inv_3m(weight_total);
    float l1w[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int gy = ty0 + v0 + p;
        l1w[p] = (gx < W && gy < H) ? l1c * weight[(size_t)gy * W + gx] : 0.0f;
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
            g[p][c] = signed_weight(l1w[p], x - y) - adj;
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

// ---- the sums: one workgroup adds n partial records of NV floats in a fixed order into NV caller words ----
template <int NV>
__global__ __launch_bounds__(NT) void weighted_finish_kernel(const float *__restrict__ part, int n, float *__restrict__ out0,
                                                             float *__restrict__ out1)
{
    __shared__ float s_red[4 * NV];
    float acc[NV] = {};
    for (int i = threadIdx.x; i < n; i += NT)
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] += part[NV * i + v];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[v] += __shfl_xor(acc[v], d, 64);
        if ((threadIdx.x & 63) == 0) s_red[4 * v + (threadIdx.x >> 6)] = acc[v];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *out0 = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        if constexpr (NV > 1) *out1 = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
    }
}

bool dims_ok(int32_t W, int32_t H) { return W > 0 && H > 0 && (int64_t)W * H <= MAX_PIXELS; }
bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }   // single floats: any slot of a float array
unsigned sum_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(MAX_SUM_BLOCKS, gsr_div_up(gsr_div_up(n, 4), NT))); }

} // namespace

extern "C" {

size_t gsr_weight_total_workspace_bytes(int32_t W, int32_t H)
{
    return dims_ok(W, H) ? gsr_align(sizeof(float) * sum_blocks((int64_t)W * H)) : 0;
}

int gsr_weight_total(const float *weight, int32_t W, int32_t H, float *total, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!weight || !total || !workspace) return GSR_E_NULL;
    if (!dims_ok(W, H)) return GSR_E_DIMS;
    if (!gsr_aligned16(weight) || !gsr_aligned16(workspace) || !aligned4(total)) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_weight_total_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)W * H;
    const unsigned blocks = sum_blocks(n);
    float *part = reinterpret_cast<float *>(workspace);
    hipLaunchKernelGGL(weight_sum_kernel, dim3(blocks), dim3(NT), 0, s, weight, part, n);
    hipLaunchKernelGGL(weighted_finish_kernel<1>, dim3(1), dim3(NT), 0, s, part, (int)blocks, total, (float *)nullptr);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_E_HIP;
}

int gsr_weighted_l1_loss_grad(const float *rendered, const float *target, const float *weight, const float *weight_total, float *pixel_grad,
                              float *loss_sum, int32_t W, int32_t H, float scale, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rendered || !target || !weight || !weight_total || !loss_sum || !workspace) return GSR_E_NULL;
    if (!dims_ok(W, H) || !(scale >= 0.0f && scale <= FLT_MAX)) return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(target) || !gsr_aligned16(weight) || !gsr_aligned16(pixel_grad) || !gsr_aligned16(workspace))
        return GSR_E_ALIGN;
    if (!aligned4(weight_total) || !aligned4(loss_sum)) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_weight_total_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)W * H;
    const unsigned blocks = sum_blocks(n);
    float *part = reinterpret_cast<float *>(workspace);
    hipLaunchKernelGGL(weighted_l1_kernel, dim3(blocks), dim3(NT), 0, s, rendered, target, weight, weight_total, pixel_grad, part, n, scale);
    hipLaunchKernelGGL(weighted_finish_kernel<1>, dim3(1), dim3(NT), 0, s, part, (int)blocks, loss_sum, (float *)nullptr);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_E_HIP;
}

size_t gsr_weighted_dssim_workspace_bytes(int32_t W, int32_t H) { return dssim_workspace_bytes(W, H); }

int gsr_weighted_l1_dssim_loss_grad(const float *rendered, const float *target, const float *weight, const float *weight_total, float *pixel_grad,
                                    float *l1_sum, float *ssim_sum, int32_t W, int32_t H, float lambda_dssim, int32_t window, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (!rendered || !target || !weight || !weight_total || !l1_sum || !ssim_sum || !workspace) return GSR_E_NULL;
    if (!dims_ok(W, H) || !(lambda_dssim >= 0.0f && lambda_dssim <= 1.0f) ||
        (window != GSR_SSIM_WINDOW_REFERENCE && window != GSR_SSIM_WINDOW_GAUSSIAN))
        return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(target) || !gsr_aligned16(weight) || !gsr_aligned16(pixel_grad) || !gsr_aligned16(workspace))
        return GSR_E_ALIGN;
    if (!aligned4(weight_total) || !aligned4(l1_sum) || !aligned4(ssim_sum)) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_weighted_dssim_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    const DssimW k = window_taps(window == GSR_SSIM_WINDOW_REFERENCE);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)gsr_div_up(W, TX), (unsigned)gsr_div_up(H, TY));
    float2 *part = reinterpret_cast<float2 *>(workspace);
    float *planes = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + partial_bytes(W, H));
    hipLaunchKernelGGL(dssim_weighted_stats_kernel, grid, dim3(NT), 0, s, rendered, target, weight, weight_total, planes, part, W, H, k,
                       lambda_dssim, pixel_grad != nullptr);
    if (pixel_grad)
        hipLaunchKernelGGL(dssim_weighted_adjoint_kernel, grid, dim3(NT), 0, s, rendered, target, weight, weight_total, planes, pixel_grad, W, H,
                           k, 1.0f - lambda_dssim);
    hipLaunchKernelGGL(weighted_finish_kernel<2>, dim3(1), dim3(NT), 0, s, reinterpret_cast<const float *>(part), (int)(grid.x * grid.y), l1_sum,
                       ssim_sum);
    return hipGetLastError() == hipSuccess ? GSR_OK : GSR_E_HIP;
}

} // extern "C"
