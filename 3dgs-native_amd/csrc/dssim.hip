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

#include "gsr_internal.h"
#include "gsr_loss.h"

namespace {

constexpr int RAD = 5;                 // window radius: 11 taps
constexpr int TX = 32, TY = 16, NT = 256;
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

struct DssimW { float w[RAD + 1]; };   // weight by tap distance 0..5

// sum of the weights of the taps of a window centred on i that fall inside [0, n): Sx(i) or Sy(j)
__device__ __forceinline__ float border_sum(const DssimW &k, int i, int n)
{
    float s = 0.0f;
#pragma unroll
    for (int d = -RAD; d <= RAD; ++d)
        if (i + d >= 0 && i + d < n) s += k.w[d < 0 ? -d : d];
    return s;
}

// s[ly * SW + lx] = src[stride * ((oy + ly) * W + ox + lx) + c], 0 outside the image (a zero tap adds nothing to a window sum)
template <int SW, int SH>
__device__ __forceinline__ void stage(const float *__restrict__ src, int stride, int c, int ox, int oy, int W, int H, float *s)
{
    for (int k = threadIdx.x; k < SW * SH; k += NT) {
        const int ly = k / SW, lx = k - ly * SW, x = ox + lx, y = oy + ly;
        s[k] = (x >= 0 && x < W && y >= 0 && y < H) ? src[(size_t)stride * ((size_t)y * W + x) + c] : 0.0f;
    }
}

// Horizontal window sums of x, y, x^2, y^2, xy: hs[q][r][u] = sum_d w(|d - 5|) f_q[r][u + d], d = 0..10, for r < SH, u < SW - 10.
// P neighbouring outputs per item share their 10 + P loads.
template <int SW, int SH, int P>
__device__ __forceinline__ void hsum_stats(const float *sx, const float *sy, float *hs, const DssimW &k)
{
    constexpr int OW = SW - 2 * RAD, G = OW / P;
    static_assert(OW % P == 0, "tile width");
    for (int it = threadIdx.x; it < SH * G; it += NT) {
        const int r = it / G, u0 = (it - r * G) * P;
        float acc[5][P];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int p = 0; p < P; ++p) acc[q][p] = 0.0f;
#pragma unroll
        for (int t = 0; t < 2 * RAD + P; ++t) {
            const float x = sx[r * SW + u0 + t], y = sy[r * SW + u0 + t];
            const float xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int d = t - p;
                if (d < 0 || d > 2 * RAD) continue;
                const float w = k.w[d < RAD ? RAD - d : d - RAD];
                acc[0][p] = fmaf(w, x, acc[0][p]);
                acc[1][p] = fmaf(w, y, acc[1][p]);
                acc[2][p] = fmaf(w, xx, acc[2][p]);
                acc[3][p] = fmaf(w, yy, acc[3][p]);
                acc[4][p] = fmaf(w, xy, acc[4][p]);
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int p = 0; p < P; ++p) hs[(q * SH + r) * OW + u0 + p] = acc[q][p];
    }
}

// Horizontal window sums of three planes a[q][r][*] (SW wide, SH rows) into hs[q][r][u], u < SW - 10
template <int SW, int SH, int P>
__device__ __forceinline__ void hsum3(const float *a, float *hs, const DssimW &k)
{
    constexpr int OW = SW - 2 * RAD, G = OW / P;
    static_assert(OW % P == 0, "tile width");
    for (int it = threadIdx.x; it < SH * G; it += NT) {
        const int r = it / G, u0 = (it - r * G) * P;
        float acc[3][P];
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int p = 0; p < P; ++p) acc[q][p] = 0.0f;
#pragma unroll
        for (int t = 0; t < 2 * RAD + P; ++t) {
            float v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = a[(q * SH + r) * SW + u0 + t];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int d = t - p;
                if (d < 0 || d > 2 * RAD) continue;
                const float w = k.w[d < RAD ? RAD - d : d - RAD];
#pragma unroll
                for (int q = 0; q < 3; ++q) acc[q][p] = fmaf(w, v[q], acc[q][p]);
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int p = 0; p < P; ++p) hs[(q * SH + r) * OW + u0 + p] = acc[q][p];
    }
}

// Vertical window sums at column u, rows v0 .. v0 + P - 1 of the output: acc[q][p] = sum_d w(|d - 5|) hs[q][v0 + p + d][u]
template <int NQ, int OW, int SH, int P>
__device__ __forceinline__ void vsum(const float *hs, int u, int v0, const DssimW &k, float (&acc)[NQ][P])
{
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int p = 0; p < P; ++p) acc[q][p] = 0.0f;
#pragma unroll
    for (int t = 0; t < 2 * RAD + P; ++t) {
        float v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = hs[(q * SH + v0 + t) * OW + u];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int d = t - p;
            if (d < 0 || d > 2 * RAD) continue;
            const float w = k.w[d < RAD ? RAD - d : d - RAD];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q][p] = fmaf(w, v[q], acc[q][p]);
        }
    }
}

// S of one channel at one pixel from its five window sums and 1 / Wp, and the adjoint weights scaled by kscale / Wp.
// dS/de12 = 2S/B and S * 2m2/A are formed as 2A/(CD) and 2m2 B/(CD): nothing divides by A or B, which may be 0.
__device__ __forceinline__ float ssim_terms(const float (&s)[5], float inv_wp, float kscale, float &al, float &be, float &ga)
{
    const float m1 = s[0] * inv_wp, m2 = s[1] * inv_wp, e11 = s[2] * inv_wp, e22 = s[3] * inv_wp, e12 = s[4] * inv_wp;
    const float m12 = m1 * m2, m11 = m1 * m1, m22 = m2 * m2;
    const float A = 2.0f * m12 + C1, B = 2.0f * (e12 - m12) + C2, C = m11 + m22 + C1, D = (e11 - m11) + (e22 - m22) + C2;
    const float inv_cd = 1.0f / (C * D);
    const float S = A * B * inv_cd;
    const float inv_c = 1.0f / C, inv_d = 1.0f / D;
    const float dm1 = 2.0f * (m2 * (B - A) * inv_cd + m1 * S * (inv_d - inv_c));
    const float f = kscale * inv_wp;
    al = f * dm1;
    be = f * (-S * inv_d);
    ga = f * (2.0f * A * inv_cd);
    return S;
}

// workgroup sums of two per-thread values into part[blockIdx] (fixed order: the same bits every call)
__device__ __forceinline__ void block_partials(float l1, float ss, float2 *part, float *s_red)
{
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
    if (threadIdx.x == 0)
        part[blockIdx.y * gridDim.x + blockIdx.x] = make_float2((s_red[0] + s_red[1]) + (s_red[2] + s_red[3]),
                                                                (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]));
}

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

constexpr int64_t MAX_PIXELS = (int64_t)1 << 28;

// workspace: [partials: one float2 per workgroup, padded to 256 bytes] [9 planes of W * H floats: alpha, beta, gamma per channel]
size_t partial_bytes(int32_t W, int32_t H) { return gsr_align(sizeof(float2) * (size_t)gsr_div_up(W, TX) * (size_t)gsr_div_up(H, TY)); }

} // namespace

extern "C" {

size_t gsr_dssim_workspace_bytes(int32_t W, int32_t H)
{
    if (W <= 0 || H <= 0 || (int64_t)W * H > MAX_PIXELS) return 0;
    return gsr_align(partial_bytes(W, H) + 9 * sizeof(float) * (size_t)W * H);
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
    DssimW k;   // sigma = 1.5 as loss.py:33-45; the reference window indexes the Gaussian centred on 5 by distance (Q21)
    for (int d = 0; d <= RAD; ++d) {
        const int x = window == GSR_SSIM_WINDOW_REFERENCE ? d - RAD : d;
        k.w[d] = expf(-1.0f * (float)(x * x) / (2.0f * 1.5f * 1.5f));
    }
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
