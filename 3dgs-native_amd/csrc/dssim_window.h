// dssim_window.h -- the separable 11-tap window of the D-SSIM kernels: tile staging, horizontal and vertical window sums, S and
// its adjoint weights at one pixel.  Used by dssim.hip (not part of the C ABI); everything sits in the including file's anonymous
// namespace.
#pragma once
#include <math.h>

#include "gsr_internal.h"

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

// the taps by distance 0..5, sigma = 1.5 as loss.py:33-45; the reference window indexes the Gaussian centred on 5 by distance (Q21)
inline DssimW window_taps(bool reference)
{
    DssimW k;
    for (int d = 0; d <= RAD; ++d) {
        const int x = reference ? d - RAD : d;
        k.w[d] = expf(-1.0f * (float)(x * x) / (2.0f * 1.5f * 1.5f));
    }
    return k;
}

// workspace: [partials: one float2 per workgroup, padded to 256 bytes] [9 planes of W * H floats: alpha, beta, gamma per channel]
inline size_t partial_bytes(int32_t W, int32_t H) { return gsr_align(sizeof(float2) * (size_t)gsr_div_up(W, TX) * (size_t)gsr_div_up(H, TY)); }
inline size_t dssim_workspace_bytes(int32_t W, int32_t H)
{
    if (!gsr_image_dims_ok(W, H)) return 0;
    return gsr_align(partial_bytes(W, H) + 9 * sizeof(float) * (size_t)W * H);
}

} // namespace
