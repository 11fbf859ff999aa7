// filter3d.hip -- the 3D smoothing filter of Mip-Splatting (include/gsr_filter3d.h): each Gaussian's sampling rate from the training
// views, the map (scales, opacity, filter_3d) -> (s', opacity') the rasterizer then runs on, and that map's transpose.
//
// It sits beside preprocess_kernel / geom_backward_kernel, not inside them: three short launches of its own, no existing kernel
// touched.  from_views is one lane per Gaussian with a loop over the views, whose 80-byte records are indexed by the loop counter
// alone -- wave-uniform, so they arrive through the scalar cache once per wave -- and is the only arithmetic here.  apply and backward
// are pure streams (36 and 52 bytes per Gaussian); a lane takes four Gaussians, so every access is a 16-byte vector, and reads all
// of its rows before it writes any, which is what lets the backward run in place in a gradient arena.
#include <math.h>

#include "gsr_filter3d.h"
#include "gsr_internal.h"

namespace {

constexpr uint32_t NO_NU = 0xFFFFFFFFu; // "no view saw anything": above the bits of every positive float

// nu per Gaussian (0 = unseen) into nu_out, and the smallest positive nu of the launch into *min_bits as uint bits: positive floats
// order like their bit patterns (the idiom of scan_sort.hip's depth extremes).  A wave reduction, then at most one vector atomic per
// wave: a wave first loads the word and skips the atomic when its own minimum cannot lower it.  The word only ever falls, so a value
// read early (or stale) is no smaller than the final one and the skip never loses a minimum; the result is the same bits.  Without
// the load, 15 625 atomics onto the one address serialise at 1 M Gaussians: 181 us for the kernel against 19 (profiles/filter3d/).
__global__ __launch_bounds__(256) void filter3d_nu_kernel(int64_t N, const float *__restrict__ means, int V, const GsrFilterView *__restrict__ views,
                                                          float *__restrict__ nu_out, uint32_t *__restrict__ min_bits)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = t < N;
    const int64_t i = in_range ? t : N - 1; // tail lanes redo the last Gaussian and store nothing (they stay in the wave reduction)
    const float px = means[3 * i], py = means[3 * i + 1], pz = means[3 * i + 2];
    float nu = 0.0f;
    for (int v = 0; v < V; ++v) {
        const GsrFilterView &c = views[v];
        // (p, 1) * view, rows accumulated in ascending order: preprocess.hip's rowvec_mul44, columns 0-2
        float x = c.view[0] * px, y = c.view[1] * px, z = c.view[2] * px;
        x += c.view[4] * py, y += c.view[5] * py, z += c.view[6] * py;
        x += c.view[8] * pz, y += c.view[9] * pz, z += c.view[10] * pz;
        x += c.view[12] * 1.0f, y += c.view[13] * 1.0f, z += c.view[14] * 1.0f;
        const float lim_x = (1.0f + GSR_FILTER3D_MARGIN) * (0.5f * (float)c.W), lim_y = (1.0f + GSR_FILTER3D_MARGIN) * (0.5f * (float)c.H);
        // |x / z * focal| <= lim with z > 0, without the division
        if (z > GSR_FILTER3D_NEAR && fabsf(x) * c.focal <= lim_x * z && fabsf(y) * c.focal <= lim_y * z) nu = fmaxf(nu, c.focal / z);
    }
    if (in_range) nu_out[t] = nu;
    uint32_t bits = (in_range && nu > 0.0f) ? __float_as_uint(nu) : NO_NU;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bits = min(bits, (uint32_t)__shfl_xor((int)bits, d, 64));
    if ((threadIdx.x & 63) == 0 && bits != NO_NU && bits < __hip_atomic_load(min_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(min_bits, bits);
}

// nu -> filter_3d = sqrt(variance) / nu, the unseen taking the smallest seen nu; zeros if no view saw anything
__global__ __launch_bounds__(256) void filter3d_finish_kernel(int64_t N, float *__restrict__ filter_3d, const uint32_t *__restrict__ min_bits, float sqrt_variance)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t bits = *min_bits;
    float nu = filter_3d[i];
    if (!(nu > 0.0f)) nu = __uint_as_float(bits);
    filter_3d[i] = bits == NO_NU ? 0.0f : sqrt_variance / nu;
}

// one Gaussian of the map: s'_k = sqrt(s_k^2 + f^2), opacity' = opacity * r_x r_y r_z with r_k = |s_k| / s'_k; f == 0 copies
__device__ __forceinline__ void apply_row(const float s[3], float o, float f, float so[3], float &oo)
{
    if (f == 0.0f) {
        so[0] = s[0], so[1] = s[1], so[2] = s[2], oo = o;
        return;
    }
    const float ff = f * f;
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        so[k] = sqrtf(s[k] * s[k] + ff);
        r[k] = fabsf(s[k]) / so[k];
    }
    oo = o * ((r[0] * r[1]) * r[2]);
}

// one Gaussian of the transpose (gsr_filter3d.h): gs / go are dL/d(s', opacity') on entry and dL/d(s, opacity) on return
__device__ __forceinline__ void backward_row(const float s[3], float o, float f, float gs[3], float &go)
{
    if (f == 0.0f) return;
    const float ff = f * f;
    float sp[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sp[k] = sqrtf(s[k] * s[k] + ff);
        r[k] = fabsf(s[k]) / sp[k];
    }
    const float go_o = go * o;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sign = (float)((s[k] > 0.0f) - (s[k] < 0.0f));
        const float q = f / sp[k];
        const float others = r[(k + 1) % 3] * r[(k + 2) % 3];
        gs[k] = gs[k] * (s[k] / sp[k]) + ((go_o * sign) * others) * ((q * q) / sp[k]); // f^2 / s'^3 as (f / s')^2 / s': no overflow of s'^3
    }
    go = go * ((r[0] * r[1]) * r[2]);
}

// Four Gaussians per lane: 3 + 1 + 1 (+ 3 + 1) float4 loads, then 3 + 1 float4 stores.  The last N % 4 rows go one by one through
// the lane that owns them.  Outputs may alias inputs row for row, so they are not __restrict__.
template <bool BACKWARD>
__global__ __launch_bounds__(256) void filter3d_map_kernel(int64_t N, const float *scales, const float *opacity, const float *__restrict__ filter_3d,
                                                           const float *g_scale_in, const float *g_opacity_in, float *out_scale, float *out_opacity)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i0 = 4 * q;
    if (i0 >= N) return;
    if (i0 + 4 <= N) {
        float s[12], o[4], f[4], gs[12], go[4];
        const auto ld = [](const float *p, int64_t idx, float *dst) {
            const float4 v = reinterpret_cast<const float4 *>(p)[idx];
            dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
        };
        const auto st = [](float *p, int64_t idx, const float *src) { reinterpret_cast<float4 *>(p)[idx] = make_float4(src[0], src[1], src[2], src[3]); };
#pragma unroll
        for (int j = 0; j < 3; ++j) ld(scales, 3 * q + j, s + 4 * j);
        ld(opacity, q, o);
        ld(filter_3d, q, f);
        if (BACKWARD) {
#pragma unroll
            for (int j = 0; j < 3; ++j) ld(g_scale_in, 3 * q + j, gs + 4 * j);
            ld(g_opacity_in, q, go);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (BACKWARD)
                backward_row(s + 3 * j, o[j], f[j], gs + 3 * j, go[j]);
            else
                apply_row(s + 3 * j, o[j], f[j], gs + 3 * j, go[j]);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) st(out_scale, 3 * q + j, gs + 4 * j);
        st(out_opacity, q, go);
        return;
    }
    for (int64_t i = i0; i < N; ++i) {
        const float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
        float gs[3], go;
        if (BACKWARD) {
            gs[0] = g_scale_in[3 * i], gs[1] = g_scale_in[3 * i + 1], gs[2] = g_scale_in[3 * i + 2], go = g_opacity_in[i];
            backward_row(s, opacity[i], filter_3d[i], gs, go);
        } else {
            apply_row(s, opacity[i], filter_3d[i], gs, go);
        }
        out_scale[3 * i] = gs[0], out_scale[3 * i + 1] = gs[1], out_scale[3 * i + 2] = gs[2], out_opacity[i] = go;
    }
}

constexpr int64_t MAX_ROWS = ((int64_t)1 << 31) - 1;
constexpr size_t WS_BYTES = 256; // one uint32, the smallest positive nu

} // namespace

extern "C" {

size_t gsr_filter3d_workspace_bytes(int64_t N)
{
    (void)N;
    return WS_BYTES;
}

int gsr_filter3d_from_views(int64_t N, const float *means, int32_t V, const GsrFilterView *views, float variance, float *filter_3d, void *ws,
                            size_t ws_bytes, void *stream)
{
    if (N > 0 && (!means || !filter_3d || (V > 0 && !views))) return GSR_E_NULL;
    if (N < 0 || N > MAX_ROWS || V < 0 || !(variance > 0.0f) || !isfinite(variance)) return GSR_E_DIMS;
    if (N == 0) return GSR_OK;
    if (!gsr_aligned16(means) || !gsr_aligned16(views) || !gsr_aligned16(filter_3d) || !gsr_aligned16(ws)) return GSR_E_ALIGN;
    if (!ws || ws_bytes < WS_BYTES) return GSR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *min_bits = static_cast<uint32_t *>(ws);
    if (hipMemsetAsync(min_bits, 0xFF, sizeof(uint32_t), s) != hipSuccess) return GSR_E_HIP;
    const dim3 grid((unsigned)gsr_div_up(N, 256));
    hipLaunchKernelGGL(filter3d_nu_kernel, grid, dim3(256), 0, s, N, means, (int)V, views, filter_3d, min_bits);
    hipLaunchKernelGGL(filter3d_finish_kernel, grid, dim3(256), 0, s, N, filter_3d, min_bits, sqrtf(variance));
    return gsr_done();
}

int gsr_filter3d_apply(int64_t N, const float *scales, const float *opacity, const float *filter_3d, float *scales_out, float *opacity_out,
                       void *stream)
{
    if (N > 0 && (!scales || !opacity || !filter_3d || !scales_out || !opacity_out)) return GSR_E_NULL;
    if (N < 0 || N > MAX_ROWS) return GSR_E_DIMS;
    if (N == 0) return GSR_OK;
    if (!gsr_aligned16(scales) || !gsr_aligned16(opacity) || !gsr_aligned16(filter_3d) || !gsr_aligned16(scales_out) || !gsr_aligned16(opacity_out))
        return GSR_E_ALIGN;
    hipLaunchKernelGGL(filter3d_map_kernel<false>, dim3((unsigned)gsr_div_up(gsr_div_up(N, 4), 256)), dim3(256), 0, (hipStream_t)stream, N, scales,
                       opacity, filter_3d, (const float *)nullptr, (const float *)nullptr, scales_out, opacity_out);
    return gsr_done();
}

int gsr_filter3d_backward(int64_t N, const float *scales, const float *opacity, const float *filter_3d, const float *dL_dscale_f,
                          const float *dL_dopacity_f, float *dL_dscale, float *dL_dopacity, void *stream)
{
    if (N > 0 && (!scales || !opacity || !filter_3d || !dL_dscale_f || !dL_dopacity_f || !dL_dscale || !dL_dopacity)) return GSR_E_NULL;
    if (N < 0 || N > MAX_ROWS) return GSR_E_DIMS;
    if (N == 0) return GSR_OK;
    if (!gsr_aligned16(scales) || !gsr_aligned16(opacity) || !gsr_aligned16(filter_3d) || !gsr_aligned16(dL_dscale_f) || !gsr_aligned16(dL_dopacity_f) ||
        !gsr_aligned16(dL_dscale) || !gsr_aligned16(dL_dopacity))
        return GSR_E_ALIGN;
    hipLaunchKernelGGL(filter3d_map_kernel<true>, dim3((unsigned)gsr_div_up(gsr_div_up(N, 4), 256)), dim3(256), 0, (hipStream_t)stream, N, scales,
                       opacity, filter_3d, dL_dscale_f, dL_dopacity_f, dL_dscale, dL_dopacity);
    return gsr_done();
}

} // extern "C"
