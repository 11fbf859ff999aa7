// exposure.hip -- per-view exposure compensation (include/gsr_exposure.h): c' = c A + b on the rendered image, its backward with the
// 12 sums of dL/dE, and the Adam step of one view's 12 numbers.
//
// It sits beside train_ops.hip / dssim.hip, between the forward and the loss: launches of its own, no existing kernel touched.  Both
// image kernels are pure streams (apply 12 B in + 12 B out per pixel, backward 24 B in + 12 B out).  A pixel is 3 floats, so a lane
// takes 4 consecutive pixels = 12 floats = three 16-byte accesses, and reads all of them before it writes any, which is what lets
// `out` be `rendered` and `dL_drendered` be `dL_dout`.  The last W H % 4 pixels go one by one through the lane that owns them.  E is
// 12 wave-uniform values behind a __restrict__ pointer: they arrive through the scalar cache once per wave and live in SGPRs.
// Cache policy: default everywhere -- the render is read again by the backward, `out` by the loss kernel that follows, and
// dL_drendered by the backward blend (an 800 x 800 image is 7.7 MB: it stays in L2 / the Infinity Cache between the launches).
// The 12 sums never meet a float atomic: they are a fixed-order sum ("The fixed-order sum"; fixed_sum.h) with pairwise
// wave sums and one 64-byte record per workgroup in the workspace.
#include <math.h>

#include "fixed_sum.h"
#include "gsr_exposure.h"

namespace {

constexpr int NT = 256;                             // threads per workgroup
constexpr int GROUP = 4;                            // pixels per lane and round
constexpr int NE = GSR_EXPOSURE_FLOATS;
constexpr int REC = GSR_EXPOSURE_RECORD_BYTES / 4;  // floats per partial record
static_assert(NT * GROUP == GSR_EXPOSURE_BLOCK_PIXELS, "gsr_exposure.h states the pixels per workgroup and round");
static_assert(REC >= NE && GSR_EXPOSURE_RECORD_BYTES % 16 == 0, "a record holds the 12 sums in whole float4s");

struct Exposure {
    float a[3][3], b[3];
};
__device__ __forceinline__ Exposure load_exposure(const float *__restrict__ E)
{
    Exposure e;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) e.a[i][j] = E[3 * i + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) e.b[j] = E[9 + j];
    return e;
}

// c' = c A + b, summed i = 0, 1, 2, then + b (gsr_exposure.h)
__device__ __forceinline__ void apply_pixel(const Exposure &e, const float c[3], float o[3])
{
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = ((c[0] * e.a[0][j] + c[1] * e.a[1][j]) + c[2] * e.a[2][j]) + e.b[j];
}

// one pixel of the backward: dc = A g, and the pixel's 12 terms added to the lane's running sums
__device__ __forceinline__ void backward_pixel(const Exposure &e, const float c[3], const float g[3], float dc[3], float s[NE])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        dc[i] = (e.a[i][0] * g[0] + e.a[i][1] * g[1]) + e.a[i][2] * g[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) s[3 * i + j] += c[i] * g[j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[9 + j] += g[j];
}

__device__ __forceinline__ void ld12(const float *p, int64_t q, float *dst)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 v = reinterpret_cast<const float4 *>(p)[3 * q + k];
        dst[4 * k] = v.x, dst[4 * k + 1] = v.y, dst[4 * k + 2] = v.z, dst[4 * k + 3] = v.w;
    }
}
__device__ __forceinline__ void st12(float *p, int64_t q, const float *src)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) reinterpret_cast<float4 *>(p)[3 * q + k] = make_float4(src[4 * k], src[4 * k + 1], src[4 * k + 2], src[4 * k + 3]);
}

// `out` may be `rendered`: neither is __restrict__
__global__ __launch_bounds__(NT) void exposure_apply_kernel(int64_t P, const float *rendered, const float *__restrict__ E, float *out)
{
    const int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (GROUP * q >= P) return;
    const Exposure e = load_exposure(E);
    if (GROUP * q + GROUP <= P) {
        float c[3 * GROUP], o[3 * GROUP];
        ld12(rendered, q, c);
#pragma unroll
        for (int p = 0; p < GROUP; ++p) apply_pixel(e, c + 3 * p, o + 3 * p);
        st12(out, q, o);
        return;
    }
    for (int64_t i = GROUP * q; i < P; ++i) {
        const float c[3] = {rendered[3 * i], rendered[3 * i + 1], rendered[3 * i + 2]};
        float o[3];
        apply_pixel(e, c, o);
        out[3 * i] = o[0], out[3 * i + 1] = o[1], out[3 * i + 2] = o[2];
    }
}

// A fixed grid of at most GSR_EXPOSURE_MAX_BLOCKS workgroups walks the 4-pixel groups (`groups` = ceil(P / 4)); workgroup k leaves
// its sums in part[REC * k].  `dL_drendered` may be `dL_dout`: neither is __restrict__.
template <bool WRITE>
__global__ __launch_bounds__(NT) void exposure_backward_kernel(int64_t P, int64_t groups, const float *__restrict__ rendered, const float *__restrict__ E,
                                                               const float *dL_dout, float *dL_drendered, float *__restrict__ part)
{
    __shared__ float s_red[GSR_SUM_WAVES][NE];
    const Exposure e = load_exposure(E);
    float s[NE] = {};
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < groups; q += stride) {
        if (GROUP * q + GROUP <= P) {
            float c[3 * GROUP], g[3 * GROUP], dc[3 * GROUP];
            ld12(rendered, q, c);
            ld12(dL_dout, q, g);
#pragma unroll
            for (int p = 0; p < GROUP; ++p) backward_pixel(e, c + 3 * p, g + 3 * p, dc + 3 * p, s);
            if (WRITE) st12(dL_drendered, q, dc);
            continue;
        }
        for (int64_t i = GROUP * q; i < P; ++i) {
            const float c[3] = {rendered[3 * i], rendered[3 * i + 1], rendered[3 * i + 2]};
            const float g[3] = {dL_dout[3 * i], dL_dout[3 * i + 1], dL_dout[3 * i + 2]};
            float dc[3];
            backward_pixel(e, c, g, dc, s);
            if (WRITE) dL_drendered[3 * i] = dc[0], dL_drendered[3 * i + 1] = dc[1], dL_drendered[3 * i + 2] = dc[2];
        }
    }
    const GsrBlockSums<float, NE> b = gsr_block_sums<NT>(s, s_red);
    if (threadIdx.x < NE) part[(size_t)REC * blockIdx.x + threadIdx.x] = b.pairwise(threadIdx.x);
}

// one wave; lanes 0-11 own one element each
__global__ __launch_bounds__(GSR_WAVE) void exposure_adam_kernel(float *__restrict__ E, const float *__restrict__ dL_dE, float *__restrict__ m,
                                                                 float *__restrict__ v, float lr, float beta1, float beta2, float eps, float bc1, float bc2)
{
    const int k = threadIdx.x;
    if (k >= NE) return;
    const float g = dL_dE[k];
    const float mk = beta1 * m[k] + (1.0f - beta1) * g;
    const float vk = beta2 * v[k] + (1.0f - beta2) * (g * g);
    m[k] = mk, v[k] = vk;
    E[k] = E[k] - lr * ((mk / bc1) / (sqrtf(vk / bc2) + eps));
}

int64_t backward_blocks(int64_t P) { return gsr_record_count(P, GSR_EXPOSURE_BLOCK_PIXELS, GSR_EXPOSURE_MAX_BLOCKS); }

} // namespace

extern "C" {

size_t gsr_exposure_workspace_bytes(int32_t W, int32_t H)
{
    if (!gsr_image_dims_ok(W, H)) return 0;
    return gsr_align((size_t)GSR_EXPOSURE_RECORD_BYTES * (size_t)backward_blocks((int64_t)W * H));
}

int gsr_exposure_apply(const float *rendered, const float *E, float *out, int32_t W, int32_t H, void *stream)
{
    if (!rendered || !E || !out) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H)) return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(out) || !gsr_aligned4(E)) return GSR_E_ALIGN;
    const int64_t P = (int64_t)W * H;
    hipLaunchKernelGGL(exposure_apply_kernel, dim3((unsigned)gsr_div_up(gsr_div_up(P, GROUP), NT)), dim3(NT), 0, (hipStream_t)stream, P, rendered, E, out);
    return gsr_done();
}

int gsr_exposure_backward(const float *rendered, const float *E, const float *dL_dout, float *dL_drendered, float *dL_dE, int32_t W, int32_t H,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rendered || !E || !dL_dout || !dL_dE || !workspace) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H)) return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(dL_dout) || !gsr_aligned16(dL_drendered) || !gsr_aligned16(workspace) || !gsr_aligned4(E) ||
        !gsr_aligned4(dL_dE))
        return GSR_E_ALIGN;
    if (workspace_bytes < gsr_exposure_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    const int64_t P = (int64_t)W * H, groups = gsr_div_up(P, GROUP);
    const int nb = (int)backward_blocks(P);
    hipStream_t s = (hipStream_t)stream;
    float *part = static_cast<float *>(workspace);
    if (dL_drendered)
        hipLaunchKernelGGL(exposure_backward_kernel<true>, dim3(nb), dim3(NT), 0, s, P, groups, rendered, E, dL_dout, dL_drendered, part);
    else
        hipLaunchKernelGGL(exposure_backward_kernel<false>, dim3(nb), dim3(NT), 0, s, P, groups, rendered, E, dL_dout, (float *)nullptr, part);
    hipLaunchKernelGGL((gsr_finish_kernel<NE, REC, 1>), dim3(1), dim3(NT), 0, s, (const float *)part, nb, GsrSumOut<1>{{dL_dE}});
    return gsr_done();
}

int gsr_exposure_adam(float *E, const float *dL_dE, float *m, float *v, float lr, float beta1, float beta2, float eps, int32_t step, void *stream)
{
    if (!E || !dL_dE || !m || !v) return GSR_E_NULL;
    if (step < 1 || !(lr >= 0.0f) || !isfinite(lr) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps > 0.0f) ||
        !isfinite(eps))
        return GSR_E_DIMS;
    if (!gsr_aligned4(E) || !gsr_aligned4(dL_dE) || !gsr_aligned4(m) || !gsr_aligned4(v)) return GSR_E_ALIGN;
    // bias corrections in float32 on the host, as gsr_adam_update forms them
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
    hipLaunchKernelGGL(exposure_adam_kernel, dim3(1), dim3(GSR_WAVE), 0, (hipStream_t)stream, E, dL_dE, m, v, lr, beta1, beta2, eps, bc1, bc2);
    return gsr_done();
}

} // extern "C"
