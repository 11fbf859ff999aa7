// depth_corr.hip -- the Pearson-correlation depth loss (include/gsr_depth_corr.h): loss = 1 - rho(rendered inverse depth, target), its
// exact pixel gradient and the least-squares fit of the target onto the render, for depth priors known up to scale and shift.
//
// It sits beside train_ops.hip's masked L1 (gsr_depth_loss_grad), between the forward and the backward: launches of its own, no
// existing kernel touched.  Three launches on the caller's stream, no host wait, no float atomics:
//   depth_corr_sums_kernel    a fixed grid of at most GSR_DEPTH_CORR_MAX_BLOCKS workgroups walks the image, 4 consecutive pixels per lane
//                             and round as one 16-byte load per image, and leaves the six float64 sums of its pixels in one 64-byte
//                             record (a fixed-order sum in float64 with pairwise wave sums: DESIGN.md, "The fixed-order sum"; fixed_sum.h).
//   depth_corr_finish_kernel  one workgroup adds the records in a fixed order, forms the moments, the degeneracy test, rho, loss and
//                             fit in float64, and leaves (mu_r, mu_t, k1, k2, degenerate) in the record behind the partial ones.
//   depth_corr_grad_kernel    one 4-pixel group per lane: grad = float(k1 m ((t - mu_t) - k2 (r - mu_r))), the centring in float64.
// The finishing pass is a launch of its own.  Folded into the gradient kernel, every one of its workgroups (625 at 800 x 800) would
// have to add all the records (40 KB there, 64 KB from 1 M pixels up) before its first pixel: 25-40 MB of L2 reads in front of a
// pass that moves 10 MB, or a last-workgroup ticket inside the sums kernel plus a grid-wide wait in front of the gradient.  One
// small launch costs less than either and keeps loss-only calls (grad == NULL) at two launches.
// Why float64: with r = 5 + 1e-3 noise a one-pass float32 sum r^2 / M - mu^2 returns 1.9e-6 for a variance of 1.0e-6, and centring a
// pixel in float32 against a float32 mean costs 600 eps32 of the spread.  In float64 the raw moments lose 1e-16 / (Vr / E[r^2]) =
// 2.5e-9 of the variance there, a fiftieth of eps32.  The work is 12 float64 operations per pixel under 8-12 bytes of loads: the
// kernels stay bound by memory.
// Cache policy: the sums pass reads r, t and m with the default policy -- the gradient pass reads them again a few microseconds
// later (an 800 x 800 call holds 7.7 MB: L2 / the Infinity Cache) -- and the gradient pass reads them non-temporally, their last use
// in the step; grad is stored with the default policy, the backward blend reads it next.
#include <math.h>

#include "fixed_sum.h"
#include "gsr_depth_corr.h"
#include "sh_stage.h"

namespace {

constexpr int NT = 256;                               // threads per workgroup
constexpr int GROUP = 4;                              // pixels per lane and round
constexpr int NS = 6;                                 // the sums: m, m r, m t, m r^2, m t^2, m r t
constexpr int REC = GSR_DEPTH_CORR_RECORD_BYTES / 8;  // float64s per record
static_assert(NT * GROUP == GSR_DEPTH_CORR_BLOCK_PIXELS, "gsr_depth_corr.h states the pixels per workgroup and round");
static_assert(REC >= NS && GSR_DEPTH_CORR_RECORD_BYTES % 16 == 0, "a record holds the six sums in whole 16-byte units");
// the record the finishing launch leaves for the gradient pass
enum { ST_MU_R = 0, ST_MU_T = 1, ST_K1 = 2, ST_K2 = 3, ST_DEGENERATE = 4 };

// one pixel's terms onto the lane's running sums, in this order
__device__ __forceinline__ void add_pixel(float rf, float tf, float mf, double s[NS])
{
    const double r = (double)rf, t = (double)tf, m = (double)mf;
    const double mr = m * r, mt = m * t;
    s[0] += m;
    s[1] += mr;
    s[2] += mt;
    s[3] += mr * r;
    s[4] += mt * t;
    s[5] += mr * t;
}

// workgroup k leaves its six sums in part[REC * k]; `groups` = ceil(P / 4)
template <bool MASK>
__global__ __launch_bounds__(NT) void depth_corr_sums_kernel(int64_t P, int64_t groups, const float *__restrict__ rendered, const float *__restrict__ target,
                                                             const float *__restrict__ mask, double *__restrict__ part)
{
    __shared__ double s_red[GSR_SUM_WAVES][NS];
    double s[NS] = {};
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < groups; q += stride) {
        if (GROUP * q + GROUP <= P) {
            const float4 r = reinterpret_cast<const float4 *>(rendered)[q], t = reinterpret_cast<const float4 *>(target)[q];
            const float4 m = MASK ? reinterpret_cast<const float4 *>(mask)[q] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            add_pixel(r.x, t.x, m.x, s);
            add_pixel(r.y, t.y, m.y, s);
            add_pixel(r.z, t.z, m.z, s);
            add_pixel(r.w, t.w, m.w, s);
            continue;
        }
        for (int64_t i = GROUP * q; i < P; ++i) add_pixel(rendered[i], target[i], MASK ? mask[i] : 1.0f, s);
    }
    const GsrBlockSums<double, NS> b = gsr_block_sums<NT>(s, s_red);
    if (threadIdx.x < NS) part[(size_t)REC * blockIdx.x + threadIdx.x] = b.pairwise(threadIdx.x);
}

// one workgroup: the record walk, then the same tree; thread 0 forms the results
__global__ __launch_bounds__(NT) void depth_corr_finish_kernel(const double *__restrict__ part, int n, float weight, float *__restrict__ loss,
                                                               float *__restrict__ fit /* may be NULL */, double *__restrict__ stats)
{
    __shared__ double s_red[GSR_SUM_WAVES][NS];
    GsrLaneSums<double, NS> s = gsr_record_walk<NS, REC>(part, n);
    const GsrBlockSums<double, NS> b = gsr_block_sums<NT>(s.v, s_red);
    if (threadIdx.x != 0) return;
    const double M = b.pairwise(0);
    double mu_r = 0.0, mu_t = 0.0, k1 = 0.0, k2 = 0.0, rho = 0.0, sc = 0.0, off = 0.0;
    bool ok = M > 0.0;
    if (ok) {
        mu_r = b.pairwise(1) / M, mu_t = b.pairwise(2) / M;
        const double err2 = b.pairwise(3) / M, ett2 = b.pairwise(4) / M;
        const double Vr = err2 - mu_r * mu_r, Vt = ett2 - mu_t * mu_t, C = b.pairwise(5) / M - mu_r * mu_t;
        ok = Vr > GSR_DEPTH_CORR_MIN_REL_VAR * err2 && Vt > GSR_DEPTH_CORR_MIN_REL_VAR * ett2;   // (false for a NaN too)
        if (ok) {
            const double sd = sqrt(Vr * Vt);
            rho = C / sd;
            sc = C / Vt, off = mu_r - sc * mu_t;
            k1 = -(double)weight / (M * sd), k2 = C / Vr;
        }
    }
    if (!ok) mu_r = mu_t = 0.0;
    loss[0] = (float)(1.0 - rho);
    if (fit) fit[0] = (float)rho, fit[1] = (float)sc, fit[2] = (float)off, fit[3] = (float)M;
    stats[ST_MU_R] = mu_r, stats[ST_MU_T] = mu_t, stats[ST_K1] = k1, stats[ST_K2] = k2, stats[ST_DEGENERATE] = ok ? 0.0 : 1.0;
}

__device__ __forceinline__ float grad_pixel(float r, float t, float m, double mu_r, double mu_t, double k1, double k2)
{
    const double d = ((double)t - mu_t) - k2 * ((double)r - mu_r);
    return (float)((k1 * (double)m) * d);
}

// one 4-pixel group per lane; the last P % 4 pixels go one by one through the lane that owns them.  A degenerate frame gets +0.
template <bool MASK>
__global__ __launch_bounds__(NT) void depth_corr_grad_kernel(int64_t P, const float *__restrict__ rendered, const float *__restrict__ target,
                                                             const float *__restrict__ mask, const double *__restrict__ stats, float *__restrict__ grad)
{
    const int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (GROUP * q >= P) return;
    const double mu_r = stats[ST_MU_R], mu_t = stats[ST_MU_T], k1 = stats[ST_K1], k2 = stats[ST_K2];
    const bool degenerate = stats[ST_DEGENERATE] != 0.0;
    if (GROUP * q + GROUP <= P) {
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!degenerate) {
            const float4 r = gsr_ld4<true>(reinterpret_cast<const float4 *>(rendered) + q), t = gsr_ld4<true>(reinterpret_cast<const float4 *>(target) + q);
            const float4 m = MASK ? gsr_ld4<true>(reinterpret_cast<const float4 *>(mask) + q) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            g.x = grad_pixel(r.x, t.x, m.x, mu_r, mu_t, k1, k2);
            g.y = grad_pixel(r.y, t.y, m.y, mu_r, mu_t, k1, k2);
            g.z = grad_pixel(r.z, t.z, m.z, mu_r, mu_t, k1, k2);
            g.w = grad_pixel(r.w, t.w, m.w, mu_r, mu_t, k1, k2);
        }
        reinterpret_cast<float4 *>(grad)[q] = g;
        return;
    }
    for (int64_t i = GROUP * q; i < P; ++i)
        grad[i] = degenerate ? 0.0f : grad_pixel(rendered[i], target[i], MASK ? mask[i] : 1.0f, mu_r, mu_t, k1, k2);
}

int64_t sum_blocks(int64_t P) { return gsr_record_count(P, GSR_DEPTH_CORR_BLOCK_PIXELS, GSR_DEPTH_CORR_MAX_BLOCKS); }

} // namespace

extern "C" {

size_t gsr_depth_corr_workspace_bytes(int32_t W, int32_t H)
{
    if (!gsr_image_dims_ok(W, H)) return 0;
    return gsr_align((size_t)GSR_DEPTH_CORR_RECORD_BYTES * (size_t)(sum_blocks((int64_t)W * H) + 1));   // + the moments' record
}

int gsr_depth_corr_loss_grad(const float *rendered, const float *target, const float *mask, float *grad, float *loss, float *fit, int32_t W, int32_t H,
                             float weight, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!rendered || !target || !loss || !workspace) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H) || !isfinite(weight)) return GSR_E_DIMS;
    if (!gsr_aligned16(rendered) || !gsr_aligned16(target) || !gsr_aligned16(mask) || !gsr_aligned16(grad) || !gsr_aligned16(workspace) ||
        !gsr_aligned4(loss) || !gsr_aligned4(fit))
        return GSR_E_ALIGN;
    if (workspace_bytes < gsr_depth_corr_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    const int64_t P = (int64_t)W * H, groups = gsr_div_up(P, GROUP);
    const int nb = (int)sum_blocks(P);
    hipStream_t s = (hipStream_t)stream;
    double *part = static_cast<double *>(workspace), *stats = part + (size_t)REC * nb;
    if (mask) hipLaunchKernelGGL(depth_corr_sums_kernel<true>, dim3(nb), dim3(NT), 0, s, P, groups, rendered, target, mask, part);
    else hipLaunchKernelGGL(depth_corr_sums_kernel<false>, dim3(nb), dim3(NT), 0, s, P, groups, rendered, target, mask, part);
    hipLaunchKernelGGL(depth_corr_finish_kernel, dim3(1), dim3(NT), 0, s, part, nb, weight, loss, fit, stats);
    if (grad) {
        const dim3 grid((unsigned)gsr_div_up(groups, NT));
        if (mask) hipLaunchKernelGGL(depth_corr_grad_kernel<true>, grid, dim3(NT), 0, s, P, rendered, target, mask, (const double *)stats, grad);
        else hipLaunchKernelGGL(depth_corr_grad_kernel<false>, grid, dim3(NT), 0, s, P, rendered, target, mask, (const double *)stats, grad);
    }
    return gsr_done();
}

} // extern "C"
