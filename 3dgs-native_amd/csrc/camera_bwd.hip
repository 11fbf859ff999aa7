// camera_bwd.hip -- dL/dview, dL/dproj and dL/dcampos (include/gsr_camera_grads.h) for gfx950.
//
// The true derivative of this library's forward (preprocess_kernel) with respect to its three camera inputs, each taken as
// independent, chained from the screen-space gradients the blend backward leaves in the 64-byte accumulator records
// (GradRec: 0-2 dL/dcolour, 3-4 dL/dndc, 6 dL/dA, 7 HALF of dL/dB (quirk conic_b_half), 9 dL/dC, 11 dL/dinvd after the aux
// backward, else 0).  Per visible Gaussian (radius > 0), with P = [p, 1] and the row-vector convention p_view = P @ view:
//   mean2D -> proj    p_hom = P @ proj, ndc = p_hom.xy / (p_hom.w + 1e-7):  dL/dproj[r][c] += P[r] dL/dp_hom[c]
//   conic  -> view    Sigma2D = T Sigma3D T^T, T = J(t) W, W = view[0:3,0:3], t = P @ view[:, 0:3], with the true derivative of
//                     the 1.3 tan(fov) clamp inside J, the 0.3 blur and the plain 1/det^2:  dL/dW = J^T dL/dT and
//                     dL/dview[r][c] += P[r] dL/dt[c]
//   invd   -> view    invd = 1 / t.z:  dL/dt.z += -dL/dinvd / t.z^2
//   colour -> campos  dir = (p - campos) / |p - campos| (unclamped channels only): dL/dcampos = -(I - n n^T) dL/ddir / |p - campos|
// Culled Gaussians add nothing; radii, rectangles and the sort order are piecewise constant.
//
// The sum over Gaussians is bitwise reproducible (no float atomics): camera_partials_kernel runs a fixed grid (a function of N
// alone), each lane sums its grid-stride Gaussians in float32, and the rest is a fixed-order sum ("The fixed-order
// sum"; fixed_sum.h) with serial wave sums: float32 butterflies and float64 wave sums into one row of partials (plain vector
// stores); camera_finish_kernel, one workgroup, walks the rows and sums them in float64 and rounds once.  A standalone pair of
// launches after the blend half: geom_backward_kernel is not touched.
#include "fixed_sum.h"
#include "sh_stage.h"
#include "sigma3d.h"

#include <algorithm>

namespace {

// the 27 entries that can be non-zero: view[r][c] for c < 3 (column 3 of view is never read), proj[r][c] for c in {0, 1, 3}
// (p_hom.z is never read) and campos.  Slot k of the partial rows holds output entry kOut[k] of the 36-float result.
constexpr int kSlots = 27;
constexpr int kRow = 32; // doubles per partial row (256 B)
__constant__ int8_t kOut[kSlots] = {0,  1,  2,  4,  5,  6,  8,  9,  10, 12, 13, 14,               // view
                                    16, 17, 19, 20, 21, 23, 24, 25, 27, 28, 29, 31, 32, 33, 34}; // proj, campos

__device__ __forceinline__ float dot3(const float a[3], const float b[3])
{
    float r = a[0] * b[0];
    r += a[1] * b[1];
    r += a[2] * b[2];
    return r;
}

// One Gaussian's term, added into acc[27] (slot order of kOut).
// AA (include/gsr_antialias.h): the forward drew with opacity * rho, so column 10 (dL/d(opacity * rho)) times opacity times
// d(rho)/d(a, b, c) joins the cotangent of the blurred covariance; rho is the forward's own (aa_scale), these are its (a, b, c).
template <bool AA, class... AaIn>
__device__ __forceinline__ void camera_term(int64_t i, const float *__restrict__ means, const float *__restrict__ scales,
                                            const float *__restrict__ rots, const float *__restrict__ shs, int degree, float scale_mod,
                                            const CamK &cam, const float *__restrict__ cov3Ds, const float *__restrict__ clamped_state,
                                            const GradRec *__restrict__ accs, const float *__restrict__ sh_dir_grad, float acc[kSlots], AaIn... aa_in)
{
    const float4 *ap = reinterpret_cast<const float4 *>(accs + i);
    const float4 a0 = ap[0], a1 = ap[1], a2 = ap[2];
    const float P[4] = {means[3 * i], means[3 * i + 1], means[3 * i + 2], 1.0f};

    // ---- mean2D -> proj ----
    {
        float ph[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r = cam.proj[j] * P[0];
            r += cam.proj[4 + j] * P[1];
            r += cam.proj[8 + j] * P[2];
            r += cam.proj[12 + j] * P[3];
            ph[j] = r;
        }
        const float pw = 1.0f / (ph[3] + 0.0000001f);
        const float gx = a0.w, gy = a1.x; // dL/dndc
        const float d0 = gx * pw, d1 = gy * pw, d3 = -(gx * ph[0] + gy * ph[1]) * pw * pw;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc[12 + 3 * r] += P[r] * d0;
            acc[13 + 3 * r] += P[r] * d1;
            acc[14 + 3 * r] += P[r] * d3;
        }
    }

    // ---- conic (and invd) -> view ----
    {
        float c3[6];
        if (cov3Ds) {
#pragma unroll
            for (int k = 0; k < 6; ++k) c3[k] = cov3Ds[6 * i + k];
        } else {
            const float4 q = *reinterpret_cast<const float4 *>(rots + 4 * i);
            gsr_sigma3d(scale_mod * scales[3 * i], scale_mod * scales[3 * i + 1], scale_mod * scales[3 * i + 2], q, c3);
        }
        const float Sg[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
        float t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float r = cam.view[j] * P[0];
            r += cam.view[4 + j] * P[1];
            r += cam.view[8 + j] * P[2];
            r += cam.view[12 + j] * P[3];
            t[j] = r;
        }
        const float tz = t[2];
        const float limx = 1.3f * cam.tan_fovx, limy = 1.3f * cam.tan_fovy;
        const float rx = fminf(limx, fmaxf(-limx, t[0] / tz)), ry = fminf(limy, fmaxf(-limy, t[1] / tz));
        const bool clx = rx != t[0] / tz, cly = ry != t[1] / tz;
        const float tx = rx * tz, ty = ry * tz;
        const float fx = (float)cam.W / (2.0f * cam.tan_fovx), fy = (float)cam.H / (2.0f * cam.tan_fovy); // the forward's focal lengths
        const float itz = 1.0f / tz, itz2 = itz * itz;
        const float J00 = fx * itz, J02 = -fx * tx * itz2, J11 = fy * itz, J12 = -fy * ty * itz2;
        float Wm[3][3], T[2][3], TS[2][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Wm[r][c] = cam.view[4 * r + c];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            T[0][j] = J00 * Wm[0][j] + J02 * Wm[2][j];
            T[1][j] = J11 * Wm[1][j] + J12 * Wm[2][j];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) TS[k][j] = T[k][0] * Sg[0][j] + T[k][1] * Sg[1][j] + T[k][2] * Sg[2][j];
        const float a = dot3(TS[0], T[0]) + 0.3f, b = dot3(TS[0], T[1]), c = dot3(TS[1], T[1]) + 0.3f;
        const float det = a * c - b * b;
        const float gA = a1.z, gB = 2.0f * a1.w, gC = a2.y; // column 7 holds half of dL/dB (conic_b_half)
        const float id2 = 1.0f / (det * det);
        float dLa = (-c * c * gA + b * c * gB - b * b * gC) * id2;
        float dLb = (2.0f * b * c * gA - (det + 2.0f * b * b) * gB + 2.0f * a * b * gC) * id2;
        float dLc = (-b * b * gA + a * b * gB - a * a * gC) * id2;
        if constexpr (AA) {
            const float a0 = dot3(TS[0], T[0]), c0 = dot3(TS[1], T[1]), bb = b * b;
            if ((a0 * c0 - bb) / det > 0.000025f) { // on the floor rho is constant
                const float *const aa_arr[] = {aa_in...}; // opacity, aa_scale
                const float kh = aa_arr[0][i] * a2.z * 0.3f * id2 / (2.0f * aa_arr[1][i]);
                dLa += kh * (c * c0 + bb);
                dLc += kh * (a * a0 + bb);
                dLb -= kh * 2.0f * b * (a + c0);
            }
        }
        // dL/dT = 2 G T Sigma3D, G = [[dLa, dLb/2], [dLb/2, dLc]]
        float dT[2][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dT[0][j] = 2.0f * dLa * TS[0][j] + dLb * TS[1][j];
            dT[1][j] = dLb * TS[0][j] + 2.0f * dLc * TS[1][j];
        }
        // dL/dW = J^T dL/dT, straight into view[0:3, 0:3]
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            acc[j] += J00 * dT[0][j];
            acc[3 + j] += J11 * dT[1][j];
            acc[6 + j] += J02 * dT[0][j] + J12 * dT[1][j];
        }
        // dL/dJ = dL/dT W^T -> dL/dt through J(t) and the frustum clamp
        const float dJ00 = dot3(dT[0], Wm[0]), dJ02 = dot3(dT[0], Wm[2]), dJ11 = dot3(dT[1], Wm[1]), dJ12 = dot3(dT[1], Wm[2]);
        const float dtx_c = -fx * itz2 * dJ02, dty_c = -fy * itz2 * dJ12; // dL/d(clamped tx), dL/d(clamped ty)
        float dt[3];
        dt[0] = clx ? 0.0f : dtx_c;
        dt[1] = cly ? 0.0f : dty_c;
        dt[2] = -fx * itz2 * dJ00 - fy * itz2 * dJ11 + 2.0f * fx * tx * itz2 * itz * dJ02 + 2.0f * fy * ty * itz2 * itz * dJ12;
        if (clx) dt[2] += rx * dtx_c; // tx = clamp(t.x / t.z) t.z: d/dt.z = the clamped ratio
        if (cly) dt[2] += ry * dty_c;
        dt[2] += -a2.w * itz2; // invd = 1 / t.z (slot 11: zero unless the aux backward ran)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 * r + j] += P[r] * dt[j];
    }

    // ---- colour -> campos ----
    if (degree > 0) {
        const float d[3] = {P[0] - cam.campos[0], P[1] - cam.campos[1], P[2] - cam.campos[2]};
        float l2 = d[0] * d[0];
        l2 += d[1] * d[1];
        l2 += d[2] * d[2];
        const float len = sqrtf(l2);
        if (len > 0.0f) {
            const float n[3] = {d[0] / len, d[1] / len, d[2] / len};
            float dRGB[3];
            dRGB[0] = a0.x * (1.0f - clamped_state[3 * i]);
            dRGB[1] = a0.y * (1.0f - clamped_state[3 * i + 1]);
            dRGB[2] = a0.z * (1.0f - clamped_state[3 * i + 2]);
            float gx[3] = {0.f, 0.f, 0.f}, gy[3] = {0.f, 0.f, 0.f}, gz[3] = {0.f, 0.f, 0.f};
            if (sh_dir_grad) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    gx[k] = sh_dir_grad[9 * i + k];
                    gy[k] = sh_dir_grad[9 * i + 3 + k];
                    gz[k] = sh_dir_grad[9 * i + 6 + k];
                }
            } else {
                sh_direction_sums(shs + 48 * i, degree, n[0], n[1], n[2], gx, gy, gz);
            }
            const float gd[3] = {dot3(gx, dRGB), dot3(gy, dRGB), dot3(gz, dRGB)};
            const float ng = dot3(n, gd);
            const float il = 1.0f / len;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[24 + k] -= (gd[k] - n[k] * ng) * il; // dcampos = -d/d(p - campos)
        }
    }
}

// (the two arrays of the AA kernel -- opacity, aa_scale -- are its parameters alone, so the classic kernel's argument block is unchanged)
template <bool AA = false, class... AaIn>
__global__ __launch_bounds__(256) void camera_partials_kernel(int64_t N, const float *__restrict__ means, const float *__restrict__ scales,
                                                              const float *__restrict__ rots, const float *__restrict__ shs, int degree,
                                                              float scale_mod, CamK cam, const int32_t *__restrict__ radii,
                                                              const float *__restrict__ cov3Ds, const float *__restrict__ clamped_state,
                                                              const GradRec *__restrict__ accs, const float *__restrict__ sh_dir_grad,
                                                              double *__restrict__ partials, AaIn... aa_in)
{
    static_assert(sizeof...(AaIn) == (AA ? 2 : 0), "opacity and aa_scale, in the AA kernel only");
    __shared__ double s_wave[GSR_SUM_WAVES][kSlots];
    float acc[kSlots];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) acc[k] = 0.0f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride)
        if (radii[i] > 0)
            camera_term<AA>(i, means, scales, rots, shs, degree, scale_mod, cam, cov3Ds, clamped_state, accs, sh_dir_grad, acc, aa_in...);
    // the wave's sums in float32, then the four waves in float64, in wave order
    const GsrBlockSums<double, kSlots> b = gsr_block_sums<256, true>(acc, s_wave);
    if (threadIdx.x < kRow) partials[(size_t)blockIdx.x * kRow + threadIdx.x] = threadIdx.x < kSlots ? b.serial(threadIdx.x) : 0.0;
}

// one workgroup: the record walk over the rows (at most four per lane: the grid is capped at GSR_CAMERA_MAX_BLOCKS) and the
// same tree, all in float64, the four wave sums again in wave order
__global__ __launch_bounds__(256) void camera_finish_kernel(int nblk, const double *__restrict__ partials, float *__restrict__ out)
{
    __shared__ double s_wave[GSR_SUM_WAVES][kSlots];
    GsrLaneSums<double, kSlots> acc = gsr_record_walk<kSlots, kRow>(partials, nblk);
    const GsrBlockSums<double, kSlots> b = gsr_block_sums<256, true>(acc.v, s_wave);
    if (threadIdx.x < 36) {
        int k = -1;
#pragma unroll
        for (int j = 0; j < kSlots; ++j)
            if (kOut[j] == (int)threadIdx.x) k = j;
        const double v = k >= 0 ? b.serial(k) : 0.0;
        out[threadIdx.x] = (float)v;
    }
}

} // namespace

int gsr_camera_blocks(int64_t N) { return N <= 0 ? 0 : (int)std::min<int64_t>(gsr_div_up(N, 256), GSR_CAMERA_MAX_BLOCKS); }
size_t gsr_camera_scratch_bytes(int64_t N) { return (size_t)gsr_camera_blocks(N) * kRow * sizeof(double); }

hipError_t gsr_launch_camera_backward(const GsrScene &sc, const CamK &cam, const GsrGeom &g, const GradRec *acc, float *dL_dcamera, void *scratch,
                                      hipStream_t s, const float *aa_scale)
{
    const int nblk = gsr_camera_blocks(sc.N);
    if (nblk == 0) return hipMemsetAsync(dL_dcamera, 0, 36 * sizeof(float), s);
    double *partials = (double *)scratch;
#define CAMERA_ARGS                                                                                                           \
    dim3((unsigned)nblk), dim3(256), 0, s, sc.N, sc.means, sc.scales, sc.rotations, sc.sh, sc.sh_degree, sc.scale_modifier, cam,      \
        g.radii, g.cov3D, g.clamped_state, acc, g.sh_dir_grad, partials
    if (aa_scale) hipLaunchKernelGGL((camera_partials_kernel<true, const float *, const float *>), CAMERA_ARGS, sc.opacity, aa_scale);
    else hipLaunchKernelGGL(camera_partials_kernel<false>, CAMERA_ARGS);
#undef CAMERA_ARGS
    hipLaunchKernelGGL(camera_finish_kernel, dim3(1), dim3(256), 0, s, nblk, partials, dL_dcamera);
    return hipGetLastError();
}
