// normals.hip -- surface normals from the rendered depth (include/gsr_normals.h): n = the unit cross product of the central
// differences of the camera-space points P = z r, z = (1 - final_T) / Dinv; the exact gradient of any dL/dn back to the inverse-depth
// and alpha images; and the cosine loss against a normal prior, fused with that gradient.
//
// It sits beside depth_corr.hip, between the forward and the backward: launches of its own, no existing kernel touched.  No float
// atomics and no host wait.
//   normals_fwd_kernel     one 32 x 8 tile per workgroup, one pixel per thread: z of the tile and a 1-pixel halo (34 x 10) and the rays
//                          of its columns and rows through LDS, then the normal and the validity flag.
//   normals_grad_kernel    one 32 x 8 tile per workgroup and round, one launch, three phases over LDS:
//                            1  z of the tile and a 2-pixel halo (36 x 12), NaN where a pixel is outside the image or not defined, and
//                               the rays of the 36 columns and 12 rows (a ray is a correctly rounded division: 48 a tile, not 8 a pixel);
//                            2  for the tile and a 1-pixel halo (34 x 10): the normal, u = (I - n n^T) g / |N| and the two cross
//                               products c1 = b x u, c2 = u x a that the pixel hands to its four neighbours (zeros where the pixel is
//                               not valid); the tile's own pixels add their loss terms to the lane's float64 sums;
//                            3  every pixel of the tile GATHERS dL/dP from its four neighbours' c1 / c2, projects it on its ray and
//                               writes gD and gA.  Nothing is scattered.
//                          MODE_VJP reads g = dL/dn; MODE_LOSS forms g = -(weight m) t^ from the target: the phases are the same code,
//                          so the fused loss gives the bits of the VJP of that g.  GRAD = false (loss only) stops after phase 2's sums.
//   normals_finish_kernel  one workgroup adds the partial records (float64, fixed_sum.h) and rounds the two totals once.
// Why one launch with a halo and not a u image in the workspace with a second gather launch: the second form writes and reads back
// 24 bytes per pixel (c1 and c2; u alone would make the gather redo a and b of four neighbours from twelve more depths) on top of
// the 20-45 bytes the pass has to move, for one launch more; the halo costs 1.69 x the 8 bytes of Dinv and final_T, most of it
// from L2, and 10 KB of LDS.  DESIGN.md, "Normals from depth", has the compiler's register and LDS report.
#include <float.h>
#include <math.h>

#include "fixed_sum.h"
#include "gsr_normals.h"

namespace {

constexpr int NT = 256;
constexpr int TW = GSR_NORMALS_TILE_W, TH = GSR_NORMALS_TILE_H;
constexpr int ZW = TW + 4, ZH = TH + 4;   // phase 1: the tile and a 2-pixel halo
constexpr int CW = TW + 2, CH = TH + 2;   // phase 2: the tile and a 1-pixel halo
constexpr int NS = GSR_NORMALS_SUMS_FLOATS;
constexpr int REC = GSR_NORMALS_RECORD_BYTES / 8;
static_assert(TW * TH == NT, "one pixel of the tile per thread");
static_assert(REC == NS && GSR_NORMALS_RECORD_BYTES % 16 == 0, "a record holds the two sums in one 16-byte unit");

enum { MODE_VJP = 0, MODE_LOSS = 1 };

struct NormalsCam {
    float tan_fovx, tan_fovy, alpha_min;
    int W, H;
};
struct Rot {
    float m[9];
};
struct V3 {
    float x, y, z;
};

__device__ __forceinline__ V3 sub3(V3 p, V3 q) { return V3{p.x - q.x, p.y - q.y, p.z - q.z}; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float norm2(V3 a) { return (a.x * a.x + a.y * a.y) + a.z * a.z; }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__device__ __forceinline__ float ray_x(const NormalsCam &c, int x) { return ((float)(2 * x + 1) / (float)c.W - 1.0f) * c.tan_fovx; }
__device__ __forceinline__ float ray_y(const NormalsCam &c, int y) { return ((float)(2 * y + 1) / (float)c.H - 1.0f) * c.tan_fovy; }

// z of pixel (x, y), NaN where it lies outside the image or is not defined
__device__ __forceinline__ float depth_at(const NormalsCam &c, const float *__restrict__ Dinv, const float *__restrict__ final_T, int x, int y)
{
    if (x < 0 || y < 0 || x >= c.W || y >= c.H) return NAN;
    const size_t i = (size_t)y * c.W + x;
    const float D = Dinv[i], A = 1.0f - final_T[i];
    const bool defined = isfinite(A) && isfinite(D) && A >= c.alpha_min && D > 0.0f;
    return defined ? A / D : NAN;
}

__device__ __forceinline__ V3 point_of(float rx, float ry, float z) { return V3{z * rx, z * ry, z}; }

// The rays of a tile's columns and rows, once per tile in LDS: a ray costs a correctly rounded division, and a pixel's frame needs
// six of them.  rx[k] belongs to column x0 + k, ry[k] to row y0 + k (columns and rows outside the image get a ray like any other).
template <int NX, int NY>
__device__ __forceinline__ void tile_rays(const NormalsCam &c, int x0, int y0, float (&rx)[NX], float (&ry)[NY])
{
    static_assert(NX + NY <= NT, "one ray per thread");
    if (threadIdx.x < NX) rx[threadIdx.x] = ray_x(c, x0 + (int)threadIdx.x);
    else if (threadIdx.x < NX + NY) ry[threadIdx.x - NX] = ray_y(c, y0 + (int)threadIdx.x - NX);
}

// The differences and the cross product of a pixel from its own and its neighbours' z (up = y - 1, down = y + 1) and the rays of its
// three columns rx[0 .. 2] = x - 1, x, x + 1 and three rows ry[0 .. 2]; false where the pixel is not valid.
// A NaN among the five (outside, not defined) makes |N|^2 a NaN and every comparison false, but the flags are tested by name.
struct Frame {
    V3 a, b, N;
    float nn;
};
__device__ __forceinline__ bool frame_of(const float *rx, const float *ry, float zc, float zu, float zd, float zl, float zr, Frame &f)
{
    if (!(zc == zc && zu == zu && zd == zd && zl == zl && zr == zr)) return false;
    f.a = sub3(point_of(rx[1], ry[2], zd), point_of(rx[1], ry[0], zu));
    f.b = sub3(point_of(rx[2], ry[1], zr), point_of(rx[0], ry[1], zl));
    f.N = cross3(f.a, f.b);
    f.nn = norm2(f.N);
    return f.nn > GSR_NORMALS_MIN_NORM2 * (norm2(f.a) * norm2(f.b)) && f.nn <= FLT_MAX;
}

// workgroup k takes tile k, in row-major tile order: z of the tile and a 1-pixel halo and the rays of its columns and rows through LDS
__global__ __launch_bounds__(NT) void normals_fwd_kernel(NormalsCam c, int tiles_x, const float *__restrict__ Dinv, const float *__restrict__ final_T,
                                                         float *__restrict__ normals, float *__restrict__ valid)
{
    __shared__ float s_z[CH][CW];
    __shared__ float s_rx[CW], s_ry[CH];
    const int x0 = (int)(blockIdx.x % tiles_x) * TW, y0 = (int)(blockIdx.x / tiles_x) * TH;
    for (int k = threadIdx.x; k < CW * CH; k += NT) s_z[k / CW][k % CW] = depth_at(c, Dinv, final_T, x0 - 1 + k % CW, y0 - 1 + k / CW);
    tile_rays(c, x0 - 1, y0 - 1, s_rx, s_ry);
    __syncthreads();
    const int i = threadIdx.x % TW, j = threadIdx.x / TW, x = x0 + i, y = y0 + j;
    if (x >= c.W || y >= c.H) return;
    Frame f;
    const bool ok = frame_of(&s_rx[i], &s_ry[j], s_z[j + 1][i + 1], s_z[j][i + 1], s_z[j + 2][i + 1], s_z[j + 1][i], s_z[j + 1][i + 2], f);
    V3 n = {0.0f, 0.0f, 0.0f};
    if (ok) {
        const float len = sqrtf(f.nn);
        n = V3{f.N.x / len, f.N.y / len, f.N.z / len};
    }
    const size_t p = (size_t)y * c.W + x;
    normals[3 * p] = n.x, normals[3 * p + 1] = n.y, normals[3 * p + 2] = n.z;
    if (valid) valid[p] = ok ? 1.0f : 0.0f;
}

// One workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... in row-major tile order.  part (MODE_LOSS): one record per workgroup.
template <int MODE, bool GRAD, bool MASK>
__global__ __launch_bounds__(NT) void normals_grad_kernel(NormalsCam c, int tiles_x, int tiles, const float *__restrict__ Dinv,
                                                          const float *__restrict__ final_T, const float *__restrict__ src /* dL/dn or the target */,
                                                          Rot R, const float *__restrict__ mask, float weight, float *__restrict__ gD,
                                                          float *__restrict__ gA, double *__restrict__ part)
{
    __shared__ float s_z[ZH][ZW];
    __shared__ float s_c[GRAD ? 6 : 1][CH][CW];   // c1.xyz, c2.xyz
    __shared__ double s_red[GSR_SUM_WAVES][NS];
    __shared__ float s_rx[ZW], s_ry[ZH];
    double s[NS] = {};
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int x0 = (tile % tiles_x) * TW, y0 = (tile / tiles_x) * TH;
        // phase 1
        for (int k = threadIdx.x; k < ZW * ZH; k += NT) s_z[k / ZW][k % ZW] = depth_at(c, Dinv, final_T, x0 - 2 + k % ZW, y0 - 2 + k / ZW);
        tile_rays(c, x0 - 2, y0 - 2, s_rx, s_ry);
        __syncthreads();
        // phase 2: pixel (x0 - 1 + i, y0 - 1 + j), whose z sits at s_z[j + 1][i + 1]
        for (int k = threadIdx.x; k < CW * CH; k += NT) {
            const int i = k % CW, j = k / CW, x = x0 - 1 + i, y = y0 - 1 + j;
            const bool own = i >= 1 && i <= TW && j >= 1 && j <= TH && x < c.W && y < c.H;
            V3 c1 = {0.0f, 0.0f, 0.0f}, c2 = {0.0f, 0.0f, 0.0f};
            Frame f;
            if ((GRAD || own) && frame_of(&s_rx[i], &s_ry[j], s_z[j + 1][i + 1], s_z[j][i + 1], s_z[j + 2][i + 1], s_z[j + 1][i], s_z[j + 1][i + 2], f)) {
                // (a valid pixel lies inside the image: its own z is not NaN)
                const size_t p = (size_t)y * c.W + x;
                const float len = sqrtf(f.nn);
                const V3 n = {f.N.x / len, f.N.y / len, f.N.z / len};
                V3 g;
                if (MODE == MODE_LOSS) {
                    const float tx = src[3 * p], ty = src[3 * p + 1], tz = src[3 * p + 2];
                    const V3 sv = {(R.m[0] * tx + R.m[1] * ty) + R.m[2] * tz, (R.m[3] * tx + R.m[4] * ty) + R.m[5] * tz,
                                   (R.m[6] * tx + R.m[7] * ty) + R.m[8] * tz};
                    const float ss = norm2(sv);
                    const bool t_ok = ss > 0.0f && ss <= FLT_MAX;
                    const float sl = sqrtf(ss), m = MASK ? mask[p] : 1.0f;
                    const V3 th = {sv.x / sl, sv.y / sl, sv.z / sl};
                    const float wm = -(weight * m);
                    g = t_ok ? V3{wm * th.x, wm * th.y, wm * th.z} : V3{0.0f, 0.0f, 0.0f};
                    if (own && t_ok) {
                        const double md = (double)m;
                        s[0] += md * (1.0 - (((double)n.x * (double)th.x + (double)n.y * (double)th.y) + (double)n.z * (double)th.z));
                        s[1] += md;
                    }
                } else {
                    g = V3{src[3 * p], src[3 * p + 1], src[3 * p + 2]};
                }
                if constexpr (GRAD) {
                    const float ng = dot3(n, g);
                    const V3 u = {(g.x - n.x * ng) / len, (g.y - n.y * ng) / len, (g.z - n.z * ng) / len};
                    c1 = cross3(f.b, u), c2 = cross3(u, f.a);
                }
            }
            if constexpr (GRAD) {
                s_c[0][j][i] = c1.x, s_c[1][j][i] = c1.y, s_c[2][j][i] = c1.z;
                s_c[3][j][i] = c2.x, s_c[4][j][i] = c2.y, s_c[5][j][i] = c2.z;
            }
        }
        __syncthreads();
        // phase 3: pixel (x0 + i, y0 + j) at s_c[.][j + 1][i + 1], s_z[j + 2][i + 2]
        if constexpr (GRAD) {
            const int i = threadIdx.x % TW, j = threadIdx.x / TW, x = x0 + i, y = y0 + j;
            if (x < c.W && y < c.H) {
                float d = 0.0f, al = 0.0f;
                const float z = s_z[j + 2][i + 2];
                if (z == z) {
                    float gP[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        gP[k] = ((s_c[k][j][i + 1] - s_c[k][j + 2][i + 1]) + s_c[3 + k][j + 1][i]) - s_c[3 + k][j + 1][i + 2];
                    const float gz = (s_rx[i + 2] * gP[0] + s_ry[j + 2] * gP[1]) + gP[2];
                    const float D = Dinv[(size_t)y * c.W + x];
                    d = gz * (-z / D), al = gz * (1.0f / D);
                    d = d == 0.0f ? 0.0f : d, al = al == 0.0f ? 0.0f : al;   // +0, never -0, where nothing depends on the pixel
                }
                gD[(size_t)y * c.W + x] = d, gA[(size_t)y * c.W + x] = al;
            }
        }
        __syncthreads();   // the next tile overwrites s_z and s_c
    }
    if (MODE == MODE_LOSS) {
        const GsrBlockSums<double, NS> b = gsr_block_sums<NT>(s, s_red);
        if (threadIdx.x < NS) part[(size_t)REC * blockIdx.x + threadIdx.x] = b.pairwise(threadIdx.x);
    }
}

// one workgroup: the record walk, the same tree, the two totals rounded once
__global__ __launch_bounds__(NT) void normals_finish_kernel(const double *__restrict__ part, int n, float *__restrict__ sums)
{
    __shared__ double s_red[GSR_SUM_WAVES][NS];
    GsrLaneSums<double, NS> s = gsr_record_walk<NS, REC>(part, n);
    const GsrBlockSums<double, NS> b = gsr_block_sums<NT>(s.v, s_red);
    if (threadIdx.x < NS) sums[threadIdx.x] = (float)b.pairwise(threadIdx.x);
}

struct Tiles {
    int x, y;
    int64_t n;
};
Tiles tiles_of(int32_t W, int32_t H)
{
    Tiles t;
    t.x = (int)gsr_div_up(W, TW), t.y = (int)gsr_div_up(H, TH);
    t.n = (int64_t)t.x * t.y;   // at most 2^28 / 8 + 1: an int
    return t;
}
int64_t record_count(int32_t W, int32_t H)
{
    const int64_t n = tiles_of(W, H).n;
    return n < GSR_NORMALS_MAX_BLOCKS ? n : GSR_NORMALS_MAX_BLOCKS;
}
bool cam_ok(float tan_fovx, float tan_fovy, int32_t W, int32_t H, float alpha_min)
{
    return gsr_image_dims_ok(W, H) && isfinite(tan_fovx) && isfinite(tan_fovy) && tan_fovx > 0.0f && tan_fovy > 0.0f && isfinite(alpha_min);
}

template <int MODE, bool GRAD>
void launch_grad(bool with_mask, int blocks, hipStream_t s, const NormalsCam &c, const Tiles &t, const float *Dinv, const float *final_T, const float *src,
                 const Rot &R, const float *mask, float weight, float *gD, float *gA, double *part)
{
    if (with_mask)
        hipLaunchKernelGGL((normals_grad_kernel<MODE, GRAD, true>), dim3(blocks), dim3(NT), 0, s, c, t.x, (int)t.n, Dinv, final_T, src, R, mask, weight, gD, gA,
                           part);
    else
        hipLaunchKernelGGL((normals_grad_kernel<MODE, GRAD, false>), dim3(blocks), dim3(NT), 0, s, c, t.x, (int)t.n, Dinv, final_T, src, R, mask, weight, gD, gA,
                           part);
}

} // namespace

extern "C" {

size_t gsr_normals_workspace_bytes(int32_t W, int32_t H)
{
    if (!gsr_image_dims_ok(W, H)) return 0;
    return gsr_align((size_t)GSR_NORMALS_RECORD_BYTES * (size_t)record_count(W, H));
}

int gsr_normals_from_depth(const float *Dinv, const float *final_T, float tan_fovx, float tan_fovy, int32_t W, int32_t H, float alpha_min,
                           float *normals_out, float *valid_out, void *stream)
{
    if (!Dinv || !final_T || !normals_out) return GSR_E_NULL;
    if (!cam_ok(tan_fovx, tan_fovy, W, H, alpha_min)) return GSR_E_DIMS;
    if (!gsr_aligned16(Dinv) || !gsr_aligned16(final_T) || !gsr_aligned16(normals_out) || !gsr_aligned16(valid_out)) return GSR_E_ALIGN;
    const NormalsCam c = {tan_fovx, tan_fovy, alpha_min, W, H};
    const Tiles t = tiles_of(W, H);
    hipLaunchKernelGGL(normals_fwd_kernel, dim3((unsigned)t.n), dim3(NT), 0, (hipStream_t)stream, c, t.x, Dinv, final_T, normals_out, valid_out);
    return gsr_done();
}

int gsr_normals_from_depth_backward(const float *Dinv, const float *final_T, float tan_fovx, float tan_fovy, int32_t W, int32_t H, float alpha_min,
                                    const float *dL_dnormals, float *gD, float *gA, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!Dinv || !final_T || !dL_dnormals || !gD || !gA || !workspace) return GSR_E_NULL;
    if (!cam_ok(tan_fovx, tan_fovy, W, H, alpha_min)) return GSR_E_DIMS;
    if (!gsr_aligned16(Dinv) || !gsr_aligned16(final_T) || !gsr_aligned16(dL_dnormals) || !gsr_aligned16(gD) || !gsr_aligned16(gA) ||
        !gsr_aligned16(workspace))
        return GSR_E_ALIGN;
    if (workspace_bytes < gsr_normals_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    const NormalsCam c = {tan_fovx, tan_fovy, alpha_min, W, H};
    const Tiles t = tiles_of(W, H);
    launch_grad<MODE_VJP, true>(false, (int)t.n, (hipStream_t)stream, c, t, Dinv, final_T, dL_dnormals, Rot{}, nullptr, 0.0f, gD, gA, nullptr);
    return gsr_done();
}

int gsr_normals_loss_grad(const float *Dinv, const float *final_T, const float *target, const float *R, const float *mask, float tan_fovx,
                          float tan_fovy, int32_t W, int32_t H, float alpha_min, float weight, float *gD, float *gA, float *sums, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    if (!Dinv || !final_T || !target || !sums || !workspace || (gD == nullptr) != (gA == nullptr)) return GSR_E_NULL;
    if (!cam_ok(tan_fovx, tan_fovy, W, H, alpha_min) || !isfinite(weight)) return GSR_E_DIMS;
    if (!gsr_aligned16(Dinv) || !gsr_aligned16(final_T) || !gsr_aligned16(target) || !gsr_aligned16(mask) || !gsr_aligned16(gD) || !gsr_aligned16(gA) ||
        !gsr_aligned16(workspace) || !gsr_aligned4(sums))
        return GSR_E_ALIGN;
    if (workspace_bytes < gsr_normals_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    const NormalsCam c = {tan_fovx, tan_fovy, alpha_min, W, H};
    const Tiles t = tiles_of(W, H);
    const int nb = (int)record_count(W, H);
    Rot rot = {{1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}};
    if (R)
        for (int k = 0; k < 9; ++k) rot.m[k] = R[k];
    hipStream_t s = (hipStream_t)stream;
    double *part = static_cast<double *>(workspace);
    if (gD) launch_grad<MODE_LOSS, true>(mask != nullptr, nb, s, c, t, Dinv, final_T, target, rot, mask, weight, gD, gA, part);
    else launch_grad<MODE_LOSS, false>(mask != nullptr, nb, s, c, t, Dinv, final_T, target, rot, mask, weight, gD, gA, part);
    hipLaunchKernelGGL(normals_finish_kernel, dim3(1), dim3(NT), 0, s, (const double *)part, nb, sums);
    return gsr_done();
}

} // extern "C"
