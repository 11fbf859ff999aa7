// normal_render.hip -- the Gaussians' own normals, their image over a frame's lists, its gradient into the backward's accumulator
// records, and the depth-normal consistency term (include/gsr_normal_render.h), for gfx950.
//
// gaussian_normals_kernel<BWD>: one thread per Gaussian, the header's steps (a) and (b) word for word; the view matrix travels as a
// kernel argument.  consistency_kernel: one thread per pixel of a grid-stride walk, elementwise, plus fixed_sum.h's tree for the two sums.
//
// normal_render_kernel<BWD> replays the forward blend's weights with frame_walk.h's FrameWalk: the tile's list staged in 48-byte
// records (position, pre-scaled conic, opacity, id, and the Gaussian's normal in the third word).
//   - forward: three running registers per lane, one fmaf per channel and applied entry in list order: what features.hip's exact
//     float32 MFMA computes at C = 3, without filing 32-column weight tiles for a product that uses 3 of its 32 channels.
//   - backward: distortion.hip's walk with u = G . n, and nine per-(pixel, entry) values instead of seven.  The flush (frame_walk.h,
//     ValueTile) sums each row of the value tile with two lanes (32 pixels each, in order, then the two halves): 2 * ROWS <= 64
//     lanes.  Nine values at four slots are 36 rows, 72 lanes: over.  The choices were (1) four slots and a second flush round for rows 32-35 --
//     two rounds of 32 dependent LDS adds for 8 more rows, and 36 x 65 x 4 B x 4 waves = 37 KB of LDS on top of the 12 KB of staging;
//     (2) one lane per row, 7 slots = 63 rows -- every lane busy, but 64 dependent adds per flush and 66 KB of LDS, two workgroups
//     per CU; (3) THREE slots: 27 rows, 54 of 64 lanes busy in the same two-lanes-per-row, 32-add flush, the header's summation
//     order unchanged, 28 KB of LDS for the value tile (distortion.hip's own figure).  With the 12 KB of staging (4 KB more than
//     that kernel's: the normals) the workgroup holds 43 KB, so three workgroups fit a CU's 160 KB where distortion.hip's 40 KB
//     fits four; the compiler's report (profiles/normal_render/kres.txt) says so too.  (3): the flush's cost
//     per entry is 32 adds / 3 entries against 32 / 4, a quarter more LDS read issue on a kernel whose walk, not whose flush,
//     is the long pole (the walk's per-entry chain -- exp, division, nine LDS stores -- is paid for every applied entry either way),
//     and it keeps the fixed order that the float32 restatement of the tests replays.  PITCH 65 (odd) spreads the flush's
//     row-parallel reads over the 64 banks; the walk's column stores (lane = consecutive floats) are conflict-free by construction.
//     Float atomics: one per (block, applied entry, value), 36 bytes per entry over two cache lines (the record's columns 3-10
//     and the Gaussian's row of dL_dnormals); -munsafe-fp-atomics makes them the hardware's global_atomic_add_f32, no CAS loop.
#include <math.h>

#include "frame_walk.h"
#include "gsr_normal_render.h"
#include "fixed_sum.h"

namespace {

constexpr int SLOTS = 3;     // entries per flush of the backward (see above)
constexpr int VALS = 9;      // S1, S2, Sxx, Sxy, Syy, Sop, Snx, Sny, Snz: the last three are the Gaussian's row of dL_dnormals
typedef ValueTile<VALS, SLOTS> Tile;

struct ViewK {
    float v[16];
};

// ---- (a), (b): one thread per Gaussian ----
// BWD: `g_in` is dL_dnormals [N][3] and `out` dL_drot [N][4] (added to); else `out` is normals [N][3].
template <bool BWD>
__global__ __launch_bounds__(256) void gaussian_normals_kernel(long long N, const float *__restrict__ scales, const float *__restrict__ rots,
                                                               const float *__restrict__ means, ViewK V, const float *__restrict__ g_in,
                                                               float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
    const float4 q = *reinterpret_cast<const float4 *>(rots + 4 * i);
    int c = 0;
    if (s[1] < s[c]) c = 1;
    if (s[2] < s[c]) c = 2;
    // column c of sigma3d.h's rotation matrix: its expressions, its order
    const float cs = 2.0f * q.w * q.w - 1.0f;
    const float qv[3] = {q.x, q.y, q.z};
    const float v[3] = {c == 0 ? 1.0f : 0.0f, c == 1 ? 1.0f : 0.0f, c == 2 ? 1.0f : 0.0f};
    const float cr[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
    float d = qv[0] * v[0];
    d += qv[1] * v[1];
    d += qv[2] * v[2];
    float a[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) a[r] = v[r] * cs + cr[r] * q.w * 2.0f + qv[r] * d * 2.0f;
    const float l2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const bool ok = l2 >= GSR_NORMAL_RENDER_MIN_AXIS2 && !(q.x == 0.0f && q.y == 0.0f && q.z == 0.0f && q.w == 0.0f);
    const float len = __fsqrt_rn(ok ? l2 : 1.0f);
    float ah[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) ah[r] = __fdiv_rn(a[r], len);
    float nc[3], pv[3];
    const float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        nc[j] = (ah[0] * V.v[j] + ah[1] * V.v[4 + j]) + ah[2] * V.v[8 + j];
        pv[j] = ((V.v[j] * p[0] + V.v[4 + j] * p[1]) + V.v[8 + j] * p[2]) + V.v[12 + j];
    }
    const float t = (nc[0] * pv[0] + nc[1] * pv[1]) + nc[2] * pv[2];
    const float sigma = t > 0.0f ? -1.0f : 1.0f;
    if (!BWD) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = ok ? sigma * nc[j] : 0.0f;
        return;
    }
    if (!ok) return;
    float gc[3], gw[3], ga[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) gc[j] = sigma * g_in[3 * i + j];
#pragma unroll
    for (int r = 0; r < 3; ++r) gw[r] = (V.v[4 * r] * gc[0] + V.v[4 * r + 1] * gc[1]) + V.v[4 * r + 2] * gc[2];
    const float e = (ah[0] * gw[0] + ah[1] * gw[1]) + ah[2] * gw[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) ga[r] = __fdiv_rn(gw[r] - ah[r] * e, len);
    const float k = (q.x * ga[0] + q.y * ga[1]) + q.z * ga[2];
    const float X[3] = {v[1] * ga[2] - v[2] * ga[1], v[2] * ga[0] - v[0] * ga[2], v[0] * ga[1] - v[1] * ga[0]};
    const float qc = qv[c], gac = ga[c];
    float4 dq = *reinterpret_cast<float4 *>(out + 4 * i);
    dq.x += ((2.0f * q.w) * X[0] + (2.0f * qc) * ga[0]) + (2.0f * k) * v[0];
    dq.y += ((2.0f * q.w) * X[1] + (2.0f * qc) * ga[1]) + (2.0f * k) * v[1];
    dq.z += ((2.0f * q.w) * X[2] + (2.0f * qc) * ga[2]) + (2.0f * k) * v[2];
    dq.w += (4.0f * q.w) * gac + 2.0f * ((ga[0] * cr[0] + ga[1] * cr[1]) + ga[2] * cr[2]);
    *reinterpret_cast<float4 *>(out + 4 * i) = dq;
}

// ---- (c), (d): the list walk ----
// BWD: `g_in` is dL_dout [H][W][3], `img` the stored forward image (read), `acc` the accumulator records, `dnorm` dL_dnormals [N][3]
// (cleared by the caller); else `img` is written.
template <bool BWD>
__global__ __launch_bounds__(256) void normal_render_kernel(FrameK f, const float *__restrict__ normals, const float *__restrict__ g_in, float *img,
                                                            float *__restrict__ acc, float *__restrict__ dnorm)
{
    __shared__ Tile::V<BWD> s_v; // the value tile: the backward's alone
    __shared__ Tile::Red s_red;
    __shared__ Tile::Con s_con;
    const FrameWalk walk(f);
    const bool inside = walk.inside;
    const size_t pix = walk.pix;

    float ox = 0.0f, oy = 0.0f, oz = 0.0f;       // forward: the running image
    float gx = 0.0f, gy = 0.0f, gz = 0.0f, total = 0.0f, P = 0.0f;
    if (BWD && inside && walk.nc > 0) {
        gx = g_in[3 * pix]; gy = g_in[3 * pix + 1]; gz = g_in[3 * pix + 2];
        total = (gx * img[3 * pix] + gy * img[3 * pix + 1]) + gz * img[3 * pix + 2];
    }
    Tile tile(s_v[BWD ? walk.wv : 0], s_red[walk.wv], s_con[walk.wv], walk, f, acc, dnorm, 3, 0);

    float T = 1.0f;
    walk.run<3>(
        f,
        [&](int id, float4 &rb, float4 &rc) {
            const float *pn = normals + (size_t)id * 3;
            rc = make_float4(pn[0], pn[1], pn[2], 0.f);
        },
        [&](const float4 &ra, const float4 &rb, const float4 &rc, float dx, float dy, float G, float t, bool applied) {
            if (BWD) {
                if (__builtin_amdgcn_ballot_w64(applied) != 0ull) {
                    float v[VALS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (applied) {
                        const float u = (gx * rc.x + gy * rc.y) + gz * rc.z;
                        const float w = t * T;
                        P = P + w * u;
                        const float R = total - P;
                        const float om = 1.0f - t;
                        const float q = T * u - R / om;
                        const float gd = G * q;
                        const float h = rb.y * gd;
                        const float hx = h * dx, hy = h * dy;
                        v[0] = hx; v[1] = hy; v[2] = hx * dx; v[3] = hx * dy; v[4] = hy * dy; v[5] = gd;
                        v[6] = w * gx; v[7] = w * gy; v[8] = w * gz;
                        T = T * om;
                    }
                    tile.file(v, ra, rb);
                }
            } else if (applied) {
                const float w = t * T;
                T = T * (1.0f - t);
                ox = __builtin_fmaf(w, rc.x, ox);
                oy = __builtin_fmaf(w, rc.y, oy);
                oz = __builtin_fmaf(w, rc.z, oz);
            }
        });
    if (BWD) {
        tile.finish();
    } else if (inside) {
        img[3 * pix] = ox; img[3 * pix + 1] = oy; img[3 * pix + 2] = oz;
    }
}

// ---- (e): the consistency term ----
constexpr int LOSS_MAX_BLOCKS = 2048;   // <= GSR_NORMALS_MAX_BLOCKS, and ceil(P / 256) <= that header's 32x8 tile count: its workspace holds the records

__global__ __launch_bounds__(GSR_SUM_THREADS) void consistency_kernel(long long npix, const float *__restrict__ Nimg, const float *__restrict__ nd,
                                                                      const float *__restrict__ valid, const float *__restrict__ m, float c,
                                                                      float *__restrict__ gN, float *__restrict__ gnd, double *__restrict__ part)
{
    __shared__ double s_red[GSR_SUM_WAVES][2];
    double s[2] = {0.0, 0.0};
    const float min2 = GSR_NORMAL_RENDER_MIN_LENGTH * GSR_NORMAL_RENDER_MIN_LENGTH;
    for (long long p = (long long)blockIdx.x * GSR_SUM_THREADS + threadIdx.x; p < npix; p += (long long)gridDim.x * GSR_SUM_THREADS) {
        const float Nx = Nimg[3 * p], Ny = Nimg[3 * p + 1], Nz = Nimg[3 * p + 2];
        const float L2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
        float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (valid[p] != 0.0f && L2 >= min2) {
            const float mm = m ? m[p] : 1.0f;
            const float len = __fsqrt_rn(L2);
            const float th[3] = {__fdiv_rn(Nx, len), __fdiv_rn(Ny, len), __fdiv_rn(Nz, len)};
            const float d[3] = {nd[3 * p], nd[3 * p + 1], nd[3 * p + 2]};
            const float dot = (d[0] * th[0] + d[1] * th[1]) + d[2] * th[2];
            const float km = c * mm;
            s[0] += (double)(mm * (1.0f - dot));
            s[1] += (double)mm;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                o[j] = -__fdiv_rn(km * (d[j] - th[j] * dot), len);
                o[3 + j] = -(km * th[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            gN[3 * p + j] = o[j];
            gnd[3 * p + j] = o[3 + j];
        }
    }
    const GsrBlockSums<double, 2> b = gsr_block_sums<GSR_SUM_THREADS>(s, s_red);
    if (threadIdx.x < 2) part[2 * (size_t)blockIdx.x + threadIdx.x] = b.pairwise(threadIdx.x);
}

// one workgroup: the record walk, the same tree, the two totals rounded once
__global__ __launch_bounds__(GSR_SUM_THREADS) void consistency_finish_kernel(const double *__restrict__ part, int n, float *__restrict__ sums)
{
    __shared__ double s_red[GSR_SUM_WAVES][2];
    GsrLaneSums<double, 2> s = gsr_record_walk<2, 2>(part, n);
    const GsrBlockSums<double, 2> b = gsr_block_sums<GSR_SUM_THREADS>(s.v, s_red);
    if (threadIdx.x < 2) sums[threadIdx.x] = (float)b.pairwise(threadIdx.x);
}

int check_gaussians(int64_t N, const float *scales, const float *rots, const float *means, const float *view, const void *a, const void *b)
{
    if (!scales || !rots || !means || !view || !a || !b) return GSR_E_NULL;
    if (N < 1 || N > 0x7FFFFFFFll) return GSR_E_DIMS;
    for (int k = 0; k < 16; ++k)
        if (!isfinite(view[k])) return GSR_E_DIMS;
    if (!gsr_aligned16(scales) || !gsr_aligned16(rots) || !gsr_aligned16(means) || !gsr_aligned16(a) || !gsr_aligned16(b)) return GSR_E_ALIGN;
    return GSR_OK;
}

ViewK view_k(const float *view)
{
    ViewK v;
    for (int k = 0; k < 16; ++k) v.v[k] = view[k];
    return v;
}

} // namespace

extern "C" int gsr_gaussian_normals(int64_t N, const float *scales, const float *rotations, const float *means, const float *viewmatrix,
                                    float *normals, void *stream)
{
    const int rc = check_gaussians(N, scales, rotations, means, viewmatrix, normals, normals);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL((gaussian_normals_kernel<false>), dim3((unsigned)gsr_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, (long long)N, scales,
                       rotations, means, view_k(viewmatrix), nullptr, normals);
    return gsr_done();
}

extern "C" int gsr_gaussian_normals_backward(int64_t N, const float *scales, const float *rotations, const float *means, const float *viewmatrix,
                                             const float *dL_dnormals, float *dL_drot, void *stream)
{
    const int rc = check_gaussians(N, scales, rotations, means, viewmatrix, dL_dnormals, dL_drot);
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL((gaussian_normals_kernel<true>), dim3((unsigned)gsr_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, (long long)N, scales,
                       rotations, means, view_k(viewmatrix), dL_dnormals, dL_drot);
    return gsr_done();
}

extern "C" int gsr_normal_render_forward(const GsrFeaturesFrame *frame, const float *normals, float *out, void *stream)
{
    const int rc = check_frame(frame, normals, out);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    // a frame with D = 0 walks nothing: every pixel is written as 0
    hipLaunchKernelGGL((normal_render_kernel<false>), dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, normals, nullptr, out, nullptr, nullptr);
    return gsr_done();
}

extern "C" int gsr_normal_render_backward(const GsrFeaturesFrame *frame, const float *normals, const float *dL_dout, const float *out,
                                          float *accumulators, float *dL_dnormals, void *stream)
{
    const int rc = check_frame(frame, normals, dL_dout, out, accumulators, dL_dnormals);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (hipMemsetAsync(dL_dnormals, 0, sizeof(float) * 3 * (size_t)k.N, (hipStream_t)stream) != hipSuccess) return GSR_E_HIP;
    if (k.D == 0) return gsr_done(); // nothing was blended: nothing to add
    hipLaunchKernelGGL((normal_render_kernel<true>), dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, normals, dL_dout, const_cast<float *>(out),
                       accumulators, dL_dnormals);
    return gsr_done();
}

extern "C" int gsr_normal_consistency_loss(const float *Nimg, const float *n_d, const float *valid, const float *m, int32_t W, int32_t H, float weight,
                                           float *gN, float *gnd, float *sums, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!Nimg || !n_d || !valid || !gN || !gnd || !sums || !workspace) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H) || !isfinite(weight)) return GSR_E_DIMS;
    if (!gsr_aligned16(Nimg) || !gsr_aligned16(n_d) || !gsr_aligned16(valid) || !gsr_aligned16(m) || !gsr_aligned16(gN) || !gsr_aligned16(gnd) ||
        !gsr_aligned4(sums) || !gsr_aligned16(workspace))
        return GSR_E_ALIGN;
    if (workspace_bytes < gsr_normals_workspace_bytes(W, H)) return GSR_E_WORKSPACE;
    const long long npix = (long long)W * H;
    const int nb = (int)gsr_record_count(npix, GSR_SUM_THREADS, LOSS_MAX_BLOCKS);
    const float c = (float)((double)weight / ((double)W * (double)H));
    double *part = static_cast<double *>(workspace);
    hipLaunchKernelGGL(consistency_kernel, dim3(nb), dim3(GSR_SUM_THREADS), 0, (hipStream_t)stream, npix, Nimg, n_d, valid, m, c, gN, gnd, part);
    hipLaunchKernelGGL(consistency_finish_kernel, dim3(1), dim3(GSR_SUM_THREADS), 0, (hipStream_t)stream, part, nb, sums);
    return gsr_done();
}
