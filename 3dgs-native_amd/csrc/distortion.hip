// distortion.hip -- the depth-distortion regulariser over a frame's lists, and its gradient (include/gsr_distortion.h), for gfx950.
//
// Both directions replay the forward blend's weights w_k(p) from the frame's buffers with frame_walk.h's FrameWalk (the tile's list
// staged in 32-byte records whose spare float carries 1/depth); the backward's reduction is that header's ValueTile.
//   - forward: the running sums A, mu, S of the header live in three registers per lane over the whole list.  No LDS beyond the
//     staging, no atomics, the same bits every call and with or without masks (an entry no pixel applies changes nothing).
//   - backward: a second front-to-back walk with the stored A, mu, S; the suffix sum of dL/dalpha is the stored total minus the
//     running prefix.  Each lane files its seven per-(pixel, entry) values as seven rows of a 28 x 64 tile in LDS (four entries per
//     tile), which ValueTile sums and adds to the entry's accumulator record.  Seven values cannot fill the 32 columns of an MFMA
//     tile (features.hip's transpose would run at 7/32 of its rate and needs the values to factor into weight x image, which they
//     do not), so the reduction is LDS reads and adds.
#include "frame_walk.h"
#include "gsr_distortion.h"

namespace {

constexpr int SLOTS = 4;     // entries per flush of the backward
constexpr int VALS = 7;      // S1, S2, Sxx, Sxy, Syy, Sop, Sdm: the seventh is d(1/depth), column 11 of the accumulator record
typedef ValueTile<VALS, SLOTS> Tile;

// The walk, its staging and its LDS are frame_walk.h's; the staged record's spare float is the Gaussian's 1/depth.
// BWD: `g_in` is dL_ddist [H][W], `mom` the forward's moments (read), `acc` the accumulator records; else `dist` and `mom` are written.
template <bool BWD>
__global__ __launch_bounds__(256) void distortion_kernel(FrameK f, const float *__restrict__ invd, long long invd_stride, const float *__restrict__ g_in,
                                                         float *__restrict__ dist, float *mom, float *__restrict__ acc)
{
    __shared__ Tile::V<BWD> s_v; // the value tile: the backward's alone
    __shared__ Tile::Red s_red;
    __shared__ Tile::Con s_con;
    const FrameWalk walk(f);
    const bool inside = walk.inside;
    const size_t pix = walk.pix;

    float A = 0.0f, mu = 0.0f, S = 0.0f; // forward: running; backward: the stored totals
    float g = 0.0f, gA = 0.0f, total = 0.0f, P = 0.0f;
    if (BWD && inside && walk.nc > 0) {
        const float4 mo = *reinterpret_cast<const float4 *>(mom + 4 * pix);
        A = mo.x; mu = mo.y; S = mo.z;
        g = g_in[pix];
        gA = g * A;
        total = 2.0f * (gA * S);
    }
    Tile tile(s_v[BWD ? walk.wv : 0], s_red[walk.wv], s_con[walk.wv], walk, f, acc, acc, 16, 11);

    float T = 1.0f;
    walk.run<2>(
        f, DepthFill{invd, invd_stride, nullptr},
        [&](const float4 &ra, const float4 &rb, float dx, float dy, float G, float t, bool applied) {
            if (BWD) {
                if (__builtin_amdgcn_ballot_w64(applied) != 0ull) {
                    float v[VALS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (applied) {
                        const float w = t * T;
                        const float d = rb.w - mu;
                        const float u = (((A * d) * d) + S) * g;
                        P = P + w * u;
                        const float R = total - P;
                        const float om = 1.0f - t;
                        const float q = T * u - R / om;
                        const float gd = G * q;
                        const float h = rb.y * gd;
                        const float hx = h * dx, hy = h * dy;
                        v[0] = hx; v[1] = hy; v[2] = hx * dx; v[3] = hx * dy; v[4] = hy * dy; v[5] = gd;
                        v[6] = ((2.0f * gA) * w) * d;
                        T = T * om;
                    }
                    tile.file(v, ra, rb);
                }
            } else if (applied) {
                const float w = t * T;
                T = T * (1.0f - t);
                const float A1 = A + w;
                const float d = rb.w - mu;
                const float r = w / A1;
                S = S + ((A * r) * d) * d;
                mu = mu + r * d;
                A = A1;
            }
        });
    if (BWD) {
        tile.finish();
    } else if (inside) {
        dist[pix] = A * S;
        *reinterpret_cast<float4 *>(mom + 4 * pix) = make_float4(A, mu, S, 0.0f);
    }
}

} // namespace

extern "C" int gsr_distortion_forward(const GsrDistortionFrame *frame, float *dist, float *moments, void *stream)
{
    const int rc = check_frame(frame, dist, moments);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    // a frame with D = 0 walks nothing: every pixel is written as 0
    hipLaunchKernelGGL((distortion_kernel<false>), dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, frame->inv_depth,
                       (long long)frame->inv_depth_stride, nullptr, dist, moments, nullptr);
    return gsr_done();
}

extern "C" int gsr_distortion_backward(const GsrDistortionFrame *frame, const float *dL_ddist, const float *moments, float *accumulators,
                                       void *stream)
{
    const int rc = check_frame(frame, dL_ddist, moments, accumulators);
    if (rc != GSR_OK) return rc;
    const FrameK k = frame_k(frame);
    if (k.D == 0) return GSR_OK; // nothing was blended: nothing to add
    hipLaunchKernelGGL((distortion_kernel<true>), dim3(frame_tiles(k)), dim3(256), 0, (hipStream_t)stream, k, frame->inv_depth,
                       (long long)frame->inv_depth_stride, dL_ddist, nullptr, const_cast<float *>(moments), accumulators);
    return gsr_done();
}
