// mesh_sample.hip -- area-weighted random points on a triangle soup (include/gsr_mesh_eval.h): what the mesh evaluation compares.
// A stage of its own: new kernels only, on the caller's stream, no host wait, no atomics.
//
//   mesh_sample_count_kernel   one thread per triangle: its area, its stochastically rounded count (entry T of the counts is 0, so the
//                              exclusive scan's entry T is the total)
//   gsr_launch_exclusive_scan  counts -> offsets
//   mesh_sample_emit_kernel    one thread per SAMPLE: a binary search over the offsets names its triangle, so one huge triangle among
//                              small ones is no longer one thread's work; the offsets of neighbouring samples are the same cache lines.
// Every float32 step is one rounded operation in the header's order (the file is compiled without contraction).
#include <math.h>

#include "gsr_internal.h"
#include "gsr_mesh_eval.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ uint32_t mix(uint32_t x)
{
    x ^= x >> 16, x *= 0x7FEB352Du, x ^= x >> 15, x *= 0x846CA68Bu, x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float unit(uint32_t seed, uint32_t t, uint32_t k)
{
    const uint32_t h = mix(mix(seed ^ (t * 0x9E3779B9u)) ^ (k * 0x85EBCA6Bu));
    return __fmul_rn((float)(h >> 8), 5.9604644775390625e-08f);   // 2^-24: exact
}
struct Tri { float3 a, e1, e2; };
__device__ __forceinline__ Tri load_tri(const float *__restrict__ tri, int64_t t)
{
    const float *v = tri + 9 * t;
    Tri r;
    r.a = make_float3(v[0], v[1], v[2]);
    r.e1 = make_float3(__fsub_rn(v[3], v[0]), __fsub_rn(v[4], v[1]), __fsub_rn(v[5], v[2]));
    r.e2 = make_float3(__fsub_rn(v[6], v[0]), __fsub_rn(v[7], v[1]), __fsub_rn(v[8], v[2]));
    return r;
}

__global__ __launch_bounds__(NT) void mesh_sample_count_kernel(int64_t T, const float *__restrict__ tri, float density, uint32_t seed,
                                                               int32_t *__restrict__ counts /* [T + 1] */)
{
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t > T) return;
    int32_t n = 0;
    if (t < T) {
        const Tri r = load_tri(tri, t);
        const float nx = __fsub_rn(__fmul_rn(r.e1.y, r.e2.z), __fmul_rn(r.e1.z, r.e2.y));
        const float ny = __fsub_rn(__fmul_rn(r.e1.z, r.e2.x), __fmul_rn(r.e1.x, r.e2.z));
        const float nz = __fsub_rn(__fmul_rn(r.e1.x, r.e2.y), __fmul_rn(r.e1.y, r.e2.x));
        const float area = __fmul_rn(0.5f, __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz))));
        if (isfinite(area)) {
            const float x = fminf(__fmul_rn(area, density), (float)GSR_SURFACE_SAMPLE_MAX_PER_TRIANGLE);
            const float whole = floorf(x);
            n = (int32_t)whole + (unit(seed, (uint32_t)t, 0xFFFFFFFFu) < __fsub_rn(x, whole) ? 1 : 0);
        }
    }
    counts[t] = n;
}

__global__ __launch_bounds__(NT) void mesh_sample_emit_kernel(int64_t T, const float *__restrict__ tri, const int32_t *__restrict__ offsets, uint32_t seed,
                                                              int64_t capacity, float *__restrict__ points, int32_t *__restrict__ tri_index /* may be NULL */)
{
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= capacity || i >= (int64_t)offsets[T]) return;
    // the triangle of sample i: the last t with offsets[t] <= i (triangles without samples share their successor's offset)
    int64_t lo = 0, hi = T;                                    // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int64_t m = lo + (hi - lo) / 2;
        if ((int64_t)offsets[m] <= i) lo = m;
        else hi = m;
    }
    const int64_t j = i - (int64_t)offsets[lo];
    const Tri r = load_tri(tri, lo);
    float r1 = unit(seed, (uint32_t)lo, (uint32_t)(2 * j)), r2 = unit(seed, (uint32_t)lo, (uint32_t)(2 * j + 1));
    if (__fadd_rn(r1, r2) > 1.0f) r1 = __fsub_rn(1.0f, r1), r2 = __fsub_rn(1.0f, r2);
    points[3 * i + 0] = __fadd_rn(__fadd_rn(r.a.x, __fmul_rn(r1, r.e1.x)), __fmul_rn(r2, r.e2.x));
    points[3 * i + 1] = __fadd_rn(__fadd_rn(r.a.y, __fmul_rn(r1, r.e1.y)), __fmul_rn(r2, r.e2.y));
    points[3 * i + 2] = __fadd_rn(__fadd_rn(r.a.z, __fmul_rn(r1, r.e1.z)), __fmul_rn(r2, r.e2.z));
    if (tri_index) tri_index[i] = (int32_t)lo;
}

bool count_ok(int64_t T) { return T >= 1 && T <= GSR_SURFACE_SAMPLE_MAX_TRIANGLES; }
size_t counts_bytes(int64_t T) { return gsr_align(4 * (size_t)(T + 1)); }

} // namespace

extern "C" {

size_t gsr_surface_sample_workspace_bytes(int64_t T)
{
    return count_ok(T) ? counts_bytes(T) + gsr_align(4 * ((size_t)gsr_div_up(T + 1, GSR_SCAN_WAVE_ITEMS) + 4)) : 0;
}

int gsr_surface_sample_count(int64_t T, const float *tri, float density, uint32_t seed, int32_t *offsets, void *ws, size_t ws_bytes, void *stream)
{
    if (!tri || !offsets || !ws) return GSR_E_NULL;
    if (!count_ok(T) || !(density > 0.0f) || isinf(density)) return GSR_E_DIMS;
    if (!gsr_aligned16(tri) || !gsr_aligned16(offsets) || !gsr_aligned16(ws)) return GSR_E_ALIGN;
    if (ws_bytes < gsr_surface_sample_workspace_bytes(T)) return GSR_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int32_t *counts = static_cast<int32_t *>(ws);
    int32_t *scan_tmp = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + counts_bytes(T));
    hipLaunchKernelGGL(mesh_sample_count_kernel, dim3((unsigned)gsr_div_up(T + 1, NT)), dim3(NT), 0, s, T, tri, density, seed, counts);
    if (gsr_launch_exclusive_scan(counts, offsets, scan_tmp, T + 1, s) != hipSuccess) return GSR_E_HIP;
    return gsr_done();
}

int gsr_surface_sample_emit(int64_t T, const float *tri, const int32_t *offsets, uint32_t seed, int64_t S_capacity, float *points, int32_t *tri_index,
                         void *stream)
{
    if (!tri || !offsets || !points) return GSR_E_NULL;
    if (!count_ok(T) || S_capacity < 1 || S_capacity > GSR_SURFACE_SAMPLE_MAX_SAMPLES) return GSR_E_DIMS;
    if (!gsr_aligned16(tri) || !gsr_aligned16(offsets) || !gsr_aligned16(points) || !gsr_aligned16(tri_index)) return GSR_E_ALIGN;
    hipLaunchKernelGGL(mesh_sample_emit_kernel, dim3((unsigned)gsr_div_up(S_capacity, NT)), dim3(NT), 0, (hipStream_t)stream, T, tri, offsets, seed,
                       S_capacity, points, tri_index);
    return gsr_done();
}

} // extern "C"
