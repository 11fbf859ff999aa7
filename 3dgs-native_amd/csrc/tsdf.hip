// tsdf.hip -- TSDF fusion of depth images into a dense volume and marching-tetrahedra mesh extraction (include/gsr_tsdf.h, which
// states every float32 step; the tests hold these kernels to it bit for bit).
//
// A stage of its own behind the forward: launches of its own, no existing kernel touched.  No atomics, no host wait.
//   tsdf_reset_kernel      tsdf = 1, weight = 0, color = 0.
//   tsdf_depth_kernel      z = (1 - T) / Dinv where gsr_normals.h's rule defines it, 0 elsewhere: the integrator's input from the forward's images.
//   tsdf_integrate_kernel  one voxel per thread, 256 consecutive voxels (x fastest) per workgroup.  Up to GSR_TSDF_VIEWS_PER_LAUNCH
//                          views arrive BY VALUE in the kernel-argument area: the loop index over them is uniform, so a view's matrix,
//                          tangents and pointers are scalar loads into SGPRs, once per wave and view.  The voxel's tsdf, weight and
//                          colour stay in registers over the views of the launch: 20 bytes read and 20 written per voxel and launch
//                          instead of per view.  Per voxel and view: 9 multiply-adds of the projection, two correctly rounded
//                          divisions for the pixel, one gathered depth (neighbouring voxels hit neighbouring pixels: L1 / L2), and
//                          for a voxel inside the truncation band two to five more divisions.  Bound by issue, not by memory.
//   mesh_count_kernel      one cell per thread, GSR_MESH_GROUP_CELLS consecutive cells per workgroup: the eight corners' weights and
//                          signs, the triangle count of the six tetrahedra from the sign bits alone, one count per workgroup.
//   mesh_scan_kernel       GSR_MESH_SCAN_GROUPS workgroup counts per workgroup -> exclusive offsets in place, one int64 sum each.
//   mesh_scan_top_kernel   one workgroup: the sums -> exclusive int64 offsets in place, and the total.
//   mesh_emit_kernel       the count's walk again, an exclusive scan of the threads' counts in LDS, then every thread writes its
//                          cell's triangles at (workgroup offset + thread offset): cell order, tetrahedron order, triangle order.
//                          Only surface cells (about G^2 of G^3) reach the vertex code, which re-reads the two ends of an edge from
//                          the volume (L1 / L2 hits: the corners were just loaded) rather than keep eight corners in indexed registers.
#include <float.h>
#include <math.h>

#include "gsr_internal.h"
#include "gsr_tsdf.h"

namespace {

constexpr int NT = 256;
constexpr int VPL = GSR_TSDF_VIEWS_PER_LAUNCH;
constexpr int GC = GSR_MESH_GROUP_CELLS;
constexpr int SG = GSR_MESH_SCAN_GROUPS;
static_assert(GC == NT, "one cell per thread");
static_assert(SG == 4 * NT, "four workgroup counts per thread of the scan");
static_assert(sizeof(GsrTsdfView) == 104, "gsr_tsdf.h states the record's size");
static_assert(sizeof(GsrTsdfView) * VPL + 128 <= 4096, "the views of a launch fit the kernel-argument area");

struct VolK {
    int Gx, Gy, Gz;
    float s;
    float o[3];
    float *tsdf, *weight, *color;
};
struct ViewBatch {
    GsrTsdfView v[VPL];
};

__global__ __launch_bounds__(NT) void tsdf_reset_kernel(VolK vol, uint32_t nvox)
{
    const uint32_t i = blockIdx.x * (uint32_t)NT + threadIdx.x;
    if (i >= nvox) return;
    vol.tsdf[i] = 1.0f;
    vol.weight[i] = 0.0f;
    if (vol.color) {
        float *c = vol.color + (size_t)i * 3;
        c[0] = 0.0f;
        c[1] = 0.0f;
        c[2] = 0.0f;
    }
}

__global__ __launch_bounds__(NT) void tsdf_depth_kernel(const float *Dinv, const float *final_T, int n, float alpha_min, float *z_out)
{
    const int i = (int)(blockIdx.x * (uint32_t)NT + threadIdx.x);
    if (i >= n) return;
    const float D = Dinv[i], A = 1.0f - final_T[i];
    z_out[i] = (isfinite(A) && isfinite(D) && A >= alpha_min && D > 0.0f) ? A / D : 0.0f;
}

__global__ __launch_bounds__(NT) void tsdf_integrate_kernel(VolK vol, uint32_t nvox, ViewBatch batch, int nv, float trunc, float depth_max, float w_max)
{
    const uint32_t i = blockIdx.x * (uint32_t)NT + threadIdx.x;
    if (i >= nvox) return;
    const uint32_t row = i / (uint32_t)vol.Gx;
    const int ix = (int)(i - row * (uint32_t)vol.Gx), iy = (int)(row % (uint32_t)vol.Gy), iz = (int)(row / (uint32_t)vol.Gy);
    const float X = vol.o[0] + vol.s * (float)ix, Y = vol.o[1] + vol.s * (float)iy, Z = vol.o[2] + vol.s * (float)iz;
    float *cp = vol.color ? vol.color + (size_t)i * 3 : nullptr;
    float ts = vol.tsdf[i], w = vol.weight[i];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (cp) {
        c0 = cp[0];
        c1 = cp[1];
        c2 = cp[2];
    }
    for (int k = 0; k < nv; ++k) {
        const GsrTsdfView &q = batch.v[k];
        const float px = ((X * q.view[0] + Y * q.view[4]) + Z * q.view[8]) + q.view[12];
        const float py = ((X * q.view[1] + Y * q.view[5]) + Z * q.view[9]) + q.view[13];
        const float pz = ((X * q.view[2] + Y * q.view[6]) + Z * q.view[10]) + q.view[14];
        if (!(pz > 0.0f && isfinite(pz))) continue;
        const float u = ((px / (pz * q.tan_fovx) + 1.0f) * (float)q.W - 1.0f) * 0.5f;
        const float v = ((py / (pz * q.tan_fovy) + 1.0f) * (float)q.H - 1.0f) * 0.5f;
        const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
        if (!(fu >= 0.0f && fu < (float)q.W && fv >= 0.0f && fv < (float)q.H)) continue;
        const int pix = (int)fv * q.W + (int)fu; // 0 <= fu < W and 0 <= fv < H, W H <= 2^28: inside the image
        const float d = q.depth[pix];
        if (!(isfinite(d) && d > 0.0f && d <= depth_max)) continue;
        const float sdf = d - pz;
        if (sdf < -trunc) continue;
        const float t = fminf(1.0f, sdf / trunc);
        const float w1 = w + q.w_obs;
        ts = (ts * w + t * q.w_obs) / w1;
        if (cp && q.color) {
            const float *col = q.color + (size_t)pix * 3;
            c0 = (c0 * w + col[0] * q.w_obs) / w1;
            c1 = (c1 * w + col[1] * q.w_obs) / w1;
            c2 = (c2 * w + col[2] * q.w_obs) / w1;
        }
        w = fminf(w1, w_max);
    }
    vol.tsdf[i] = ts;
    vol.weight[i] = w;
    if (cp) {
        cp[0] = c0;
        cp[1] = c1;
        cp[2] = c2;
    }
}

// ---- marching tetrahedra ----
// the six Kuhn tetrahedra: corner codes c0 | c1 << 4 | c2 << 8 | c3 << 12 for the permutations 012 021 102 120 201 210
constexpr unsigned tet_codes(int a, int b) { return 0u | (1u << a) << 4 | ((1u << a) | (1u << b)) << 8 | 7u << 12; }
constexpr unsigned TET[6] = {tet_codes(0, 1), tet_codes(0, 2), tet_codes(1, 0), tet_codes(1, 2), tet_codes(2, 0), tet_codes(2, 1)};
constexpr bool TET_NEG[6] = {false, true, true, false, false, true};

__device__ __forceinline__ int code_of(unsigned codes, int idx) { return (int)((codes >> (4 * idx)) & 15u); }
// inside bits of a tetrahedron's four corners from the cell's eight
__device__ __forceinline__ unsigned tet_mask(unsigned in8, unsigned codes)
{
    return ((in8 >> code_of(codes, 0)) & 1u) | ((in8 >> code_of(codes, 1)) & 1u) << 1 | ((in8 >> code_of(codes, 2)) & 1u) << 2 |
           ((in8 >> code_of(codes, 3)) & 1u) << 3;
}
__device__ __forceinline__ int tet_triangles(unsigned m)
{
    const int pc = __popc(m);
    return pc == 2 ? 2 : (pc == 1 || pc == 3) ? 1 : 0;
}

struct Cell {
    int ix, iy, iz;
    unsigned in8; // inside bits of the eight corners, by corner code
    int ntri;     // 0 for a cell that is not active or past the end
};

__device__ __forceinline__ Cell load_cell(const VolK &vol, uint32_t c, uint32_t ncells, float min_weight)
{
    Cell cell = {0, 0, 0, 0u, 0};
    if (c >= ncells) return cell;
    const uint32_t cx = (uint32_t)(vol.Gx - 1), cy = (uint32_t)(vol.Gy - 1);
    const uint32_t row = c / cx;
    cell.ix = (int)(c - row * cx);
    cell.iy = (int)(row % cy);
    cell.iz = (int)(row / cy);
    const size_t sx = 1, sy = (size_t)vol.Gx, sz = (size_t)vol.Gx * (size_t)vol.Gy;
    const size_t base = (size_t)cell.iz * sz + (size_t)cell.iy * sy + (size_t)cell.ix; // corners reach ix + 1 <= Gx - 1 ...: inside the volume
    bool active = true;
    unsigned in8 = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const size_t p = base + (k & 1) * sx + ((k >> 1) & 1) * sy + (size_t)(k >> 2) * sz;
        active = active && (vol.weight[p] >= min_weight);
        in8 |= (vol.tsdf[p] < 0.0f ? 1u : 0u) << k;
    }
    if (!active) return cell;
    cell.in8 = in8;
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) n += tet_triangles(tet_mask(in8, TET[t]));
    cell.ntri = n;
    return cell;
}

// exclusive scan of one value per thread over the workgroup; *total = the sum.  T = int or long long.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T x, T *lds /* [2 * NT] */, T *total)
{
    const int t = threadIdx.x;
    int cur = 0;
    lds[t] = x;
    __syncthreads();
    for (int step = 1; step < NT; step <<= 1) {
        const T v = lds[cur * NT + t] + (t >= step ? lds[cur * NT + t - step] : (T)0);
        lds[(cur ^ 1) * NT + t] = v;
        cur ^= 1;
        __syncthreads();
    }
    const T incl = lds[cur * NT + t];
    *total = lds[cur * NT + NT - 1];
    __syncthreads(); // the caller may scan again
    return incl - x;
}

__global__ __launch_bounds__(NT) void mesh_count_kernel(VolK vol, uint32_t ncells, float min_weight, int32_t *cnt)
{
    __shared__ int lds[2 * NT];
    const Cell cell = load_cell(vol, blockIdx.x * (uint32_t)GC + threadIdx.x, ncells, min_weight);
    int total;
    block_exclusive_scan<int>(cell.ntri, lds, &total);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// cnt[0 .. groups): counts -> exclusive offsets within each run of SG, sums[b] = the run's total
__global__ __launch_bounds__(NT) void mesh_scan_kernel(int32_t *cnt, uint32_t groups, long long *sums)
{
    __shared__ int lds[2 * NT];
    const uint32_t first = blockIdx.x * (uint32_t)SG + threadIdx.x * 4u;
    int v[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = first + j < groups ? cnt[first + j] : 0;
        mine += v[j];
    }
    int total;
    int off = block_exclusive_scan<int>(mine, lds, &total); // at most SG * GC * 12 = 3.1 M: an int
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (first + j < groups) cnt[first + j] = off;
        off += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = (long long)total;
}

// sums[0 .. n): totals -> exclusive offsets, *total = their sum.  One workgroup; n <= 2^23 / SG = 8192.
__global__ __launch_bounds__(NT) void mesh_scan_top_kernel(long long *sums, int n, long long *total)
{
    __shared__ long long lds[2 * NT];
    const int per = (n + NT - 1) / NT, lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    long long mine = 0;
    for (int k = lo; k < hi; ++k) mine += sums[k];
    long long all;
    long long off = block_exclusive_scan<long long>(mine, lds, &all);
    for (int k = lo; k < hi; ++k) {
        const long long v = sums[k];
        sums[k] = off;
        off += v;
    }
    if (threadIdx.x == 0) *total = all;
}

struct Vtx {
    float p[3], c[3];
    long long key;
};

// the vertex of the crossed edge from corner code cp to corner code cq (cp a subset of cq) of the cell
__device__ __forceinline__ Vtx edge_vertex(const VolK &vol, const Cell &cell, int cp, int cq)
{
    const int P[3] = {cell.ix + (cp & 1), cell.iy + ((cp >> 1) & 1), cell.iz + (cp >> 2)};
    const int dbits = cq ^ cp;
    const int D[3] = {dbits & 1, (dbits >> 1) & 1, dbits >> 2};
    const size_t sy = (size_t)vol.Gx, sz = (size_t)vol.Gx * (size_t)vol.Gy;
    const size_t lp = (size_t)P[2] * sz + (size_t)P[1] * sy + (size_t)P[0];
    const size_t lq = lp + (size_t)D[2] * sz + (size_t)D[1] * sy + (size_t)D[0];
    const float a = vol.tsdf[lp], b = vol.tsdf[lq];
    const float t = a / (a - b);
    Vtx v;
#pragma unroll
    for (int c = 0; c < 3; ++c) v.p[c] = (vol.o[c] + vol.s * (float)P[c]) + t * (vol.s * (float)D[c]);
    if (vol.color) {
        const float *ca = vol.color + lp * 3, *cb = vol.color + lq * 3;
        const float one_t = 1.0f - t;
#pragma unroll
        for (int c = 0; c < 3; ++c) v.c[c] = one_t * ca[c] + t * cb[c];
    } else {
        v.c[0] = v.c[1] = v.c[2] = 0.0f;
    }
    v.key = (long long)lp * GSR_MESH_DIRECTIONS + (long long)((0x65423100u >> (4 * dbits)) & 15u); // direction number of the bits 1 .. 7
    return v;
}
__device__ __forceinline__ Vtx tet_edge(const VolK &vol, const Cell &cell, unsigned codes, int m, int n)
{
    const int lo = m < n ? m : n, hi = m < n ? n : m;
    return edge_vertex(vol, cell, code_of(codes, lo), code_of(codes, hi));
}

// the key alone of the edge between tetrahedron corners (pair >> 2) and (pair & 3)
__device__ __forceinline__ long long tet_edge_key(const VolK &vol, const Cell &cell, unsigned codes, int pair)
{
    const int m = pair >> 2, n = pair & 3;
    const int cp = code_of(codes, m < n ? m : n), cq = code_of(codes, m < n ? n : m);
    const size_t lp = ((size_t)(cell.iz + (cp >> 2)) * (size_t)vol.Gy + (size_t)(cell.iy + ((cp >> 1) & 1))) * (size_t)vol.Gx + (size_t)(cell.ix + (cp & 1));
    return (long long)lp * GSR_MESH_DIRECTIONS + (long long)((0x65423100u >> (4 * (cq ^ cp))) & 15u);
}

__device__ __forceinline__ void put_triangle(long long T, long long T_cap, const Vtx &v0, const Vtx &v1, const Vtx &v2, float *vertices, float *colors,
                                             long long *keys)
{
    if (T < 0 || T >= T_cap) return; // nothing at or past the caller's capacity (T < 0: a workspace no count has filled)
    const Vtx *v[3] = {&v0, &v1, &v2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            vertices[(T * 3 + k) * 3 + c] = v[k]->p[c];
            if (colors) colors[(T * 3 + k) * 3 + c] = v[k]->c[c];
        }
        keys[T * 3 + k] = v[k]->key;
    }
}

__global__ __launch_bounds__(NT) void mesh_emit_kernel(VolK vol, uint32_t ncells, float min_weight, const int32_t *cnt, const long long *sums,
                                                       long long T_cap, float *vertices, float *colors, long long *keys)
{
    __shared__ int lds[2 * NT];
    const Cell cell = load_cell(vol, blockIdx.x * (uint32_t)GC + threadIdx.x, ncells, min_weight);
    int total;
    const int off = block_exclusive_scan<int>(cell.ntri, lds, &total);
    if (cell.ntri == 0) return;
    long long T = sums[blockIdx.x / (uint32_t)SG] + (long long)cnt[blockIdx.x] + (long long)off;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const unsigned codes = TET[t];
        const unsigned m = tet_mask(cell.in8, codes);
        const int pc = __popc(m);
        if (pc == 1 || pc == 3) {
            const int L = __ffs(pc == 1 ? m : (~m & 15u)) - 1;
            const unsigned oth = (0x06132C39u >> (8 * L)) & 255u; // (j, k, l) of L, two bits each: 123 032 301 210
            const Vtx v0 = tet_edge(vol, cell, codes, L, (int)(oth & 3u));
            const Vtx v1 = tet_edge(vol, cell, codes, L, (int)((oth >> 2) & 3u));
            const Vtx v2 = tet_edge(vol, cell, codes, L, (int)((oth >> 4) & 3u));
            const bool flip = TET_NEG[t] != (pc == 3); // pc == 3: the lone corner is outside
            if (flip) put_triangle(T, T_cap, v0, v2, v1, vertices, colors, keys);
            else put_triangle(T, T_cap, v0, v1, v2, vertices, colors, keys);
            T += 1;
        } else if (pc == 2) {
            const unsigned out = ~m & 15u;
            const int i = __ffs(m) - 1, j = 31 - __clz(m), k = __ffs(out) - 1, l = 31 - __clz(out);
            const bool flip = TET_NEG[t] != (m == 5u || m == 10u);
            // the cyclic order as four (m, n) corner pairs of four bits each, then rotated to start at the smallest key
            const unsigned e0 = (unsigned)(i << 2 | k), e1 = (unsigned)(i << 2 | l), e2 = (unsigned)(j << 2 | l), e3 = (unsigned)(j << 2 | k);
            unsigned cyc = flip ? (e0 | e3 << 4 | e2 << 8 | e1 << 12) : (e0 | e1 << 4 | e2 << 8 | e3 << 12);
            int r = 0;
            long long best = tet_edge_key(vol, cell, codes, (int)(cyc & 15u));
#pragma unroll
            for (int n = 1; n < 4; ++n) {
                const long long key = tet_edge_key(vol, cell, codes, (int)((cyc >> (4 * n)) & 15u));
                if (key < best) {
                    best = key;
                    r = n;
                }
            }
            cyc = ((cyc | cyc << 16) >> (4 * r)) & 0xFFFFu;
            const Vtx q0 = tet_edge(vol, cell, codes, (int)((cyc >> 2) & 3u), (int)(cyc & 3u));
            const Vtx q1 = tet_edge(vol, cell, codes, (int)((cyc >> 6) & 3u), (int)((cyc >> 4) & 3u));
            const Vtx q2 = tet_edge(vol, cell, codes, (int)((cyc >> 10) & 3u), (int)((cyc >> 8) & 3u));
            const Vtx q3 = tet_edge(vol, cell, codes, (int)((cyc >> 14) & 3u), (int)((cyc >> 12) & 3u));
            put_triangle(T, T_cap, q0, q1, q2, vertices, colors, keys);
            put_triangle(T + 1, T_cap, q0, q2, q3, vertices, colors, keys);
            T += 2;
        }
    }
}

// ---- host checks ----
bool dims_ok(int32_t Gx, int32_t Gy, int32_t Gz)
{
    return Gx >= 1 && Gy >= 1 && Gz >= 1 && Gx <= GSR_TSDF_MAX_DIM && Gy <= GSR_TSDF_MAX_DIM && Gz <= GSR_TSDF_MAX_DIM &&
           (int64_t)Gx * Gy * Gz <= (int64_t)GSR_TSDF_MAX_VOXELS;
}
bool volume_ok(const GsrTsdfVolume &v)
{
    return dims_ok(v.Gx, v.Gy, v.Gz) && isfinite(v.origin[0]) && isfinite(v.origin[1]) && isfinite(v.origin[2]) && isfinite(v.voxel_size) &&
           v.voxel_size > 0.0f;
}
bool volume_aligned(const GsrTsdfVolume &v) { return gsr_aligned16(v.tsdf) && gsr_aligned16(v.weight) && gsr_aligned16(v.color); }
bool positive_or_inf(float x) { return x > 0.0f; } // a NaN fails; +Inf passes
VolK vol_k(const GsrTsdfVolume &v) { return VolK{v.Gx, v.Gy, v.Gz, v.voxel_size, {v.origin[0], v.origin[1], v.origin[2]}, v.tsdf, v.weight, v.color}; }
int64_t cells_of(int32_t Gx, int32_t Gy, int32_t Gz) { return (int64_t)(Gx - 1) * (Gy - 1) * (Gz - 1); }
int64_t groups_of(int32_t Gx, int32_t Gy, int32_t Gz)
{
    const int64_t g = gsr_div_up(cells_of(Gx, Gy, Gz), GC);
    return g < 1 ? 1 : g;
}
bool view_ok(const GsrTsdfView &q)
{
    if (!gsr_image_dims_ok(q.W, q.H) || q.W > GSR_TSDF_MAX_SIDE || q.H > GSR_TSDF_MAX_SIDE) return false; // (float)W and (float)H are exact
    if (!(isfinite(q.tan_fovx) && isfinite(q.tan_fovy) && q.tan_fovx > 0.0f && q.tan_fovy > 0.0f && isfinite(q.w_obs) && q.w_obs > 0.0f)) return false;
    for (int k = 0; k < 16; ++k)
        if (!isfinite(q.view[k])) return false;
    return true;
}

} // namespace

extern "C" {

size_t gsr_mesh_workspace_bytes(int32_t Gx, int32_t Gy, int32_t Gz)
{
    if (!dims_ok(Gx, Gy, Gz)) return 0;
    const int64_t groups = groups_of(Gx, Gy, Gz);
    return gsr_align(4 * (size_t)groups) + gsr_align(8 * (size_t)gsr_div_up(groups, SG));
}

int gsr_tsdf_reset(const GsrTsdfVolume *volume, void *stream)
{
    if (!volume || !volume->tsdf || !volume->weight) return GSR_E_NULL;
    if (!volume_ok(*volume)) return GSR_E_DIMS;
    if (!volume_aligned(*volume)) return GSR_E_ALIGN;
    const int64_t nvox = (int64_t)volume->Gx * volume->Gy * volume->Gz;
    hipLaunchKernelGGL(tsdf_reset_kernel, dim3((unsigned)gsr_div_up(nvox, NT)), dim3(NT), 0, (hipStream_t)stream, vol_k(*volume), (uint32_t)nvox);
    return gsr_done();
}

int gsr_tsdf_integrate(const GsrTsdfVolume *volume, int32_t V, const GsrTsdfView *views, float trunc, float depth_max, float w_max, void *stream)
{
    if (!volume || !volume->tsdf || !volume->weight || !views) return GSR_E_NULL;
    for (int32_t k = 0; k < V; ++k)
        if (!views[k].depth) return GSR_E_NULL;
    if (!volume_ok(*volume) || V < 1 || !(isfinite(trunc) && trunc > 0.0f) || !positive_or_inf(depth_max) || !positive_or_inf(w_max)) return GSR_E_DIMS;
    for (int32_t k = 0; k < V; ++k)
        if (!view_ok(views[k])) return GSR_E_DIMS;
    if (!volume_aligned(*volume)) return GSR_E_ALIGN;
    for (int32_t k = 0; k < V; ++k)
        if (!gsr_aligned16(views[k].depth) || !gsr_aligned16(views[k].color)) return GSR_E_ALIGN;
    const int64_t nvox = (int64_t)volume->Gx * volume->Gy * volume->Gz;
    const VolK vol = vol_k(*volume);
    for (int32_t first = 0; first < V; first += VPL) {
        const int nv = V - first < VPL ? V - first : VPL;
        ViewBatch batch = {};
        for (int k = 0; k < nv; ++k) batch.v[k] = views[first + k];
        hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)gsr_div_up(nvox, NT)), dim3(NT), 0, (hipStream_t)stream, vol, (uint32_t)nvox, batch, nv, trunc,
                           depth_max, w_max);
    }
    return gsr_done();
}

int gsr_tsdf_depth(const float *Dinv, const float *final_T, int32_t W, int32_t H, float alpha_min, float *z_out, void *stream)
{
    if (!Dinv || !final_T || !z_out) return GSR_E_NULL;
    if (!gsr_image_dims_ok(W, H) || !isfinite(alpha_min)) return GSR_E_DIMS;
    if (!gsr_aligned16(Dinv) || !gsr_aligned16(final_T) || !gsr_aligned16(z_out)) return GSR_E_ALIGN;
    const int n = W * H;
    hipLaunchKernelGGL(tsdf_depth_kernel, dim3((unsigned)gsr_div_up(n, NT)), dim3(NT), 0, (hipStream_t)stream, Dinv, final_T, n, alpha_min, z_out);
    return gsr_done();
}

int gsr_mesh_count(const GsrTsdfVolume *volume, float min_weight, void *workspace, size_t workspace_bytes, int64_t *total, void *stream)
{
    if (!volume || !volume->tsdf || !volume->weight || !workspace || !total) return GSR_E_NULL;
    if (!volume_ok(*volume) || !positive_or_inf(min_weight)) return GSR_E_DIMS;
    if (!volume_aligned(*volume) || !gsr_aligned16(workspace) || ((uintptr_t)total & 7u) != 0) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_mesh_workspace_bytes(volume->Gx, volume->Gy, volume->Gz)) return GSR_E_WORKSPACE;
    const int64_t groups = groups_of(volume->Gx, volume->Gy, volume->Gz), runs = gsr_div_up(groups, SG);
    int32_t *cnt = static_cast<int32_t *>(workspace);
    long long *sums = reinterpret_cast<long long *>(static_cast<char *>(workspace) + gsr_align(4 * (size_t)groups));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)groups), dim3(NT), 0, s, vol_k(*volume), (uint32_t)cells_of(volume->Gx, volume->Gy, volume->Gz),
                       min_weight, cnt);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3((unsigned)runs), dim3(NT), 0, s, cnt, (uint32_t)groups, sums);
    hipLaunchKernelGGL(mesh_scan_top_kernel, dim3(1), dim3(NT), 0, s, sums, (int)runs, reinterpret_cast<long long *>(total));
    return gsr_done();
}

int gsr_mesh_emit(const GsrTsdfVolume *volume, float min_weight, const void *workspace, size_t workspace_bytes, int64_t T_cap, float *vertices,
                  float *colors, int64_t *keys, void *stream)
{
    if (!volume || !volume->tsdf || !volume->weight || !workspace || !vertices || !keys) return GSR_E_NULL;
    if (!volume_ok(*volume) || !positive_or_inf(min_weight) || T_cap < 0) return GSR_E_DIMS;
    if (!volume_aligned(*volume) || !gsr_aligned16(workspace) || !gsr_aligned16(vertices) || !gsr_aligned16(colors) || !gsr_aligned16(keys)) return GSR_E_ALIGN;
    if (workspace_bytes < gsr_mesh_workspace_bytes(volume->Gx, volume->Gy, volume->Gz)) return GSR_E_WORKSPACE;
    const int64_t groups = groups_of(volume->Gx, volume->Gy, volume->Gz);
    const int32_t *cnt = static_cast<const int32_t *>(workspace);
    const long long *sums = reinterpret_cast<const long long *>(static_cast<const char *>(workspace) + gsr_align(4 * (size_t)groups));
    hipLaunchKernelGGL(mesh_emit_kernel, dim3((unsigned)groups), dim3(NT), 0, (hipStream_t)stream, vol_k(*volume),
                       (uint32_t)cells_of(volume->Gx, volume->Gy, volume->Gz), min_weight, cnt, sums, (long long)T_cap, vertices, colors,
                       reinterpret_cast<long long *>(keys));
    return gsr_done();
}

} // extern "C"
