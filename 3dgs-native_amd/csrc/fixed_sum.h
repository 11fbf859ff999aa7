// fixed_sum.h -- the fixed-order sum ("The fixed-order sum"): the one tree behind every sum that promises the same bits
// every call.  Device code only; like dssim_window.h, everything sits in the including file's anonymous namespace.
//   lane values -> 64-lane butterfly -> four wave sums in LDS -> pairwise() or serial() -> a record per workgroup
//   -> gsr_record_walk in one finishing workgroup -> the same tree again.
#pragma once
#include "gsr_internal.h"

namespace {

constexpr int GSR_SUM_THREADS = 256;                       // a workgroup of the tree: four waves
constexpr int GSR_SUM_WAVES = GSR_SUM_THREADS / GSR_WAVE;

// The four wave sums of NV values, as the accumulator type A, in the caller's LDS.  Any thread may read total k, in one of the
// two orders the kernels were written with; a site names its order and keeps it.  The array is red[wave][k], or red[k][wave]
// (dssim.hip's stats pass, whose thread 0 reads both totals): the caller's declaration says which.
template <class A, int NV, bool WAVE_MAJOR = true>
struct GsrBlockSums {
    const A *red;
    __device__ __forceinline__ A wave(int w, int k) const { return WAVE_MAJOR ? red[w * NV + k] : red[k * GSR_SUM_WAVES + w]; }
    __device__ __forceinline__ A pairwise(int k) const { return (wave(0, k) + wave(1, k)) + (wave(2, k) + wave(3, k)); }
    __device__ __forceinline__ A serial(int k) const { return ((wave(0, k) + wave(1, k)) + wave(2, k)) + wave(3, k); }
};

// The workgroup's sums of s[0 .. NV).  The wave butterfly: partners 32, 16, .. 1 lanes away, in T (float or double: it stays what
// the site has), so every lane ends with the same bits.  Lane 0 of each wave stores its sums to `red` converted to A; a barrier.
// s is left holding the wave sums.  NT is the caller's workgroup size, stated so that it can be checked.
// The values are independent, so the loop nest changes no bit, only the order in which the compiler meets the shuffles: step by
// step across the values, or BY_VALUE, each value's six steps in turn (camera_bwd.hip, whose many values schedule better so).
template <int NT, bool BY_VALUE, bool WAVE_MAJOR, class T, class A, int NV>
__device__ __forceinline__ GsrBlockSums<A, NV, WAVE_MAJOR> gsr_block_sums_in(T (&s)[NV], A *red)
{
    static_assert(NT == GSR_SUM_THREADS, "the tree is four waves of 64");
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
    if constexpr (BY_VALUE) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d, 64);
    } else {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
            for (int k = 0; k < NV; ++k) s[k] += __shfl_xor(s[k], d, 64);
    }
    if ((threadIdx.x & (GSR_WAVE - 1)) == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) red[WAVE_MAJOR ? threadIdx.x / GSR_WAVE * NV + k : k * GSR_SUM_WAVES + threadIdx.x / GSR_WAVE] = (A)s[k];
    __syncthreads();
    return GsrBlockSums<A, NV, WAVE_MAJOR>{red};
}
// The caller's declaration of `red` picks the layout: [GSR_SUM_WAVES][NV] or [NV][GSR_SUM_WAVES].  A new site takes the first and
// the default nest; the other choices exist for the sites that had them.  With NV == 4 the two overloads are ambiguous and the
// call does not compile: no site has four values, and one that does calls gsr_block_sums_in with its layout spelled out.
template <int NT, bool BY_VALUE = false, class T, class A, int NV>
__device__ __forceinline__ GsrBlockSums<A, NV, true> gsr_block_sums(T (&s)[NV], A (&red)[GSR_SUM_WAVES][NV])
{
    return gsr_block_sums_in<NT, BY_VALUE, true>(s, &red[0][0]);
}
template <int NT, bool BY_VALUE = false, class T, class A, int NV>
__device__ __forceinline__ GsrBlockSums<A, NV, false> gsr_block_sums(T (&s)[NV], A (&red)[NV][GSR_SUM_WAVES])
{
    return gsr_block_sums_in<NT, BY_VALUE, false>(s, &red[0][0]);
}
template <int NT, class T, class A>
__device__ __forceinline__ GsrBlockSums<A, 1> gsr_block_sum(T v, A (&red)[GSR_SUM_WAVES][1]) // one value
{
    T s[1] = {v};
    return gsr_block_sums<NT>(s, red);
}

// The record walk of the finishing workgroup: thread t's sums of the first NV values of records t, t + 256, ... added in ascending
// order onto +0.  A record is STRIDE values of T; `part` is 16-byte aligned (it is a workspace), so whole-16-byte records load as
// such.  The sums come back by value: as an in-out array argument the same loop cost exposure.hip's finish a register.
template <class T, int NV>
struct GsrLaneSums {
    T v[NV];
};
template <int NV, int STRIDE, class T>
__device__ __forceinline__ GsrLaneSums<T, NV> gsr_record_walk(const T *__restrict__ part, int n)
{
    static_assert(STRIDE >= NV, "a record holds the NV values");
    constexpr int BYTES = STRIDE * (int)sizeof(T), ALIGN = BYTES % 16 == 0 ? 16 : BYTES % 8 == 0 ? 8 : (int)sizeof(T);
    GsrLaneSums<T, NV> s = {};
    for (int r = threadIdx.x; r < n; r += GSR_SUM_THREADS) {
        const T *rec = static_cast<const T *>(__builtin_assume_aligned(part + (size_t)STRIDE * r, ALIGN));
#pragma unroll
        for (int k = 0; k < NV; ++k) s.v[k] += rec[k];
    }
    return s;
}

// Where a finishing launch leaves its totals: NOUT = 1, one array of NV words, thread k writes word k; NOUT = NV, one pointer per
// word, thread 0 writes them all.
template <int NOUT>
struct GsrSumOut {
    float *p[NOUT];
};

// one workgroup: the walk over n float records, the tree, the pairwise totals into the caller's words
template <int NV, int STRIDE, int NOUT>
__global__ __launch_bounds__(GSR_SUM_THREADS) void gsr_finish_kernel(const float *__restrict__ part, int n, GsrSumOut<NOUT> out)
{
    static_assert(NOUT == 1 || NOUT == NV, "one array, or one pointer per word");
    __shared__ float s_red[GSR_SUM_WAVES][NV];
    GsrLaneSums<float, NV> s = gsr_record_walk<NV, STRIDE>(part, n);
    const GsrBlockSums<float, NV> b = gsr_block_sums<GSR_SUM_THREADS>(s.v, s_red);
    if constexpr (NOUT == 1) {
        if (threadIdx.x < NV) out.p[0][threadIdx.x] = b.pairwise(threadIdx.x);
    } else {
        if (threadIdx.x == 0)
#pragma nounroll   // one total at a time: unrolled, the wave sums of all NV are read at once, into more registers than the sites had
            for (int k = 0; k < NV; ++k) *out.p[k] = b.pairwise(k);
    }
}

} // namespace
