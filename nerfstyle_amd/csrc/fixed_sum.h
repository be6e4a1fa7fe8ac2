// Fixed-order sums and scans over a wave and a block, written once.
//
// The contract of every sum here: no atomics, a fixed order of additions, so the same inputs give the same bits on every call.
//   wave    an xor butterfly over the 64 lanes, offsets 32, 16, 8, 4, 2, 1: every lane ends with the wave's sum
//   block   each wave's sum through LDS, then the waves added in ascending order onto +0.0 (never onto the first wave's sum:
//           a block whose values are all -0.0 sums to +0.0)
// A kernel that sums over more than one block writes one partial per block and adds them in a second launch: thread t of one
// block adds partials t, t + blockDim, ... in that order, then the block sum.
//
// The block sum is two steps, because some callers want every sum on thread 0 and others sum k on thread k:
//   nsr_block_sum_stage(v, red)        every thread of the block calls it: butterfly, lane 0 of wave w writes red[k][w], barrier
//   nsr_block_sum_col<WAVES>(red[k])   any thread, after it: 0 + red[k][0] + red[k][1] + ...
// The caller owns `red` (a __shared__ array of its kernel).  Staging into the same array a second time needs a barrier after
// the last nsr_block_sum_col of the first.  A block that leaves before the stage leaves as a whole.
//
// The scan is the inclusive __shfl_up scan over a wave; its callers carry the waves' totals through LDS themselves.  It is
// used on integers only, where any order is exact.
#pragma once
#include "nsr_common.h"

template <typename T>
__device__ __forceinline__ T nsr_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int WAVES, typename T>
__device__ __forceinline__ void nsr_block_sum_stage(T v, T (&red)[WAVES]) {
    v = nsr_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
}

// NV values: the same butterfly for each, the NV shuffles of an offset side by side (they do not wait for one another)
template <int NV, int WAVES, typename T>
__device__ __forceinline__ void nsr_block_sum_stage(const T (&v)[NV], T (&red)[NV][WAVES]) {
    T s[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) s[k] = v[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NV; k++) s[k] += __shfl_xor(s[k], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; k++) red[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
}

template <int WAVES, typename T>
__device__ __forceinline__ T nsr_block_sum_col(const T *col) {
    T s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) s += col[w];
    return s;
}

// __shfl_up of a pair of u32 side by side
__device__ __forceinline__ uint2 nsr_shfl_up(uint2 v, int off) { return make_uint2(__shfl_up(v.x, off, 64), __shfl_up(v.y, off, 64)); }
template <typename T>
__device__ __forceinline__ T nsr_shfl_up(T v, int off) { return __shfl_up(v, off, 64); }

// inclusive scan over the wave: lane l ends with v of lanes 0..l (u32, u64, uint2)
template <typename T>
__device__ __forceinline__ T nsr_wave_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = nsr_shfl_up(v, off);
        if (lane >= off) v += up;
    }
    return v;
}
