// Per-frame sums over the segments of a mixed-frame batch (S segments of K rays, segment s names frame seg_frame[s]), shared by
// the pose backward (frame_batch.hip, 12 columns), the lens backward (lens.hip, 18) and the exposure gradient (composite.hip, 3).
// Every one is three parts over a workspace of partials [S][B][NV] f64, B = seg_blocks(K):
//   K <  SEG_THREAD_K   a thread per segment walks its K rays in order and writes the segment's NV sums (B = 1).  K = 1,
//                       per-ray frames, is S threads with one ray each.
//   K >= SEG_THREAD_K   block s * B + b takes rays b * 256 + t, strided by B * 256, of segment s: per thread in that order,
//                       then the block sum of fixed_sum.h; B = ceil(K / 256) capped at SEG_MAX_BLOCKS
//   seg_frame_sum       a wave per output row walks the segments in ascending s and adds the partials of those it picks
// A segment naming no frame in [0, F) writes no partial and none of it is read; a frame no segment names meets no add and gets
// +0.0.  No atomics, no counters; every partial read was written earlier in the same call.
//
// The first two parts are seg_sum_thread and seg_sum_block, each the whole body of a kernel of SEG_BLOCK threads that the
// caller launches through seg_sum_launch.  What is summed is the caller's: make_term(f, n0), called once a thread knows that
// its segment names frame f in [0, F) and starts at ray n0 = s * K, builds what is constant over the segment (a rotation, a lens
// in fp64, a pointer to the segment's rows) and returns term(k, acc), which adds the NV values of the segment's ray k, ray
// n0 + k of the batch, to acc.
#pragma once
#include "fixed_sum.h"

#define SEG_BLOCK 256                    // threads of both kernels: seg_blocks counts in it
#define SEG_THREAD_K 64u
#define SEG_MAX_BLOCKS 64u
static inline uint32_t seg_blocks(uint32_t K) {
    if (K < SEG_THREAD_K) return 1u;
    const uint32_t b = nsr_div_up(K, SEG_BLOCK);
    return b < SEG_MAX_BLOCKS ? b : SEG_MAX_BLOCKS;
}

// what the host checks before it launches a segment sum over N = S * K rays: 32-bit ray and block indices, fp64 partials
static inline bool seg_sum_ok(uint64_t N, uint32_t S, uint32_t K, const void *workspace) {
    return N <= 0xffffffffull && (uint64_t)S * seg_blocks(K) <= 0x7fffffffull && ((uintptr_t)workspace & 7u) == 0;
}

// part one or part two, by K: two kernels of the same arguments whose bodies are seg_sum_thread and seg_sum_block
template <typename... Params, typename... Args>
static inline void seg_sum_launch(void (*thread)(Params...), void (*block)(Params...), uint32_t S, uint32_t K, hipStream_t stream,
                                  Args... args) {
    if (K < SEG_THREAD_K) hipLaunchKernelGGL(thread, dim3(nsr_div_up(S, SEG_BLOCK)), dim3(SEG_BLOCK), 0, stream, args...);
    else hipLaunchKernelGGL(block, dim3(S * seg_blocks(K)), dim3(SEG_BLOCK), 0, stream, args...);
}

// thread s: the K rays of segment s in order, its NV sums to partials[s]
template <int NV, typename MakeTerm>
__device__ __forceinline__ void seg_sum_thread(const int32_t *__restrict__ seg_frame, uint32_t F, uint32_t S, uint32_t K,
                                               double *__restrict__ partials, MakeTerm make_term) {
    const uint32_t s = blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (s >= S) return;
    const uint32_t f = (uint32_t)seg_frame[s];
    if (f >= F) return;
    const auto term = make_term(f, (size_t)s * K);
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; c++) acc[c] = 0.0;
    for (uint32_t k = 0; k < K; k++) term(k, acc);
#pragma unroll
    for (int c = 0; c < NV; c++) partials[(size_t)s * NV + c] = acc[c];
}

// block s * B + b: rays b * 256 + t, strided by B * 256, of segment s, then the block sum; thread c writes sum c to
// partials[blockIdx.x].  `red` is the kernel's LDS (the rule of fixed_sum.h).
template <int NV, typename MakeTerm>
__device__ __forceinline__ void seg_sum_block(const int32_t *__restrict__ seg_frame, uint32_t F, uint32_t K, uint32_t B,
                                              double *__restrict__ partials, double (&red)[NV][SEG_BLOCK / 64], MakeTerm make_term) {
    const uint32_t s = blockIdx.x / B, b = blockIdx.x - s * B;
    const uint32_t f = (uint32_t)seg_frame[s];
    if (f >= F) return;                                       // the whole block: nobody waits at the block sum's barrier
    const auto term = make_term(f, (size_t)s * K);
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; c++) acc[c] = 0.0;
    for (uint32_t k = b * SEG_BLOCK + threadIdx.x; k < K; k += B * SEG_BLOCK) term(k, acc);
    nsr_block_sum_stage(acc, red);
    if (threadIdx.x < NV) partials[(size_t)blockIdx.x * NV + threadIdx.x] = nsr_block_sum_col<SEG_BLOCK / 64>(red[threadIdx.x]);
}

// One wave: the segments in ascending s, 64 at a time (a ballot of picks(seg_frame[s]), then the set bits from the lowest);
// for a picked segment, lane l < ncol adds column col + l of its B partials (rows of `stride` doubles) in order and then that
// sum to its own.  Returns the lane's sum; lanes from ncol on read nothing and return 0.
template <typename Picks>
__device__ __forceinline__ double seg_frame_sum(const int32_t *__restrict__ seg_frame, uint32_t S, uint32_t B,
                                                const double *__restrict__ partials, uint32_t stride, uint32_t col, uint32_t ncol,
                                                Picks picks) {
    const uint32_t lane = threadIdx.x;
    double acc = 0.0;
    for (uint32_t base = 0; base < S; base += 64u) {
        const uint32_t mine = base + lane;
        uint64_t named = __ballot(mine < S && picks(seg_frame[mine]));
        while (named) {
            const uint32_t s = base + (uint32_t)__ffsll((long long)named) - 1u;
            named &= named - 1u;
            if (lane < ncol) {
                double t = 0.0;
                for (uint32_t b = 0; b < B; b++) t += partials[((size_t)s * B + b) * stride + col + lane];
                acc += t;
            }
        }
    }
    return acc;
}
