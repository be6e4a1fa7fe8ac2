// Per-frame sums over the segments of a mixed-frame batch (S segments of K rays, segment s names frame seg_frame[s]), shared by
// the pose backward (frame_batch.hip, 12 columns), the lens backward (lens.hip, 18) and the exposure gradient (composite.hip, 3).
// Every one is three parts over a workspace of partials [S][B][NV] f64, B = seg_blocks(K):
//   K <  SEG_THREAD_K   a thread per segment walks its K rays in order and writes the segment's NV sums (B = 1).  K = 1,
//                       per-ray frames, is S threads with one ray each.
//   K >= SEG_THREAD_K   block s * B + b takes rays b * 256 + t, strided by B * 256, of segment s: per thread in that order,
//                       then the block sum of fixed_sum.h; B = ceil(K / 256) capped at SEG_MAX_BLOCKS
//   seg_frame_sum       a wave per output row walks the segments in ascending s and adds the partials of those it picks
// A segment naming no frame in [0, F) writes no partial and none of it is read; a frame no segment names meets no add and gets
// +0.0.  No atomics, no counters; every partial read was written earlier in the same call.  The per-ray term is the caller's.
#pragma once
#include "fixed_sum.h"

#define SEG_BLOCK 256                    // threads of a block-per-segment kernel: seg_blocks counts in it
#define SEG_THREAD_K 64u
#define SEG_MAX_BLOCKS 64u
static inline uint32_t seg_blocks(uint32_t K) {
    if (K < SEG_THREAD_K) return 1u;
    const uint32_t b = nsr_div_up(K, SEG_BLOCK);
    return b < SEG_MAX_BLOCKS ? b : SEG_MAX_BLOCKS;
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
