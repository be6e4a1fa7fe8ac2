// Deterministic stream compaction, shared by surface_nets.hip and mesh_clean.hip: in-block ranks from wave64 ballots, block
// totals scanned level by level, no atomics.  A workgroup of BS_BLOCK threads owns BS_BLOCK consecutive items; an item's output
// slot is its block's scanned offset plus its rank in the block.  The totals are uint2: two counts are ranked side by side.
//   bs_block_rank    exclusive rank of a count (0..3) among the block's threads, and the block's total
//   k_bs_scan        BS_SCAN totals a block, exclusive in place, the block's sum to the next level (the levels are walked on
//                    the host: BsLevels); the top level (one block) writes the grand totals and three caller's words into the
//                    workspace header, and the totals once more to counts_out
//   k_bs_scan_add    adds the scanned level above back into a level
#pragma once
#include "fixed_sum.h"

#define BS_BLOCK 256
#define BS_SCAN 256                      // totals per scan block (one a thread)
#define BS_MAX_LEVELS 4                  // 2^32 items are 2^24 blocks -> 65 536 -> 256 -> 1
#define BS_HEADER_WORDS 8                // total.x, total.y, three caller's words, 0, 0, 0

struct BsLevels {                        // byte offsets from the start of the workspace, each a multiple of 16
    uint32_t levels;
    uint32_t n[BS_MAX_LEVELS];           // entries of level l (n[0]: the counting kernel's blocks)
    uint64_t off[BS_MAX_LEVELS];
    uint64_t end;                        // the first byte after the levels
};

// the header, then the levels of `blocks` block totals
static inline BsLevels bs_levels(uint32_t blocks) {
    BsLevels l;
    uint64_t at = BS_HEADER_WORDS * 4;
    uint32_t n = blocks;
    l.levels = 0;
    for (;;) {
        l.n[l.levels] = n;
        l.off[l.levels] = at;
        at += ((uint64_t)n * 8 + 15) & ~15ull;
        l.levels++;
        if (n <= BS_SCAN) break;
        n = nsr_div_up(n, BS_SCAN);
    }
    l.end = at;
    return l;
}

// lanes below this one in the wave whose bit is set
__device__ __forceinline__ uint32_t bs_below(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// Exclusive rank of `count` (0..3) among the block's threads in thread order, and the block's total.  All threads call it.
__device__ __forceinline__ uint32_t bs_block_rank(uint32_t count, uint32_t *s_wave, uint32_t &total) {
    const unsigned long long b0 = __ballot(count & 1u), b1 = __ballot(count & 2u);
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t rank = bs_below(b0) + 2u * bs_below(b1);
    if ((threadIdx.x & 63) == 0) s_wave[wave] = (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1);
    __syncthreads();
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < BS_BLOCK / 64; w++) {
        const uint32_t t = s_wave[w];
        if (w < wave) rank += t;
        total += t;
    }
    __syncthreads();                                // s_wave is free for the next call
    return rank;
}

// t[0 .. n) in chunks of BS_SCAN: exclusive scan of each chunk in place, the chunk's sum to sums[block]; counts_out (the top
// level only, one block, whose `sums` is the workspace header): the grand totals once more, and `tag` into the header
static __global__ void __launch_bounds__(BS_SCAN) k_bs_scan(uint2 *__restrict__ t, uint32_t n, uint2 *__restrict__ sums,
                                                            uint32_t *__restrict__ counts_out, uint3 tag) {
    __shared__ uint2 s_wave[BS_SCAN / 64];
    const uint32_t i = blockIdx.x * BS_SCAN + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint2 mine = i < n ? t[i] : make_uint2(0u, 0u);
    const uint2 incl = nsr_wave_scan(mine);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint2 before = make_uint2(0u, 0u), total = make_uint2(0u, 0u);
#pragma unroll
    for (uint32_t w = 0; w < BS_SCAN / 64; w++) {
        const uint2 sw = s_wave[w];
        if (w < wave) before.x += sw.x, before.y += sw.y;
        total.x += sw.x, total.y += sw.y;
    }
    if (i < n) t[i] = make_uint2(before.x + incl.x - mine.x, before.y + incl.y - mine.y);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total;
        if (counts_out) {                           // sums is the workspace header: what was counted beside the totals
            counts_out[0] = total.x, counts_out[1] = total.y;
            uint32_t *header = (uint32_t *)sums;
            header[2] = tag.x, header[3] = tag.y, header[4] = tag.z;
        }
    }
}

static __global__ void __launch_bounds__(BS_SCAN) k_bs_scan_add(uint2 *__restrict__ t, uint32_t n, const uint2 *__restrict__ above) {
    const uint32_t i = blockIdx.x * BS_SCAN + threadIdx.x;
    if (i < n) {
        const uint2 a = above[blockIdx.x];
        uint2 v = t[i];
        v.x += a.x, v.y += a.y;
        t[i] = v;
    }
}

// Scans the block totals at level 0 of `ws` (already written) into exclusive offsets; header and counts_out as k_bs_scan says.
static inline void bs_scan_levels(char *ws, const BsLevels &l, uint32_t *counts_out, uint3 tag, hipStream_t st) {
    uint2 *lv[BS_MAX_LEVELS];
    for (uint32_t i = 0; i < l.levels; i++) lv[i] = (uint2 *)(ws + l.off[i]);
    for (uint32_t i = 0; i < l.levels; i++) {
        const bool top = i + 1 == l.levels;         // one block: its sum is the grand total -> header[0..1] and counts_out
        hipLaunchKernelGGL(k_bs_scan, dim3(nsr_div_up(l.n[i], BS_SCAN)), dim3(BS_SCAN), 0, st, lv[i], l.n[i],
                           top ? (uint2 *)ws : lv[i + 1], top ? counts_out : (uint32_t *)nullptr, tag);
    }
    for (uint32_t i = l.levels - 1; i-- > 0;)
        hipLaunchKernelGGL(k_bs_scan_add, dim3(nsr_div_up(l.n[i], BS_SCAN)), dim3(BS_SCAN), 0, st, lv[i], l.n[i], lv[i + 1]);
}
