// Philox4x32-10 (Salmon et al., SC'11): counter-based, so a draw depends only on (seed, sequence, index) -- identical on every
// rank without communication.  Shared by the occupancy update (occupancy.hip) and the mixed-frame batch draw (frame_batch.hip).
#pragma once
#include "nsr_common.h"

struct OccU4 { uint32_t x, y, z, w; };
__device__ __forceinline__ OccU4 occ_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return OccU4{c0, c1, c2, c3};
}
// uniform in [0, 1) with 24 random bits (what torch.rand gives a float32)
__device__ __forceinline__ float occ_u01(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }
