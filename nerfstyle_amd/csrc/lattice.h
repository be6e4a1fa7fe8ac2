// Lattice geometry of the spatially ordered walk, shared by the table scatter (table_scatter.hip: LDS lattices of corner
// GRADIENTS) and the forward (field.hip: LDS lattices of table ROWS).  The order's key is the sample's BLOCK: its encoder input
// quantised to LAT_KEY_BITS bits per axis (nsr_sample_order).  Per level, a lattice of S^3 corners anchored at the cell of the
// origin of the group of 2^shift blocks the walk is in covers every cell a sample of that group can fall into.
#pragma once
#include "nsr_common.h"

constexpr int LAT_KEY_BITS = 10;                     // must match nsr_sample_order's quantisation
constexpr uint32_t LAT_NONE = 0xFFFFFFFFu;

struct LatGeom {
    uint16_t base[16];      // first slot of the level's lattice
    uint8_t S[16];          // corners per axis
    uint8_t shift[16];      // the level's lattice is anchored at the origin of the 2^shift-block group the walk is in
};

// corners per axis of a lattice that covers every cell a group of 2^shift blocks (each 1/1024 wide) can touch on a level:
// the group spans e = res * 2^shift / 1024 cells, i.e. at most floor(e) + 2 of them (exactly e when the cells tile it)
static inline uint32_t lat_corners(uint32_t res, uint32_t shift) {
    const uint64_t span = (uint64_t)res << shift, blocks = 1u << LAT_KEY_BITS;
    const uint32_t cells = (span % blocks == 0) ? (uint32_t)(span / blocks) : (uint32_t)(span / blocks) + 2u;
    return cells + 1u;
}

// Host: lattice geometry.  The walk is in Morton order of the blocks, so the 8 (64, ...) blocks of an aligned group follow
// one another; a level whose cells are larger than a block is anchored at the GROUP's origin as long as that costs no
// lattice slots (a group narrower than a cell still touches at most 2 cells per axis: 3^3 corners) -- its lattice then
// survives the block changes inside the group and is flushed that much less often (bench frame, backward pair: 23.5 ->
// 22.3 ms).  Levels finer than that keep the block as their anchor: paying a 4^3 lattice for a group of two on the levels
// with cells of 1 - 2 blocks was measured and lost (22.7 ms: more slots to scan per flush, more LDS).
// False when a level needs more than 6 corners per axis or the 16 lattices more than max_slots slots (rounded up to 64).
static inline bool lat_geometry(const NsrLevel *lv, LatGeom &g, uint32_t max_slots) {
    uint32_t total = 0;
    for (int l = 0; l < 16; l++) {
        const uint32_t res = lv[l].resolution;
        uint32_t shift = 0, S = lat_corners(res, 0);
        while (shift < (uint32_t)LAT_KEY_BITS && lat_corners(res, shift + 1) <= (S > 3u ? S : 3u)) shift++;   // free
        // (letting the 1, 2 or 3 finest levels pay a larger lattice for a group of 2^3 blocks: bench frame, backward pair
        // 22.14, 22.09, 22.91 ms against 22.2 -- nothing to gain)
        S = lat_corners(res, shift) > S ? lat_corners(res, shift) : S;
        if (S < 2u || S > 6u) return false;
        g.S[l] = (uint8_t)S;
        g.shift[l] = (uint8_t)shift;
        g.base[l] = (uint16_t)total;
        total += S * S * S;
    }
    return ((total + 63u) & ~63u) <= max_slots;
}

#ifdef __HIPCC__
// field_corner_row (field_common.h) restated per corner with the cheap cases taken out (the level is wave-uniform here): a
// power-of-two table is masked, a dense level needs neither 32-bit multiplies (index < 2^19) nor the modulo (index < (res + 1)^3 <= size).
__device__ __forceinline__ uint32_t lat_row(const NsrLevel &lv, uint32_t x, uint32_t y, uint32_t z) {
    if (lv.use_hash) {
        const uint32_t index = x ^ (y * 2654435761u) ^ (z * 805459861u);
        if ((lv.size & (lv.size - 1u)) == 0u) return index & (lv.size - 1u);
        const uint32_t t = __umulhi(lv.magic, index);
        const uint32_t q = (t + ((index - t) >> lv.sh1)) >> lv.sh2;
        return index - q * lv.size;
    }
    return __umul24(x, lv.mul[0]) + __umul24(y, lv.mul[1]) + __umul24(z, lv.mul[2]);
}
#endif
