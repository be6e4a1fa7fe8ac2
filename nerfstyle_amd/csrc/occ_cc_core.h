// The edges of the occupancy grid's cell graph (include/nsr.h, "Occupancy components"), written once for the device
// (occ_components.hip) and for the host (tests/occ_cc_host.cpp runs it from many threads): which occupied cells an occupied
// cell is joined to, read from the bitfield alone, and the union of those pairs through uf_core.h.
//
// Cell id u = cas * H^3 + morton(ix, iy, iz); cell u is occupied iff bit (u & 7) of byte (u >> 3) is set.  One byte is the 8
// cells of one 2x2x2 Morton block: bit j holds the cell at (2 bx + (j & 1), 2 by + ((j >> 1) & 1), 2 bz + (j >> 2)), and the
// block's own index inside its cascade is morton(bx, by, bz).  Every edge is owned by its LOWER end along its axis: a cell
// names its +x, +y and +z neighbours only, which lie in its own byte (the coordinate's low bit is 0) or in the byte of the
// next block along that axis (the low bit is 1).  No edge leaves [0, H) and none leaves the cascade.
#pragma once
#include "uf_core.h"

// x -> its bits at every third place (H <= 512: 9 bits and more are kept), and back
UF_FN uint32_t occ_cc_spread(uint32_t v) {
    v = (v | (v << 16)) & 0xFF0000FFu;
    v = (v | (v << 8)) & 0x0F00F00Fu;
    v = (v | (v << 4)) & 0xC30C30C3u;
    v = (v | (v << 2)) & 0x49249249u;
    return v;
}
UF_FN uint32_t occ_cc_compact(uint32_t x) {
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xC30C30C3u;
    x = (x | (x >> 4)) & 0x0F00F00Fu;
    x = (x | (x >> 8)) & 0xFF0000FFu;
    x = (x | (x >> 16)) & 0x0000FFFFu;
    return x;
}
UF_FN uint32_t occ_cc_morton(uint32_t x, uint32_t y, uint32_t z) {
    return occ_cc_spread(x) | (occ_cc_spread(y) << 1) | (occ_cc_spread(z) << 2);
}

// One bitfield byte with what its edges need: the id of its first cell, its own bits, and per axis the first cell id and the
// bits of the next block along +x, +y, +z (bits 0 where the block lies at the grid's face: nothing is joined across it).
struct OccCcBlock {
    uint32_t base, self;
    uint32_t nbase[3], nbits[3];
};

// Byte n of the bitfield (n < C * H^3 / 8).  An empty byte owns no edge, so its neighbours are not read.
UF_FN OccCcBlock occ_cc_block(const uint8_t *bitfield, uint32_t H, uint32_t n) {
    OccCcBlock b;
    b.base = n * 8u;
    b.self = bitfield[n];
    const uint32_t bytes_per_cas = H * H * H / 8u, half = H / 2u;
    const uint32_t first = n / bytes_per_cas * bytes_per_cas, m = n - first;       // the cascade's first byte, the block's index
    const uint32_t at[3] = {occ_cc_compact(m), occ_cc_compact(m >> 1), occ_cc_compact(m >> 2)};
    for (int a = 0; a < 3; a++) {
        b.nbase[a] = 0u, b.nbits[a] = 0u;
        if (b.self == 0u || at[a] + 1u >= half) continue;
        const uint32_t nn = first + occ_cc_morton(at[0] + (a == 0), at[1] + (a == 1), at[2] + (a == 2));
        b.nbase[a] = nn * 8u;
        b.nbits[a] = bitfield[nn];
    }
    return b;
}

// The partners of the block's occupied cell j (0..7): the ids of its occupied +x, +y, +z neighbours -> how many (0..3)
UF_FN uint32_t occ_cc_partners(const OccCcBlock &b, uint32_t j, uint32_t out[3]) {
    uint32_t k = 0;
    for (uint32_t a = 0; a < 3; a++) {
        const uint32_t bit = 1u << a;
        if (!(j & bit)) {
            if ((b.self >> (j | bit)) & 1u) out[k++] = b.base + (j | bit);
        } else {
            if ((b.nbits[a] >> (j & ~bit)) & 1u) out[k++] = b.nbase[a] + (j & ~bit);
        }
    }
    return k;
}

// Unites every occupied cell of the block with its partners.  parent[] as uf_core.h wants it: parent[u] = u at every occupied
// cell before the first union.  Unoccupied cells are never read or written through parent[].
UF_FN void occ_cc_unite_block(uint32_t *parent, const OccCcBlock &b) {
    for (uint32_t j = 0; j < 8; j++) {
        if (!((b.self >> j) & 1u)) continue;
        uint32_t partner[3];
        const uint32_t k = occ_cc_partners(b, j, partner);
        for (uint32_t i = 0; i < k; i++) uf_unite(parent, b.base + j, partner[i]);
    }
}
