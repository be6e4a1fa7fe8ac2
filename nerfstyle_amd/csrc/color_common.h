// What the colour-transfer passes share (color_match.hip: one transform for all rows; color_regions.hip: one per region):
// the launch shape of the moment pass, the fp64 accumulation of a row and the f32 fma chain of the map, written once so that
// both files compute the same bits.
#pragma once
#include "fixed_sum.h"

#define CM_BLOCK 256
#define CM_WAVES (CM_BLOCK / 64)
#define CM_UNITS_PER_THREAD 4      // moments: units a thread is sized for before the grid reaches its cap
#define CM_MAX_BLOCKS 2048         // 256 CUs x 8 blocks

// ---- moments -------------------------------------------------------------------------------------------------------------------
// A unit is one row (stride 4: one float4) or a group of four consecutive rows (stride 3: three float4 when aligned; the last
// group of n may hold fewer rows).  The grid depends on the unit count alone.
static inline uint32_t cm_moment_blocks(uint64_t units) {
    uint64_t b = (units + (uint64_t)CM_BLOCK * CM_UNITS_PER_THREAD - 1) / ((uint64_t)CM_BLOCK * CM_UNITS_PER_THREAD);
    if (b > CM_MAX_BLOCKS) b = CM_MAX_BLOCKS;
    return b == 0 ? 1u : (uint32_t)b;
}
static inline uint64_t cm_moment_units(uint64_t n, uint32_t stride) { return stride == 4 ? n : (n + 3) / 4; }

struct CmAcc {
    double s[9];                   // r, g, b, rr, rg, rb, gg, gb, bb
};

__device__ __forceinline__ void cm_add(CmAcc &a, float rf, float gf, float bf) {
    const double r = rf, g = gf, b = bf;      // the products of two converted f32 are exact in fp64
    a.s[0] += r; a.s[1] += g; a.s[2] += b;
    a.s[3] += r * r; a.s[4] += r * g; a.s[5] += r * b;
    a.s[6] += g * g; a.s[7] += g * b; a.s[8] += b * b;
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------
struct CmTf {
    float m[3][4];                 // rows 0..2 of the [4,4] transform
};

__device__ __forceinline__ CmTf cm_load_tf(const float *tf) {
    CmTf t;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 4; k++) t.m[c][k] = tf[c * 4 + k];
    return t;
}

__device__ __forceinline__ void cm_map(const CmTf &t, int clamp, float &r, float &g, float &b) {
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = fmaf(t.m[c][2], b, fmaf(t.m[c][1], g, fmaf(t.m[c][0], r, t.m[c][3])));
        o[c] = clamp ? fminf(fmaxf(v, 0.0f), 1.0f) : v;
    }
    r = o[0]; g = o[1]; b = o[2];
}
