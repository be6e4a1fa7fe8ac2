// Shared pieces of the fused field kernels (forward: field.hip, backward: field_bwd.hip, inference render: render_infer.hip).
#pragma once
#include <hip/hip_fp16.h>

#include <type_traits>

#include "mfma_tiles.h"

// ---- parameter layout (floats) inside mlp_params: density, color1, color2, class ------------
constexpr int P_D1 = 0;        // 64 x 32
constexpr int P_D2 = 2048;     // 16 x 64 (row 0 = logit)
constexpr int P_C1A = 3072;    // 64 x 32
constexpr int P_C1B = 5120;    // 16 x 64
constexpr int P_R1 = 6144;     // 64 x 16
constexpr int P_R2 = 7168;     // 64 x 64
constexpr int P_R3 = 11264;    // 16 x 64 (rows 0..2 = rgb)
constexpr int P_K1 = 12288;    // 64 x 32
constexpr int P_K2 = 14336;    // 16 x 64 (rows 0..nc-1 = classes)
constexpr int P_TOTAL = 15360;
// view-dependent models only (the *_dirs entry points): color2's first layer is 64 x 32 = [color1 | SH]; its SH columns are
// appended so that every offset above stays where it is
constexpr int P_SH = 15360;    // 64 x 16
constexpr int P_TOTAL_DIRS = 16384;

// ---- forward LDS image (units: shorts).  frag32 = 512 shorts, frag16 = 256 shorts ----------
constexpr int FW_D1 = 0, FW_D2 = 2048, FW_C1A = 3072, FW_C1B = 5120, FW_K1 = 6144, FW_K2 = 8192, FW_R2 = 9216,
              FW_R3 = 13312, FW_R1 = 14336, FW_TOTAL = 15360, FW_SIGMA_TOTAL = 3072;
// with directions FW_R1, the image's last block, is four frag32 (K = 32: color1 output | SH coefficients) instead of four frag16
constexpr int FW_TOTAL_DIRS = 16384;
template <bool DIRS> constexpr int FW_IMAGE = DIRS ? FW_TOTAL_DIRS : FW_TOTAL;
// class logits live in rows 3..3+nc-1 of their output tile so that (row == output channel) and
// lane (s,g) stores channels 4g..4g+3 of rgbs[m, :] as one 16-byte piece.
constexpr int CLASS_ROW_SHIFT = 3;

struct FieldArgs {
    const void *tables;
    const float *params;
    const float *xyzs;
    const int32_t *m_dev;
    uint32_t M;
    float *sigmas;
    float *rgbs;
    void *feats;          // optional [ntiles][64 lanes][2] x 16 B: (xd, xc) B fragments per lane
    const uint32_t *perm; // optional [M]: tile t works on samples perm[16t .. 16t+15] (nsr_sample_order); feats stay tile-major
    float bmin[3], bsize[3];
    float density_scale;
    uint32_t C_ch;
    uint32_t tiles_per_block;
    uint32_t fast_levels;     // bit l: level l is hashed and its size is a power of two
    NsrLevel lv[16];
};
// argument of the direction-taking forward kernels: dirs [M,3], indexed like xyzs
struct FieldDirsArgs : FieldArgs {
    const float *dirs;
};
template <bool DIRS> using FieldArgsOf = std::conditional_t<DIRS, FieldDirsArgs, FieldArgs>;
__device__ __forceinline__ const float *field_dirs_of(const FieldArgs &) { return nullptr; }
__device__ __forceinline__ const float *field_dirs_of(const FieldDirsArgs &a) { return a.dirs; }

// color2's first layer with directions, four frag32: the lane that holds rows 4g..4g+3 of the color1 output tile evaluates SH
// coefficients 4g..4g+3 (field_sh4), so its B fragment is cat(color1 rows, SH coefficients) and element e of lane (r, g) of
// the A fragment is W[row][4g + e] for e < 4 and Wsh[row][4g + e - 4] for e >= 4 (column 8g + e of the instruction's k axis).
template <int CD>
__device__ __forceinline__ void field_build_r1_dirs(short *lds, const float *__restrict__ w, const float *__restrict__ wsh) {
    for (int idx = threadIdx.x; idx < 4 * 64 * 8; idx += blockDim.x) {
        const int e = idx & 7, lane = (idx >> 3) & 63, m = idx >> 9;
        const int row = 16 * m + (lane & 15), col = 4 * (lane >> 4) + (e & 3);
        lds[idx] = MM<CD>::cvt((e < 4 ? w : wsh)[row * 16 + col]);
    }
}

template <int CD, bool SIGMA_ONLY, bool DIRS = false>
__device__ __forceinline__ void field_build_fw(short *lds, const float *__restrict__ p) {
    mm_build_frags<CD>(lds + FW_D1, p + P_D1, 64, 32, 4, 32, false, 0, true);
    mm_build_frags<CD>(lds + FW_D2, p + P_D2, 16, 64, 1, 64, false, 0, true);
    if (!SIGMA_ONLY) {
        mm_build_frags<CD>(lds + FW_C1A, p + P_C1A, 64, 32, 4, 32, false, 0, true);
        mm_build_frags<CD>(lds + FW_C1B, p + P_C1B, 16, 64, 1, 64, false, 0, true);
        mm_build_frags<CD>(lds + FW_K1, p + P_K1, 64, 32, 4, 32, false, 0, true);
        mm_build_frags<CD>(lds + FW_K2, p + P_K2, 16, 64, 1, 64, false, CLASS_ROW_SHIFT, true);
        mm_build_frags<CD>(lds + FW_R2, p + P_R2, 64, 64, 4, 64, false, 0, true);
        mm_build_frags<CD>(lds + FW_R3, p + P_R3, 16, 64, 1, 64, false, 0, true);
        if constexpr (DIRS) field_build_r1_dirs<CD>(lds + FW_R1, p + P_R1, p + P_SH);
        else mm_build_frags<CD>(lds + FW_R1, p + P_R1, 64, 16, 4, 16, false, 0, false);
    }
}

// Degree-4 spherical harmonics of a viewing direction, tiny-cuda-nn's SphericalHarmonics encoding: the reference feeds
// u = (d + 1) / 2 and the encoder maps back with 2u - 1, both in fp32.  Returns coefficients 4g .. 4g+3.
__device__ __forceinline__ f4v field_sh4(int g, float d0, float d1, float d2) {
#pragma clang fp contract(off)      // the same bits in every kernel that inlines this
    const float x = 2.0f * ((d0 + 1.0f) / 2.0f) - 1.0f, y = 2.0f * ((d1 + 1.0f) / 2.0f) - 1.0f, z = 2.0f * ((d2 + 1.0f) / 2.0f) - 1.0f;
    const float xx = x * x, yy = y * y, zz = z * z;
    f4v r;
    if (g == 0) {
        r[0] = 0.28209479177387814f;
        r[1] = -0.48860251190291987f * y;
        r[2] = 0.48860251190291987f * z;
        r[3] = -0.48860251190291987f * x;
    } else if (g == 1) {
        r[0] = 1.0925484305920792f * (x * y);
        r[1] = -1.0925484305920792f * (y * z);
        r[2] = 0.94617469575755997f * zz - 0.31539156525251999f;
        r[3] = -1.0925484305920792f * (x * z);
    } else if (g == 2) {
        r[0] = 0.54627421529603959f * (xx - yy);
        r[1] = 0.59004358992664352f * y * (-3.0f * xx + yy);
        r[2] = 2.8906114426405538f * (x * y) * z;
        r[3] = 0.45704579946446572f * y * (1.0f - 5.0f * zz);
    } else {
        r[0] = 0.3731763325901154f * z * (5.0f * zz - 3.0f);
        r[1] = 0.45704579946446572f * x * (1.0f - 5.0f * zz);
        r[2] = 1.4453057213202769f * z * (xx - yy);
        r[3] = 0.59004358992664352f * x * (-xx + 3.0f * yy);
    }
    return r;
}
// the same four coefficients as the upper half of color2's K = 32 B fragment (rounded to the compute type: the MLP contract)
template <int CD>
__device__ __forceinline__ s4v field_sh_frag(const float *__restrict__ dirs, uint32_t m, bool valid, int g) {
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (valid) { d0 = dirs[(size_t)m * 3 + 0]; d1 = dirs[(size_t)m * 3 + 1]; d2 = dirs[(size_t)m * 3 + 2]; }
    return mm_round4<CD, false>(field_sh4(g, d0, d1, d2));
}

// Encoder input of a world position: BBox.normalize (common.py:276-288) then GridEncoder's
// (x + bound) / (2 * bound) with bound = 1 (grid.py:177).  Same op order as the oracle.
__device__ __forceinline__ float field_unit(float x, float mn, float sz) {
#pragma clang fp contract(off)
    const float xn = (x - mn) / sz;
    return (xn + 1.0f) / 2.0f;
}

template <typename TT> struct RowLd;
template <> struct RowLd<float> {
    // one interleaved row = [d0 d1 c0 c1] fp32 = 16 bytes
    static __device__ __forceinline__ float4 full(const float *t, uint32_t row) {
        return reinterpret_cast<const float4 *>(t)[row];
    }
    static __device__ __forceinline__ float2 dens(const float *t, uint32_t row) {
        return reinterpret_cast<const float2 *>(t)[(size_t)row * 2];
    }
    // acc += sum over the 8 corners of w * row (all gathers issued first)
    static __device__ __forceinline__ void accumulate(const float *t, const uint32_t (&rows)[8], const float (&w)[8], float4 &acc) {
        float4 v[8];
#pragma unroll
        for (int idx = 0; idx < 8; idx++) v[idx] = full(t, rows[idx]);
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            acc.x += w[idx] * v[idx].x; acc.y += w[idx] * v[idx].y;
            acc.z += w[idx] * v[idx].z; acc.w += w[idx] * v[idx].w;
        }
    }
};
template <> struct RowLd<_Float16> {
    static __device__ __forceinline__ float4 full(const _Float16 *t, uint32_t row) {
        const h4v v = reinterpret_cast<const h4v *>(t)[row];
        return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    }
    static __device__ __forceinline__ float2 dens(const _Float16 *t, uint32_t row) {
        typedef _Float16 h2v __attribute__((ext_vector_type(2)));
        const h2v v = reinterpret_cast<const h2v *>(t)[(size_t)row * 2];
        return make_float2((float)v[0], (float)v[1]);
    }
    // fp32 accumulation straight from the packed halves: v_fma_mix_f32 widens its f16 operand inside the
    // multiply-add (same value as v_cvt_f32_f16 followed by v_fma_f32: the widening is exact), so the 32
    // conversions per level disappear from a kernel that is VALU-issue-bound half of the time
    static __device__ __forceinline__ void accumulate(const _Float16 *t, const uint32_t (&rows)[8], const float (&w)[8], float4 &acc) {
        uint2 v[8];
#pragma unroll
        for (int idx = 0; idx < 8; idx++) v[idx] = reinterpret_cast<const uint2 *>(t)[rows[idx]];
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "+v"(acc.x) : "v"(w[idx]), "v"(v[idx].x));
            asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(acc.y) : "v"(w[idx]), "v"(v[idx].x));
            asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "+v"(acc.z) : "v"(w[idx]), "v"(v[idx].y));
            asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(acc.w) : "v"(w[idx]), "v"(v[idx].y));
        }
    }
};

// In-range test of an encoder input (gridencoder.cu:107-132: inputs outside [0,1] encode to zeros); NaN -> zeros too
__device__ __forceinline__ bool field_in_unit_cube(float u0, float u1, float u2) {
    return u0 >= 0 && u0 <= 1 && u1 >= 0 && u1 <= 1 && u2 >= 0 && u2 <= 1;
}

// ---- one level of the encoders (gridencoder.cu:134-181, align_corners = True, style = 0: networks/tcnn_nerf.py:26-35) ------
// The helpers below fix an OPERATION ORDER as well as a value: the kernels that inline them sit at register steps (k_field_fwd
// at 125 of 128 VGPRs), and e.g. forming all eight weights before the eight rows costs the forward five registers and a wave
// per SIMD.  After any edit compare tools/kernel_stats.py against the parent (DESIGN.md "Shared encode helpers").

// cell, fractions and the weights' product table of one level: w[idx] = wxy[idx & 3] * wz[idx >> 2] is (wx*wy)*wz, the
// reference's product order (gridencoder.cu:160-175)
__device__ __forceinline__ void field_level_front(const NsrLevel &lv, float u0, float u1, float u2, uint32_t (&c)[3], float (&f)[3],
                                                  float (&wxy)[4], float (&wz)[2]) {
    nsr_grid_locate(u0, lv.resolution, 1, f[0], c[0]);
    nsr_grid_locate(u1, lv.resolution, 1, f[1], c[1]);
    nsr_grid_locate(u2, lv.resolution, 1, f[2], c[2]);
    wxy[0] = (1 - f[0]) * (1 - f[1]); wxy[1] = f[0] * (1 - f[1]); wxy[2] = (1 - f[0]) * f[1]; wxy[3] = f[0] * f[1];
    wz[0] = 1 - f[2]; wz[1] = f[2];
}

// The corner index, written once.  FAST (wave-uniform, from the host's level table): the four levels a call handles, one per
// 16-lane group, are all hashed with a power-of-two size, so row = (x ^ y*P1 ^ z*P2) & (size - 1) -- the value nsr_grid_row
// gives -- without the per-lane hash/dense select and the invariant-divisor modulo.  The y and z products of a cell's two
// planes are formed once per level (field_corner_yz), not once per corner.
template <bool FAST>
__device__ __forceinline__ bool field_corner_yz(const NsrLevel &lv, uint32_t c1, uint32_t c2, uint32_t (&ty)[2], uint32_t (&tz)[2]) {
    const bool hashed = FAST || lv.use_hash != 0;
    const uint32_t mulY = hashed ? 2654435761u : lv.mul[1], mulZ = hashed ? 805459861u : lv.mul[2];
    ty[0] = c1 * mulY; ty[1] = (c1 + 1u) * mulY;
    tz[0] = c2 * mulZ; tz[1] = (c2 + 1u) * mulZ;
    return hashed;
}
// table row of the corner with x coordinate x, y product a and z product b
template <bool FAST>
__device__ __forceinline__ uint32_t field_corner_row(const NsrLevel &lv, bool hashed, uint32_t x, uint32_t a, uint32_t b) {
    if (FAST) return lv.offset + ((x ^ a ^ b) & (lv.size - 1u));
    const uint32_t index = hashed ? (x ^ a ^ b) : (x * lv.mul[0] + a + b);
    const uint32_t t = __umulhi(lv.magic, index);
    const uint32_t q = (t + ((index - t) >> lv.sh1)) >> lv.sh2;
    return lv.offset + (index - q * lv.size);
}

// cell and corner weights of one level
__device__ __forceinline__ void field_level_cell(const NsrLevel &lv, float u0, float u1, float u2, uint32_t (&c)[3], float (&w)[8]) {
    float f[3], wxy[4], wz[2];
    field_level_front(lv, u0, u1, u2, c, f, wxy, wz);
#pragma unroll
    for (uint32_t idx = 0; idx < 8; idx++) w[idx] = wxy[idx & 3] * wz[idx >> 2];
}

// table rows of the eight corners of cell c (corner idx: bit 0 = x, bit 1 = y, bit 2 = z)
template <bool FAST>
__device__ __forceinline__ void field_cell_rows(const NsrLevel &lv, const uint32_t (&c)[3], uint32_t (&rows)[8]) {
    uint32_t ty[2], tz[2];
    const bool hashed = field_corner_yz<FAST>(lv, c[1], c[2], ty, tz);
#pragma unroll
    for (uint32_t idx = 0; idx < 8; idx++) rows[idx] = field_corner_row<FAST>(lv, hashed, c[0] + (idx & 1u), ty[(idx >> 1) & 1], tz[idx >> 2]);
}

// rows and weights of one level.  ONE interleaved loop, not field_level_cell then field_cell_rows: weights-first takes
// k_field_fwd<_Float16, f16, false> from 125 to 130 VGPRs (four waves per SIMD to three) and k_render_infer from 153-155 to 158-159
template <bool FAST>
__device__ __forceinline__ void field_level_rows(const NsrLevel &lv, float u0, float u1, float u2, uint32_t (&rows)[8], float (&w)[8]) {
    float f[3], wxy[4], wz[2];
    uint32_t c[3], ty[2], tz[2];
    field_level_front(lv, u0, u1, u2, c, f, wxy, wz);
    const bool hashed = field_corner_yz<FAST>(lv, c[1], c[2], ty, tz);
#pragma unroll
    for (uint32_t idx = 0; idx < 8; idx++) {
        w[idx] = wxy[idx & 3] * wz[idx >> 2];
        rows[idx] = field_corner_row<FAST>(lv, hashed, c[0] + (idx & 1u), ty[(idx >> 1) & 1], tz[idx >> 2]);
    }
}

// Trilinear interpolation of one level for both encoders
template <typename TT, bool SIGMA_ONLY, bool FAST>
__device__ __forceinline__ float4 field_encode_level(const NsrLevel &lv, const TT *__restrict__ tables, float u0, float u1,
                                                     float u2, bool live) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        uint32_t rows[8];
        float w[8];
        field_level_rows<FAST>(lv, u0, u1, u2, rows, w);
        if (SIGMA_ONLY) {
            float2 v[8];
#pragma unroll
            for (int idx = 0; idx < 8; idx++) v[idx] = RowLd<TT>::dens(tables, rows[idx]);
#pragma unroll
            for (int idx = 0; idx < 8; idx++) { acc.x += w[idx] * v[idx].x; acc.y += w[idx] * v[idx].y; }
        } else {
            RowLd<TT>::accumulate(tables, rows, w, acc);
        }
    }
    return acc;
}

// The lane's level assignment: lane group g runs four calls, call i on level field_lane_level(g, i), so call i covers one level per
// group: {0,2,4,6} {1,3,5,7} {8,10,12,14} {9,11,13,15} (field_call_levels).  A call takes the FAST path when all four are fast.
__device__ __forceinline__ int field_lane_level(int g, int i) { return i == 0 ? 2 * g : i == 1 ? 2 * g + 1 : i == 2 ? 8 + 2 * g : 9 + 2 * g; }
__device__ __forceinline__ uint32_t field_call_levels(int i) { return 0x0055u << ((i & 1) + 8 * (i >> 1)); }
__device__ __forceinline__ bool field_call_is_fast(uint32_t fast_levels, int i) {
    return (fast_levels & field_call_levels(i)) == field_call_levels(i);
}

// fp32 sums of the four levels' gathered 16-bit rows (corners 0..7 in that order) -> the two B fragments
template <int CD>
__device__ __forceinline__ void field_mix_rows(const uint2 (&v)[4][8], const float (&w)[4][8], bool live, s8v &xd, s8v &xc) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
#pragma unroll
            for (int idx = 0; idx < 8; idx++) {
                asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "+v"(a.x) : "v"(w[i][idx]), "v"(v[i][idx].x));
                asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(a.y) : "v"(w[i][idx]), "v"(v[i][idx].x));
                asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "+v"(a.z) : "v"(w[i][idx]), "v"(v[i][idx].y));
                asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(a.w) : "v"(w[i][idx]), "v"(v[i][idx].y));
            }
        }
        xd[2 * i + 0] = MM<CD>::cvt(a.x);
        xd[2 * i + 1] = MM<CD>::cvt(a.y);
        xc[2 * i + 0] = MM<CD>::cvt(a.z);
        xc[2 * i + 1] = MM<CD>::cvt(a.w);
    }
}

// Encodes this lane's four levels; returns the two K=32 B fragments (density, colour).
// BATCH_GATHER (the forward only): all 32 gathers of a lane's four levels in flight before the first is used.
template <typename TT, int CD, bool SIGMA_ONLY, bool BATCH_GATHER = false>
__device__ __forceinline__ void field_encode(const NsrLevel *lds_lv, const TT *__restrict__ tables, float u0, float u1, float u2,
                                             bool live, int g, s8v &xd, s8v &xc, uint32_t fast_levels) {
    if constexpr (BATCH_GATHER && !SIGMA_ONLY && sizeof(TT) == 2) {
        uint2 v[4][8];
        float w[4][8];
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const NsrLevel lv = lds_lv[field_lane_level(g, i)];
                uint32_t rows[8];
                if (field_call_is_fast(fast_levels, i)) field_level_rows<true>(lv, u0, u1, u2, rows, w[i]);
                else field_level_rows<false>(lv, u0, u1, u2, rows, w[i]);
#pragma unroll
                for (int idx = 0; idx < 8; idx++) v[i][idx] = reinterpret_cast<const uint2 *>(tables)[rows[idx]];
            }
        }
        field_mix_rows<CD>(v, w, live, xd, xc);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const NsrLevel lv = lds_lv[field_lane_level(g, i)];
        const float4 a = field_call_is_fast(fast_levels, i)
                             ? field_encode_level<TT, SIGMA_ONLY, true>(lv, tables, u0, u1, u2, live)
                             : field_encode_level<TT, SIGMA_ONLY, false>(lv, tables, u0, u1, u2, live);
        xd[2 * i + 0] = MM<CD>::cvt(a.x);
        xd[2 * i + 1] = MM<CD>::cvt(a.y);
        xc[2 * i + 0] = MM<CD>::cvt(a.z);
        xc[2 * i + 1] = MM<CD>::cvt(a.w);
    }
}

__device__ __forceinline__ float field_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- the MLP chain of one 16-sample tile, in registers (k_field_fwd and k_render_infer run this one copy) -----------
// density net: 32 -> 64 -> 1.  Row 0 of the returned tile is the logit: element 0 on the g == 0 lanes.
template <int CD>
__device__ __forceinline__ f4v field_density_net(const short *wl, int lane, s8v xd) {
    f4v h[4];
    s8v hb[2];
    const s8v b1[1] = {xd};
    mm_layer32<CD, 4, 1>(wl + FW_D1, lane, b1, h);
    mm_pack64<CD, true, true>(h, hb);
    f4v o[1];
    mm_layer32<CD, 1, 2>(wl + FW_D2, lane, hb, o);
    return o[0];
}

// class, color1 and color2 nets on the colour features: rgb rows 0..2 (before the sigmoid), class rows 3..3+nc-1
// DIRS: color2's first layer is the K = 32 product over cat(color1 output, shb) -- the same four MFMAs on the wider instruction
template <int CD, bool DIRS = false>
__device__ __forceinline__ void field_colour_nets(const short *wl, int lane, s8v xc, f4v &rgb_out, f4v &cls_out, s4v shb = s4v{}) {
    f4v h[4];
    s8v hb[2];
    // ---- class net: 32 -> 64 -> nc (rows 3..) -----------------------------------------
    f4v cls[1];
    {
        const s8v b1[1] = {xc};
        mm_layer32<CD, 4, 1>(wl + FW_K1, lane, b1, h);
        mm_pack64<CD, true, true>(h, hb);
        mm_layer32<CD, 1, 2>(wl + FW_K2, lane, hb, cls);
    }
    // ---- color1 net: 32 -> 64 -> 16 ----------------------------------------------------
    f4v c1[1];
    {
        const s8v b1[1] = {xc};
        mm_layer32<CD, 4, 1>(wl + FW_C1A, lane, b1, h);
        mm_pack64<CD, true, true>(h, hb);
        mm_layer32<CD, 1, 2>(wl + FW_C1B, lane, hb, c1);
    }
    // ---- color2 net: 16 -> 64 -> 64 -> 3, sigmoid --------------------------------------
    f4v rgb[1];
    {
        const s4v c1b = mm_round4<CD, false>(c1[0]);
        if constexpr (DIRS) {
            const s8v b1[1] = {mm_cat(c1b, shb)};
            mm_layer32<CD, 4, 1>(wl + FW_R1, lane, b1, h);
        } else {
            mm_layer16<CD, 4>(wl + FW_R1, lane, c1b, h);
        }
        mm_pack64<CD, true, true>(h, hb);
        mm_layer32<CD, 4, 2>(wl + FW_R2, lane, hb, h);
        mm_pack64<CD, true, true>(h, hb);
        mm_layer32<CD, 1, 2>(wl + FW_R3, lane, hb, rgb);
    }
    rgb_out = rgb[0];
    cls_out = cls[0];
}

// cat(rgb, classes): this lane's channels ch = 4g + e (style_nerf.py:141)
__device__ __forceinline__ void field_cat(int g, f4v rgb, f4v cls, float (&v)[4]) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int ch = 4 * g + e;
        v[e] = ch < 3 ? field_sigmoid(rgb[e]) : cls[e];
    }
}

// XCD-aware logical block id: hardware deals blocks round-robin over the 8 XCDs, so blocks b and
// b+8 share an L2.  Give each XCD one contiguous eighth of the tiles (neighbouring tiles =
// neighbouring samples/rays = shared coarse-level table lines).  Bijective for any grid size.
__device__ __forceinline__ uint32_t field_logical_block() {
    const uint32_t nb = gridDim.x, b = blockIdx.x;
    const uint32_t q = nb / 8, r = nb % 8, xcd = b % 8, i = b / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
}

// The device-side sample count (M is only a capacity).  A macro: inlined from a function the clamp gets another scalar prologue
// and the kernel behind it another schedule; expanded in the kernel it compiles as it always has.
#define FIELD_COUNT(a) ((a).m_dev ? min((uint32_t)max((a).m_dev[0], 0), (a).M) : (a).M)

// host: everything of FieldArgs that the descriptor, the two parameter pointers and the sample count decide (the buffers are
// the caller's); `tables` must be 16-byte aligned for the gathers
static int field_fill_args(const nsr_field_desc *d, const void *tables, const float *mlp_params, FieldArgs &a, uint32_t M,
                           uint32_t &nblocks) {
    if (d->L != 16) return NSR_ERR_UNSUPPORTED;             // 32 features = two K=32 halves per encoder
    if (d->num_classes > 13) return NSR_ERR_UNSUPPORTED;    // class rows 3..15 of one 16-row tile
    if (d->offsets == nullptr) return NSR_ERR_INVALID_ARG;
    NsrLevels lv;
    nsr_fill_levels(&lv, d->offsets, 16, d->S, d->H, 0u);
    a.fast_levels = 0;
    for (int l = 0; l < 16; l++) {
        a.lv[l] = lv.lv[l];
        if (lv.lv[l].size == 0) return NSR_ERR_INVALID_ARG;
        if (lv.lv[l].use_hash && (lv.lv[l].size & (lv.lv[l].size - 1u)) == 0) a.fast_levels |= 1u << l;
    }
    for (int i = 0; i < 3; i++) { a.bmin[i] = d->bbox_min[i]; a.bsize[i] = d->bbox_size[i]; }
    a.density_scale = d->density_scale;
    a.C_ch = 3 + d->num_classes;
    a.M = M;
    const uint32_t ntiles = (M + 15) / 16;
    // >= 8 tiles per wave so the per-block weight-image build amortises; <= 8 blocks per CU
    uint32_t nb = (ntiles + 31) / 32;
    constexpr uint32_t max_blocks = 2048;
    if (nb > max_blocks) nb = max_blocks;
    if (nb == 0) nb = 1;
    nblocks = nb;
    a.tiles_per_block = (ntiles + nb - 1) / nb;
    a.tables = tables;
    a.params = mlp_params;
    return ((uintptr_t)tables & 15u) ? NSR_ERR_INVALID_ARG : NSR_OK;
}

// host: the (table type, compute type) instantiation of a field kernel.  `launch` is called with two tags: a value of the table
// type and the compute type as an integral constant.
template <typename F>
static int field_dispatch(int table_dtype, int compute_dtype, F &&launch) {
    using f16 = std::integral_constant<int, NSR_F16>;
    using bf16 = std::integral_constant<int, NSR_BF16>;
    if (table_dtype == NSR_F32 && compute_dtype == NSR_F16) return launch(float(), f16());
    if (table_dtype == NSR_F32 && compute_dtype == NSR_BF16) return launch(float(), bf16());
    if (table_dtype == NSR_F16 && compute_dtype == NSR_F16) return launch(_Float16(), f16());
    if (table_dtype == NSR_F16 && compute_dtype == NSR_BF16) return launch(_Float16(), bf16());
    return NSR_ERR_UNSUPPORTED;
}

