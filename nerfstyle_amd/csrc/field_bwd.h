// Fused field backward for gfx950: what its three kernels share.  One launch does what the reference does with composite's
// saved tensors + 4 tcnn backward launches + 2 grid backward launches (+ two zeros_like fills):
//
//   recompute encode + forward chain (nothing was saved by the forward: no [M,.] activations in
//   HBM) -> trunc_exp' / sigmoid' / ReLU masks -> dgrad chain on MFMA (W^T as the A operand,
//   samples stay on lanes) -> wgrad on MFMA -> table scatter with fp32 atomics.
//
// wgrad needs the sample index on the MFMA k axis, i.e. every activation / gradient block
// transposed.  That is done in registers with one 16x16x16 MFMA against the identity per block
// (exact), not through LDS.  The 60 weight-gradient tiles (15360 fp32) live in the accumulator
// half of the register file for the whole launch: workgroups are 4 waves = one wave per SIMD, so a
// wave owns all 512 registers of its lane slice (240 of them these accumulators) and every wgrad
// MFMA accumulates in place; each wave adds its tiles to grad_mlp once, at the end.
// (A first version accumulated them in LDS with ds_add_f32: that alone cost 59 of 73 ms -- LDS
// float atomics retire at well under one lane per clock -- see profiles/ and DESIGN.md.)
//
// Lane (s = lane&15, g = lane>>4) owns levels {2g, 2g+1, 8+2g, 9+2g} of sample s in both
// directions, so dX arrives from the MFMA on the lane that scatters it.
//
// The kernels, one translation unit each, with the schedule measured fastest for each:
//   field_bwd.hip       k_field_bwd_tracker: scatters the table gradients itself (the fused run tracker);
//   field_bwd_gout.hip  k_field_bwd_gout: writes them out for the stand-alone table scatter (table_scatter.hip), and
//                       k_field_bwd_color, its colour-table-only form; compiled with -mllvm --amdgpu-mfma-vgpr-form.
#pragma once
#include <type_traits>

#include "field_common.h"
#include "table_scatter.h"

// ---- backward LDS image (units: shorts) ------------------------------------------------------
constexpr int BW_R3T = 0;        // r3^T  [64 x 16]  4 frag16
constexpr int BW_R2T = 1024;     // r2^T  [64 x 64]  8 frag32
constexpr int BW_R1T = 5120;     // r1^T  [16 x 64]  2 frag32
constexpr int BW_C1BT = 6144;    // c1b^T [64 x 16]  4 frag16
constexpr int BW_C1AT = 7168;    // c1a^T [32 x 64]  4 frag32
constexpr int BW_K2T = 9216;     // k2^T  [64 x 16]  4 frag16 (k index = class row + 3)
constexpr int BW_K1T = 10240;    // k1^T  [32 x 64]  4 frag32
constexpr int BW_D2T = 12288;    // d2^T  [64 x 16]  4 frag16
constexpr int BW_D1T = 13312;    // d1^T  [32 x 64]  4 frag32
constexpr int BW_TOTAL = 15360;

constexpr int BWD_THREADS = 256;
// per wave: the tracker's record ring (1024 x {float4 sums, row}) + its [16 levels][16 samples] float4 gradient staging buffer
constexpr size_t BWD_QUEUE_BYTES_PER_WAVE = 1024 * 16 + 1024 * 4 + 16 * 16 * 16;
constexpr size_t BWD_LDS_BYTES = (size_t)FW_TOTAL * 2 + (size_t)BW_TOTAL * 2 + 16 * sizeof(NsrLevel) +
                                 (BWD_THREADS / 64) * BWD_QUEUE_BYTES_PER_WAVE;
// the direction-taking instantiations: the forward image is 2 KB larger (field_common.h), everything behind it moves up
constexpr size_t BWD_LDS_BYTES_DIRS = BWD_LDS_BYTES + (size_t)(FW_TOTAL_DIRS - FW_TOTAL) * 2;
static_assert(BWD_LDS_BYTES_DIRS <= 160 * 1024, "one workgroup per CU owns all of its LDS, and no more");


struct FieldBwdArgs {
    FieldArgs f;
    const float *grad_sigmas;
    const float *grad_rgbs;
    float *grad_tables;
    float *grad_mlp;
    int train_density, train_color;
    uint32_t nc;
    float4 *gout;              // gradients-out kernels: [M][16 levels] float4 = d loss / d (density f0, f1, colour f0, f1) of every sample
};
// argument of the direction-taking kernels (nsr_field_backward_dirs): dirs [M,3], indexed like xyzs.  Their recomputed forward
// runs color2's K = 32 first layer; the dgrad through it is unchanged (only the color1 columns carry a gradient onwards, BW_R1T
// stays), and the SH columns' weight gradient dH1^T x SH is four more accumulator tiles (64 in all: 256 registers).
struct FieldBwdDirsArgs : FieldBwdArgs {
    const float *dirs;
};
template <bool DIRS> using FieldBwdArgsOf = std::conditional_t<DIRS, FieldBwdDirsArgs, FieldBwdArgs>;
__device__ __forceinline__ const float *field_dirs_of(const FieldBwdArgs &) { return nullptr; }
__device__ __forceinline__ const float *field_dirs_of(const FieldBwdDirsArgs &b) { return b.dirs; }
static inline FieldBwdDirsArgs field_bwd_with_dirs(const FieldBwdArgs &b, const float *dirs) {
    FieldBwdDirsArgs bd;
    static_cast<FieldBwdArgs &>(bd) = b;
    bd.dirs = dirs;
    return bd;
}

template <int CD>
__device__ __forceinline__ void field_build_bw(short *lds, const float *__restrict__ p) {
    mm_build_frags<CD>(lds + BW_R3T, p + P_R3, 16, 64, 4, 16, true, 0, false);
    mm_build_frags<CD>(lds + BW_R2T, p + P_R2, 64, 64, 4, 64, true, 0, true);
    mm_build_frags<CD>(lds + BW_R1T, p + P_R1, 64, 16, 1, 64, true, 0, true);
    mm_build_frags<CD>(lds + BW_C1BT, p + P_C1B, 16, 64, 4, 16, true, 0, false);
    mm_build_frags<CD>(lds + BW_C1AT, p + P_C1A, 64, 32, 2, 64, true, 0, true);
    mm_build_frags<CD>(lds + BW_K2T, p + P_K2, 16, 64, 4, 16, true, CLASS_ROW_SHIFT, false);
    mm_build_frags<CD>(lds + BW_K1T, p + P_K1, 64, 32, 2, 64, true, 0, true);
    mm_build_frags<CD>(lds + BW_D2T, p + P_D2, 16, 64, 4, 16, true, 0, false);
    mm_build_frags<CD>(lds + BW_D1T, p + P_D1, 64, 32, 2, 64, true, 0, true);
}

// 4 gradient tiles -> masked by the forward activation -> two K=32 B fragments
template <int CD, bool PKMASK>
__device__ __forceinline__ void field_mask_pack(const f4v (&gacc)[4], const s8v (&act)[2], s8v (&out)[2]) {
    if constexpr (PKMASK) {
        // Round first, mask afterwards on the packed 16-bit pairs: (act > 0 as a signed 16-bit pattern) -> all-ones / zero by
        // a saturating negate and an arithmetic shift -- two packed instructions per PAIR instead of a compare and a select
        // per element, and one packed conversion per pair.  Same bits: a masked element is +0 either way, the others are
        // rounded alike (round to nearest even).  (The saturation matters for 0x8000 alone, whose plain negate is itself;
        // until round 5 the chain was max(act, 0), negate, shift: the same mask for all 65 536 patterns, checked one by
        // one on the CPU, DESIGN.md "(r5)".)  The mask is inline asm: the compiler turns the same arithmetic back into
        // compares and selects.  One statement per fragment, negates first and shifts behind them: the compiler pads one
        // wait state between an asm statement and the first VALU instruction that reads its outputs, and with a
        // statement per pair that was one no-op per pair.
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const uint4 a4 = __builtin_bit_cast(uint4, act[t]);
            uint32_t gp[4], m[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {                       // pair p of this fragment: elements 2p, 2p + 1
                const f4v &g = gacc[2 * t + (p >> 1)];
                const int e = 2 * (p & 1);
                // (the conversion is left to the compiler: it reads MFMA results, and only the compiler knows how many wait
                // states that read needs -- an inline-asm conversion here returned stale accumulators in one instantiation)
                if (CD == NSR_F16) {
                    typedef _Float16 hh2 __attribute__((ext_vector_type(2)));
                    const hh2 hp = {(_Float16)g[e], (_Float16)g[e + 1]};
                    gp[p] = __builtin_bit_cast(uint32_t, hp);
                } else {
                    typedef __bf16 bb2 __attribute__((ext_vector_type(2)));
                    const bb2 bp = {(__bf16)g[e], (__bf16)g[e + 1]};
                    gp[p] = __builtin_bit_cast(uint32_t, bp);
                }
            }
            asm("v_pk_sub_i16 %0, 0, %4 clamp\n\t"
                "v_pk_sub_i16 %1, 0, %5 clamp\n\t"
                "v_pk_sub_i16 %2, 0, %6 clamp\n\t"
                "v_pk_sub_i16 %3, 0, %7 clamp\n\t"
                "v_pk_ashrrev_i16 %0, 15, %0 op_sel_hi:[0,1]\n\t"
                "v_pk_ashrrev_i16 %1, 15, %1 op_sel_hi:[0,1]\n\t"
                "v_pk_ashrrev_i16 %2, 15, %2 op_sel_hi:[0,1]\n\t"
                "v_pk_ashrrev_i16 %3, 15, %3 op_sel_hi:[0,1]"
                : "=&v"(m[0]), "=&v"(m[1]), "=&v"(m[2]), "=&v"(m[3])
                : "v"(a4.x), "v"(a4.y), "v"(a4.z), "v"(a4.w));
            out[t] = __builtin_bit_cast(s8v, make_uint4(gp[0] & m[0], gp[1] & m[1], gp[2] & m[2], gp[3] & m[3]));
        }
    } else {
        out[0] = mm_cat(mm_round4<CD, false>(mm_relu_mask(gacc[0], mm_lo(act[0]))),
                        mm_round4<CD, false>(mm_relu_mask(gacc[1], mm_hi(act[0]))));
        out[1] = mm_cat(mm_round4<CD, false>(mm_relu_mask(gacc[2], mm_lo(act[1]))),
                        mm_round4<CD, false>(mm_relu_mask(gacc[3], mm_hi(act[1]))));
    }
}

// ---- weight gradients ------------------------------------------------------------------------
// wgrad of one layer over a wave's 16 samples, accumulated in registers (field_wgrad of either unit):
//   dW[o][i] += sum_s G[o][s] * A[i][s]
// Gt / At are the transposed blocks (lane = feature, elements = samples 4g+e).  Tile (ot,it) of
// the result, at index ot * NA + it: lane (i = lane&15, g) element e = dW[16ot + 4g + e][16it + i].
// End of launch: one global atomic per weight per wave.  Rows are shifted by row_shift and clipped
// to [0, row_hi) (rows outside hold zeros by construction: padded outputs get no gradient).
template <int NG, int NA>
__device__ __forceinline__ void field_wgrad_flush(float *__restrict__ gw, int in_p, int row_shift, int row_hi,
                                                  const f4v (&acc)[NG * NA], int lane) {
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ot = 0; ot < NG; ot++) {
#pragma unroll
        for (int it = 0; it < NA; it++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int row = 16 * ot + 4 * g + e - row_shift;
                const float v = acc[ot * NA + it][e];
                if (row >= 0 && row < row_hi && v != 0.0f) atomicAdd(gw + row * in_p + 16 * it + i, v);
            }
        }
    }
}

// ---- host: the (table type, compute type, FEATS) instantiation of a one-wave-per-SIMD kernel ----------------------------
// `launch` is called with three tags: a value of the table type and two integral constants.
template <typename F>
static int field_bwd_dispatch(int table_dtype, int compute_dtype, bool feats, F &&launch) {
    using f16 = std::integral_constant<int, NSR_F16>;
    using bf16 = std::integral_constant<int, NSR_BF16>;
    if (feats) {                                 // no gather in the kernel: the table type does not matter
        if (compute_dtype == NSR_F16) return launch(float(), f16(), std::true_type());
        if (compute_dtype == NSR_BF16) return launch(float(), bf16(), std::true_type());
    } else {
        if (table_dtype == NSR_F32 && compute_dtype == NSR_F16) return launch(float(), f16(), std::false_type());
        if (table_dtype == NSR_F32 && compute_dtype == NSR_BF16) return launch(float(), bf16(), std::false_type());
        if (table_dtype == NSR_F16 && compute_dtype == NSR_F16) return launch(_Float16(), f16(), std::false_type());
        if (table_dtype == NSR_F16 && compute_dtype == NSR_BF16) return launch(_Float16(), bf16(), std::false_type());
    }
    return NSR_ERR_UNSUPPORTED;
}

// field_bwd_gout.hip: the gradients-out kernel, or its colour-table-only form where that is all the caller wants
// (dirs != NULL: the direction-taking instantiations)
int nsr_field_bwd_launch_gout(const FieldBwdArgs &b, int table_dtype, int compute_dtype, bool feats, dim3 grid, hipStream_t s,
                              const float *dirs);
