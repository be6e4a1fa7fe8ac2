// Gradients-out kernels of the fused field backward: the per-level encoder gradients of every sample are written to
// FieldBwdArgs::gout (256 B/sample) for the stand-alone, high-occupancy table scatter (table_scatter.hip) that walks the
// samples in nsr_sample_order's spatial order -- the scatter's dependent LDS / atomic chains are exactly what one wave per
// SIMD cannot hide.  k_field_bwd_gout is the full backward, k_field_bwd_color its colour-table-only form.  What they share
// with the fused tracker kernel (field_bwd.hip) is in field_bwd.h.
//
// This unit is compiled with -mllvm --amdgpu-mfma-vgpr-form (nerfstyle_amd/build.py): the 60 accumulator tiles are pinned to
// the ACCUMULATOR half of the register file by inline assembly ("+a"), and every other MFMA (forward recompute, dgrad, the
// identity transposes) then writes straight to VGPRs (1816 -> 1435 instructions per tile, 14.4 -> 13.5 ms).  Left to its
// heuristics the compiler gives ALL MFMAs of a kernel that needs AGPRs an AGPR destination and copies each transient result
// back (396 v_accvgpr_read per 16-sample tile, 22 % of the loop).
#include "field_bwd.h"

// The assembly is issued in hazard-complete blocks of four MFMAs on four DIFFERENT accumulators (field_wgrad_mfma4).  The
// compiler neither sees nor pads what is inside an asm statement, so each block carries what the gfx950 ISA asks of it:
//   head: a VALU write of a VGPR needs 2 wait states before an MFMA reads it as SrcA / SrcB (CDNA3 / CDNA4 ISA guide,
//         "Manually Inserted Wait States": VALU write VGPR -> v_mfma* read).  The operands come from the transposes'
//         packed conversions, which the compiler may place directly in front of the block: one `s_nop 1`, once per block,
//         whatever the distance (the previous form paid it in front of every MFMA);
//   body: MFMAs with different destinations and read-only A / B need no wait between them, and an accumulator's own chain
//         (the same instruction taking the previous result whole as SrcC, from the previous tile's block) is interlocked
//         by the hardware: 0 wait states;
//   tail: nothing but such a chain reads an accumulator inside the sample loop.  Their first other reader is the
//         reduction after the loop, which sits behind field_wgrad_settle.
// The statements are volatile: they stay in program order among themselves, so each accumulator sees its tiles in the
// order the samples are walked.
template <int CD>
__device__ __forceinline__ void field_wgrad_mfma4(f4v &c0, f4v &c1, f4v &c2, f4v &c3, s4v a0, s4v b0, s4v a1, s4v b1, s4v a2,
                                                  s4v b2, s4v a3, s4v b3) {
    if (CD == NSR_F16)
        asm volatile("s_nop 1\n\t"
                     "v_mfma_f32_16x16x16_f16 %0, %4, %5, %0\n\t"
                     "v_mfma_f32_16x16x16_f16 %1, %6, %7, %1\n\t"
                     "v_mfma_f32_16x16x16_f16 %2, %8, %9, %2\n\t"
                     "v_mfma_f32_16x16x16_f16 %3, %10, %11, %3"
                     : "+a"(c0), "+a"(c1), "+a"(c2), "+a"(c3)
                     : "v"(a0), "v"(b0), "v"(a1), "v"(b1), "v"(a2), "v"(b2), "v"(a3), "v"(b3));
    else
        asm volatile("s_nop 1\n\t"
                     "v_mfma_f32_16x16x16_bf16 %0, %4, %5, %0\n\t"
                     "v_mfma_f32_16x16x16_bf16 %1, %6, %7, %1\n\t"
                     "v_mfma_f32_16x16x16_bf16 %2, %8, %9, %2\n\t"
                     "v_mfma_f32_16x16x16_bf16 %3, %10, %11, %3"
                     : "+a"(c0), "+a"(c1), "+a"(c2), "+a"(c3)
                     : "v"(a0), "v"(b0), "v"(a1), "v"(b1), "v"(a2), "v"(b2), "v"(a3), "v"(b3));
}
// Behind the last block of the launch: an MFMA's result needs up to 18 wait states (the longest, 16-pass, form) before
// anything but its own accumulate chain may read it; the compiler, which does not know that the blocks hold MFMAs, pads
// nothing in front of the reduction's v_accvgpr_read.
template <int NT>
__device__ __forceinline__ void field_wgrad_settle(f4v (&acc)[NT]) {
    static_assert(NT % 4 == 0, "accumulators come in blocks of four");
#pragma unroll
    for (int k = 0; k < NT; k += 4)
        asm volatile("s_nop 15\n\ts_nop 3" : "+a"(acc[k]), "+a"(acc[k + 1]), "+a"(acc[k + 2]), "+a"(acc[k + 3]));
}
// wgrad of one layer (field_bwd.h): tile j = ot * NA + it; four consecutive tiles per block
template <int CD, int NG, int NA>
__device__ __forceinline__ void field_wgrad(f4v (&acc)[NG * NA], const s4v (&Gt)[NG], const s4v (&At)[NA]) {
    static_assert((NG * NA) % 4 == 0, "accumulators come in blocks of four");
#pragma unroll
    for (int j = 0; j < NG * NA; j += 4)
        field_wgrad_mfma4<CD>(acc[j], acc[j + 1], acc[j + 2], acc[j + 3], Gt[j / NA], At[j % NA], Gt[(j + 1) / NA],
                              At[(j + 1) % NA], Gt[(j + 2) / NA], At[(j + 2) % NA], Gt[(j + 3) / NA], At[(j + 3) % NA]);
}

// the four 16x16 blocks of a 64-row activation / gradient pair (+ one extra K = 16 block) as ONE transpose pipeline
constexpr int TR_DEPTH = 4;      // identity MFMAs in flight (mm_transpose16_n); every step more costs the kernel a register quad
template <int CD>
__device__ __forceinline__ void field_tr4p(const s8v (&x)[2], s4v ident, s4v (&out)[4]) {
    const s4v in[4] = {mm_lo(x[0]), mm_hi(x[0]), mm_lo(x[1]), mm_hi(x[1])};
    mm_transpose16_n<CD, 4, TR_DEPTH>(in, ident, out);
}
template <int CD>
__device__ __forceinline__ void field_tr5p(const s8v (&x)[2], s4v y, s4v ident, s4v (&out)[4], s4v (&yt)[1]) {
    const s4v in[5] = {mm_lo(x[0]), mm_hi(x[0]), mm_lo(x[1]), mm_hi(x[1]), y};
    s4v o[5];
    mm_transpose16_n<CD, 5, TR_DEPTH>(in, ident, o);
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = o[3]; yt[0] = o[4];
}
template <int CD>
__device__ __forceinline__ void field_tr6p(const s8v (&x)[2], s4v y, s4v z, s4v ident, s4v (&out)[4], s4v (&yt)[1], s4v (&zt)[1]) {
    const s4v in[6] = {mm_lo(x[0]), mm_hi(x[0]), mm_lo(x[1]), mm_hi(x[1]), y, z};
    s4v o[6];
    mm_transpose16_n<CD, 6, TR_DEPTH>(in, ident, o);
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = o[3]; yt[0] = o[4]; zt[0] = o[5];
}

// One wave per SIMD (its 240 weight-gradient accumulators).  The schedule of the MLP section is the one measured fastest
// for this kernel on the bench frame (48.6 M samples): straight order (one net at a time: 13.45 against 13.0 ms once the
// ReLUs are packed); ReLU on packed halves (13.5 -> 13.0 ms); the next tile's inputs requested right after this tile's
// first layer, with `cur` waited for at the loop top (13.2 -> 11.7 ms); weight-fragment reads queued ahead of the MFMA
// stream (11.7 -> 10.7 ms); the backward's ReLU masks on packed 16-bit pairs (1412 -> 1304 instructions per tile, 10.6 ->
// 10.0 ms); the wgrad operand transposes as pipelines of four identity MFMAs in flight, the wgrad MFMAs in blocks of four
// with one wait-state pad, the mask chain one instruction shorter (1254 -> 1114 instructions, 158 -> 59 no-ops per tile,
// 10.43 -> 9.56 ms; DESIGN.md "(r5)"); the wave index, and with it the tile counter and the prefetch conditions, in scalar
// registers, lanes past the count masked by selects instead of EXEC regions, the next tile requested unconditionally (1095 ->
// 996 instructions, 23 -> 5 EXEC regions, 9.59 -> 9.29 ms; DESIGN.md "(r9)").  An 8-deep queue for the two 8-fragment layers: no change.  The wgrad operand
// transposes through LDS (ds_write_b64 + ds_read_b64_tr_b16, 49 per tile) instead of an MFMA with the identity +
// re-rounding: 1304 -> 1240 instructions per tile and the same time (21.4 vs 21.5 ms for the pair) -- the LDS round trips
// cost what the MFMAs did.
// DIRS: 64 accumulator tiles -- all 256 registers of the accumulator half.
template <typename TT, int CD, bool FEATS, bool DIRS = false>
__global__ void __launch_bounds__(BWD_THREADS)
k_field_bwd_gout(FieldBwdArgsOf<DIRS> b) {
    constexpr int FWT = FW_IMAGE<DIRS>;
    const float *const dirs = field_dirs_of(b);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    short *wl = reinterpret_cast<short *>(smem);
    short *wt = wl + FWT;
    NsrLevel *lds_lv = reinterpret_cast<NsrLevel *>(smem + (size_t)(FWT + BW_TOTAL) * 2);
    const FieldArgs &a = b.f;
    field_build_fw<CD, false, DIRS>(wl, a.params);
    field_build_bw<CD>(wt, a.params);
    if (threadIdx.x < 16) lds_lv[threadIdx.x] = a.lv[threadIdx.x];
    __syncthreads();

    const uint32_t Mc = FIELD_COUNT(a);
    const uint32_t ntiles = (Mc + 15) / 16;
    // The wave index is read through one lane: the compiler cannot tell that threadIdx.x >> 6 is the same for a wave's 64
    // lanes, and with it per-lane the tile counter, the loop's back edge and the `is there a next tile` test all ran as
    // EXEC-masked regions on vector registers (DESIGN.md "(r9)").
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = lane & 15, g = lane >> 4;
    const TT *tables = reinterpret_cast<const TT *>(a.tables);
    const uint32_t lb = field_logical_block();
    // split by the DEVICE-side sample count (M is only a capacity): every block gets work
    const uint32_t tpb = (ntiles + gridDim.x - 1) / gridDim.x;
    const uint32_t t_begin = lb * tpb;
    const uint32_t t_end = min(t_begin + tpb, ntiles);
    const s4v ident = mm_identity_frag<CD>(lane);
    const int nc = (int)b.nc;
    const bool td = b.train_density != 0, tc = b.train_color != 0;
    // weight-gradient accumulators (60 tiles x 4 regs), resident for the whole launch
    f4v w_r3[4], w_r2[16], w_r1[4], w_c1b[4], w_c1a[8], w_k2[4], w_k1[8], w_d2[4], w_d1[8];
    f4v w_sh[4];             // DIRS: color2's SH columns (P_SH), tiles 60..63
    {
        const f4v z = {0.f, 0.f, 0.f, 0.f};
        if constexpr (DIRS) { w_sh[0] = z; w_sh[1] = z; w_sh[2] = z; w_sh[3] = z; }
#pragma unroll
        for (int q4 = 0; q4 < 4; q4++) { w_r3[q4] = z; w_r1[q4] = z; w_c1b[q4] = z; w_k2[q4] = z; w_d2[q4] = z; }
#pragma unroll
        for (int q8 = 0; q8 < 8; q8++) { w_c1a[q8] = z; w_k1[q8] = z; w_d1[q8] = z; }
#pragma unroll
        for (int q16 = 0; q16 < 16; q16++) w_r2[q16] = z;
    }

    // A tile's raw inputs: loads only, nothing here consumes a loaded value (a use would make the
    // compiler wait for the whole memory round trip inside the prefetch).  Lanes past the sample count
    // read sample 0 (always in bounds) and are masked where the values are used.
    struct TileIn {
        float x0, x1, x2;
        s8v xd, xc;
        float gsig;        // grad_sigmas[m] (used by the g == 0 lanes)
        float grgb[4];     // grad_rgbs[m, 4g .. 4g+3]
    };
    // position `16 * tile + s` of the walk -> index into the sample buffers (a valid one for lanes past the count).  With a
    // permutation (the forward walked the same order, its saved features are tile-major in it) this is a LOAD:
    // the entry of tile t + 2 is requested while tile t runs, so that tile t + 1's loads never wait for their index.
    auto fetch_idx = [&](uint32_t tile) -> uint32_t {
        const uint32_t m = tile * 16 + s;
        if (a.perm) return a.perm[min(m, Mc - 1u)];
        return m < Mc ? m : 0u;
    };
    auto load_tile = [&](uint32_t tile, uint32_t buf_idx) {
        TileIn r;
        const size_t mc = buf_idx;
        r.x0 = a.xyzs[mc * 3 + 0];
        r.x1 = a.xyzs[mc * 3 + 1];
        r.x2 = a.xyzs[mc * 3 + 2];
        r.gsig = b.grad_sigmas[mc];
        const float *gp = b.grad_rgbs + mc * a.C_ch;
        if (a.C_ch == 8) {
            const float4 t4 = reinterpret_cast<const float4 *>(gp)[g & 1];
            r.grgb[0] = t4.x; r.grgb[1] = t4.y; r.grgb[2] = t4.z; r.grgb[3] = t4.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) r.grgb[e] = gp[(uint32_t)(4 * g + e) < a.C_ch ? 4 * g + e : 0];
        }
        if (FEATS) {
            // the forward saved this lane's two B fragments: two 16-byte loads instead of 32 gathers
            const s8v *fi = reinterpret_cast<const s8v *>(a.feats) + ((size_t)tile * 64 + lane) * 2;
            r.xd = fi[0];
            r.xc = fi[1];
        }
        return r;
    };
    // Each wave walks a CONTIGUOUS quarter of the block's tiles: consecutive tiles continue the same ray,
    // so the rows of its coarse and middle levels recur and merge with records still held in the ring.
    const uint32_t wchunk = (t_end > t_begin ? (t_end - t_begin + BWD_THREADS / 64 - 1) / (BWD_THREADS / 64) : 0u);
    const uint32_t w_begin = min(t_begin + wave * wchunk, t_end), w_end = min(w_begin + wchunk, t_end);
    TileIn cur;
    uint32_t idx_cur = 0, idx_next = 0;          // buffer index of this lane's sample in the current / next tile
    if (w_begin < w_end) {
        idx_cur = fetch_idx(w_begin);
        cur = load_tile(w_begin, idx_cur);
        idx_next = w_begin + 1 < w_end ? fetch_idx(w_begin + 1) : idx_cur;
    }
    // one tile's per-level encoder gradients, 4 x 16 bytes per lane = 256 contiguous bytes per sample ([16][4] floats)
    float4 gout_v[4];
    uint32_t gout_m = 0;
    bool gout_valid = false;
    auto gout_store = [&]() {
        if (gout_valid) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int lv_i = (i < 2 ? 2 * g : 8 + 2 * g) + (i & 1);
                b.gout[(size_t)gout_m * 16 + lv_i] = gout_v[i];
            }
        }
        gout_valid = false;
    };
    // Which of this lane's four output channels (4g + e) exist, and which of them are colours (sigmoid) or class logits:
    // per-launch constants.  The loop selects with them and runs no EXEC-masked region for a sample past the count: such a
    // lane computes on the (valid) sample its clamped index names and every value it could contribute is selected to zero.
    bool ch_on[4], ch_rgb[4], ch_cls[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int ch = 4 * g + e;
        ch_on[e] = a.C_ch == 8 ? g < 2 : (uint32_t)ch < a.C_ch;
        ch_rgb[e] = (uint32_t)ch < a.C_ch && ch < 3;
        ch_cls[e] = (uint32_t)ch < a.C_ch && ch >= 3;
    }
    // weight-fragment queue of the MLP section (mfma_tiles.h, mm_queue32): holds the next layer's first four fragments
    s8v wq[4];
    s4v wq16[4];
    mm_queue32<4>(wq, wl + FW_D1, lane);
    for (uint32_t tile = w_begin; tile < w_end; tile++) {
        const uint32_t m = tile * 16 + s;
        const bool valid = m < Mc;
        // Nothing writes LDS inside this loop, so the compiler would hoist the (loop-invariant) weight-fragment LDS reads
        // out of it and spill them all -- 220 VGPRs to scratch, reloaded every tile.  The barrier keeps them where they are.
        asm volatile("" ::: "memory");
        // Every member of `cur` is made resident HERE, before this tile issues its own stores and loads: left to its
        // first use, a member's wait comes after them and -- one in-order vmcnt, loop-carried -- is emitted as vmcnt(0): the
        // wave then sits out the round trip of the loads it issued a moment ago (seen in the ISA: vmcnt(0) in front of the
        // first MFMA that reads cur.xc).  The loads of `cur` are a whole tile old at this point.
        asm volatile("" :: "v"(cur.x0), "v"(cur.x1), "v"(cur.x2), "v"(cur.gsig), "v"(cur.grgb[0]), "v"(cur.grgb[1]),
                     "v"(cur.grgb[2]), "v"(cur.grgb[3]), "v"(cur.xd), "v"(cur.xc), "v"(idx_next));
        // DIRS: this tile's direction is requested here, not a tile ahead with the other inputs (three registers the 64
        // accumulator tiles do not leave): its first use, color2's first layer, is four layers away
        float dv[3] = {0.f, 0.f, 0.f};
        // (idx_cur is a valid index on every lane: a lane past the count reads a direction it does not use)
        if constexpr (DIRS) { dv[0] = dirs[(size_t)idx_cur * 3 + 0]; dv[1] = dirs[(size_t)idx_cur * 3 + 1]; dv[2] = dirs[(size_t)idx_cur * 3 + 2]; }
        // the u of a lane past the count are those of the sample it read instead; `live` alone says whether they are used
        const float u0 = field_unit(cur.x0, a.bmin[0], a.bsize[0]);
        const float u1 = field_unit(cur.x1, a.bmin[1], a.bsize[1]);
        const float u2 = field_unit(cur.x2, a.bmin[2], a.bsize[2]);
        const bool live = valid && (u0 >= 0 && u0 <= 1 && u1 >= 0 && u1 <= 1 && u2 >= 0 && u2 <= 1);   // field_in_unit_cube, spelled out: through the call one s_and_b64 here takes its operands in the other order
        const float cur_gsig = valid ? cur.gsig : 0.f;
        float cur_grgb[4];
#pragma unroll
        for (int e = 0; e < 4; e++) cur_grgb[e] = (valid && ch_on[e]) ? cur.grgb[e] : 0.f;
        // no saved features: gather them now (dependent loads, the slow path)
        if (!FEATS) field_encode<TT, CD, false>(lds_lv, tables, u0, u1, u2, live, g, cur.xd, cur.xc, a.fast_levels);

        f4v gxd[2], gxc[2];        // d L / d (density, colour) features of this lane's levels
        // ================= recompute forward, keeping rounded activations ====================
        s8v xd[1] = {cur.xd}, xc[1] = {cur.xc};
        f4v h[4];
        s8v hd[2], hk[2], hc[2], hr1[2], hr2[2];
        f4v logit[1], c1[1], rgb[1];
        mm_layer32_q<CD, 4, 1>(wq, wl + FW_D1, lane, xd, h);          // queued at the end of the previous tile
        mm_queue32<2>(wq, wl + FW_D2, lane);
        gout_store();            // the previous tile's encoder gradients: after this tile's inputs have been waited for
        // There is no scatter between the end of the MLP section and the loop edge: loads issued there are waited for at
        // once (SQ_WAIT_ANY = 51 % of the wave's cycles, profiles/).  The next tile's inputs are requested HERE instead, a
        // whole MLP section ahead, at the price of 16 registers held through it.
        // The wave's last tile requests itself again (idx_next is then idx_cur, the index two ahead any clamped one): a few
        // loads nobody uses, once per wave, instead of a branch and sixteen zeroed registers in every tile.
        const TileIn nxt = load_tile(min(tile + 1, w_end - 1), idx_next);
        const uint32_t idx_nn = fetch_idx(min(tile + 2, w_end - 1));
        mm_pack64<CD, true, true>(h, hd);
        mm_layer32_q<CD, 1, 2>(wq, wl + FW_D2, lane, hd, logit);
        mm_queue32<4>(wq, wl + FW_K1, lane);
        mm_layer32_q<CD, 4, 1>(wq, wl + FW_K1, lane, xc, h);
        mm_queue32<4>(wq, wl + FW_C1A, lane);
        mm_pack64<CD, true, true>(h, hk);
        mm_layer32_q<CD, 4, 1>(wq, wl + FW_C1A, lane, xc, h);
        mm_queue32<2>(wq, wl + FW_C1B, lane);
        mm_pack64<CD, true, true>(h, hc);
        mm_layer32_q<CD, 1, 2>(wq, wl + FW_C1B, lane, hc, c1);
        s4v shb = {};
        if constexpr (DIRS) mm_queue32<4>(wq, wl + FW_R1, lane);
        else mm_queue16<4>(wq16, wl + FW_R1, lane);
        const s4v c1b = mm_round4<CD, false>(c1[0]);
        if constexpr (DIRS) {
            shb = mm_round4<CD, false>(field_sh4(g, dv[0], dv[1], dv[2]));
            const s8v b1[1] = {mm_cat(c1b, shb)};
            mm_layer32_q<CD, 4, 1>(wq, wl + FW_R1, lane, b1, h);
        } else {
            mm_layer16_q<CD, 4>(wq16, c1b, h);
        }
        mm_queue32<8>(wq, wl + FW_R2, lane);
        mm_pack64<CD, true, true>(h, hr1);
        mm_layer32_q<CD, 4, 2>(wq, wl + FW_R2, lane, hr1, h);
        mm_queue32<2>(wq, wl + FW_R3, lane);
        mm_pack64<CD, true, true>(h, hr2);
        mm_layer32_q<CD, 1, 2>(wq, wl + FW_R3, lane, hr2, rgb);
        mm_queue16<4>(wq16, wt + BW_R3T, lane);

        // ================= upstream gradients in B-fragment form (row = 4g + e) ===============
        s4v dyd, dyr, dyk;
        {
            // Every lane evaluates the derivatives of its row and SELECTS: the same expressions on the lanes that keep them,
            // zero on the others (rows that are no colour, lanes past the count), and no EXEC-masked region.  Only rows
            // 0..2 can be colours, so element 3 has no sigmoid.
            float gd[4] = {0.f, 0.f, 0.f, 0.f}, gr[4] = {0.f, 0.f, 0.f, 0.f}, gk[4] = {0.f, 0.f, 0.f, 0.f};
            {
                // sigma = exp(logit) * density_scale; trunc_exp backward clamps (tcnn_nerf.py:62-66)
                const float x = logit[0][0];
                const float d = cur_gsig * a.density_scale * expf(fminf(fmaxf(x, -15.0f), 15.0f));
                gd[0] = (valid && g == 0) ? d : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float gv = cur_grgb[e];
                if (e < 3) {
                    const float sg = field_sigmoid(rgb[0][e]);
                    const float d = gv * sg * (1.0f - sg);
                    gr[e] = (valid && ch_rgb[e]) ? d : 0.f;
                }
                gk[e] = (valid && ch_cls[e]) ? gv : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; e++) { dyd[e] = MM<CD>::cvt(gd[e]); dyr[e] = MM<CD>::cvt(gr[e]); dyk[e] = MM<CD>::cvt(gk[e]); }
        }

        // ================= color2: 16 -> 64 -> 64 -> 3 =======================================
        s8v g2[2], g1[2];
        s4v gc1;
        {
            mm_layer16_q<CD, 4>(wq16, dyr, h);
            mm_queue32<8>(wq, wt + BW_R2T, lane);
            field_mask_pack<CD, true>(h, hr2, g2);
            mm_layer32_q<CD, 4, 2>(wq, wt + BW_R2T, lane, g2, h);
            mm_queue32<2>(wq, wt + BW_R1T, lane);
            field_mask_pack<CD, true>(h, hr1, g1);
            f4v t1[1];
            mm_layer32_q<CD, 1, 2>(wq, wt + BW_R1T, lane, g1, t1);
            mm_queue16<4>(wq16, wt + BW_C1BT, lane);
            gc1 = mm_round4<CD, false>(t1[0]);
            // wgrads of r3, r2, r1
            // (every block is transposed right in front of the wgrad that consumes it: the transposed copies are then
            // live for one layer only, which is where the pipeline's extra register quads come from)
            s4v hr2t[4], hr1t[4], g2t[4], g1t[4], dyrt[1], c1t[1];
            field_tr5p<CD>(hr2, dyr, ident, hr2t, dyrt);
            field_wgrad<CD>(w_r3, dyrt, hr2t);
            field_tr4p<CD>(g2, ident, g2t);
            field_tr4p<CD>(hr1, ident, hr1t);
            field_wgrad<CD>(w_r2, g2t, hr1t);
            if constexpr (DIRS) {
                // the SH values sit in the lane layout of the color1 output tile: the same transpose, one more in the pipeline
                s4v sht[1];
                field_tr6p<CD>(g1, c1b, shb, ident, g1t, c1t, sht);
                field_wgrad<CD>(w_r1, g1t, c1t);
                field_wgrad<CD>(w_sh, g1t, sht);
            } else {
                field_tr5p<CD>(g1, c1b, ident, g1t, c1t);
                field_wgrad<CD>(w_r1, g1t, c1t);
            }
        }
        // transposed encoder features (shared by the color1 / class / density wgrads)
        s4v xct[2], xdt[2];
        {
            const s8v xcd[2] = {xc[0], xd[0]};
            s4v xt[4];
            field_tr4p<CD>(xcd, ident, xt);
            xct[0] = xt[0]; xct[1] = xt[1]; xdt[0] = xt[2]; xdt[1] = xt[3];
        }

        // ================= color1: 32 -> 64 -> 16, and class: 32 -> 64 -> nc ==================
        {
            s8v gh[2];
            s4v ght[4], hct[4], gc1t[1];
            mm_layer16_q<CD, 4>(wq16, gc1, h);
            mm_queue32<4>(wq, wt + BW_C1AT, lane);
            field_mask_pack<CD, true>(h, hc, gh);
            mm_layer32_q<CD, 2, 2>(wq, wt + BW_C1AT, lane, gh, gxc);
            mm_queue16<4>(wq16, wt + BW_K2T, lane);
            field_tr5p<CD>(hc, gc1, ident, hct, gc1t);
            field_wgrad<CD>(w_c1b, gc1t, hct);
            field_tr4p<CD>(gh, ident, ght);
            field_wgrad<CD>(w_c1a, ght, xct);
        }
        {
            s8v gh[2];
            s4v ght[4], hkt[4], dykt[1];
            mm_layer16_q<CD, 4>(wq16, dyk, h);
            mm_queue32<4>(wq, wt + BW_K1T, lane);
            field_mask_pack<CD, true>(h, hk, gh);
            mm_layer32_q<CD, 2, 2, true>(wq, wt + BW_K1T, lane, gh, gxc);
            mm_queue16<4>(wq16, wt + BW_D2T, lane);
            field_tr5p<CD>(hk, dyk, ident, hkt, dykt);
            field_wgrad<CD>(w_k2, dykt, hkt);
            field_tr4p<CD>(gh, ident, ght);
            field_wgrad<CD>(w_k1, ght, xct);
        }
        // ================= density: 32 -> 64 -> 1 =============================================
        {
            s8v gh[2];
            s4v ght[4], hdt[4], dydt[1];
            mm_layer16_q<CD, 4>(wq16, dyd, h);
            mm_queue32<4>(wq, wt + BW_D1T, lane);
            field_mask_pack<CD, true>(h, hd, gh);
            mm_layer32_q<CD, 2, 2>(wq, wt + BW_D1T, lane, gh, gxd);
            mm_queue32<4>(wq, wl + FW_D1, lane);          // the next tile's first layer
            field_tr5p<CD>(hd, dyd, ident, hdt, dydt);
            field_wgrad<CD>(w_d2, dydt, hdt);
            field_tr4p<CD>(gh, ident, ght);
            field_wgrad<CD>(w_d1, ght, xdt);
        }

        // ================= encoder gradients out ===============================================
        // gxd[t][2*(i&1)+f] is d L / d feature f of level lvl[i] (t = i >> 1): same lane<->level map as the forward encode.
        if (td || tc) {
            // kept in registers over the loop edge and stored early in the NEXT tile (gout_store): a store issued here
            // would be waited for -- one in-order vmcnt -- together with the next tile's loads at the loop top
            float4 sg[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int t = i >> 1, e0 = 2 * (i & 1);
                sg[i] = live ? make_float4(gxd[t][e0], gxd[t][e0 + 1], gxc[t][e0], gxc[t][e0 + 1]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) gout_v[i] = sg[i];
            gout_m = idx_cur;
            gout_valid = valid;
        }
        cur = nxt;
        idx_cur = idx_next; idx_next = idx_nn;
    }
    gout_store();
        field_wgrad_settle(w_r3); field_wgrad_settle(w_r2); field_wgrad_settle(w_r1); field_wgrad_settle(w_c1b);
        field_wgrad_settle(w_c1a); field_wgrad_settle(w_k2); field_wgrad_settle(w_k1); field_wgrad_settle(w_d2);
        field_wgrad_settle(w_d1);
        if constexpr (DIRS) field_wgrad_settle(w_sh);

    // ---- weight gradients: summed over the workgroup's waves in LDS, then ONE wave adds them to grad_mlp ----------------
    // Every wave holds 60 tiles = 15 360 partial sums.  Flushed wave by wave (rounds 1-2) that is 240 atomic wave-instructions
    // x 4 64-byte requests from each of 1 024 waves onto the same 960 lines -- ~1 M requests at the hot-line rate of the
    // memory-side atomic unit (5.5 G/s, tools/atomic_footprint_bench.hip): 0.18 ms per launch whatever the batch, half of a
    // 4 096-ray step's backward.  The weight-fragment image (61 440 B = exactly 60 tiles x 64 lanes x 16 B) is dead by now and
    // serves as the reduction buffer: four passes of read-add-write, then wave 0 reloads the totals and flushes them --
    // a quarter of the requests, and fp32 sums of four partials instead of four atomics (same value up to rounding order).
    if (b.grad_mlp) {
        f4v *const red = reinterpret_cast<f4v *>(smem);
#define NSR_RED_ALL(OP)                                                                                              \
        OP(w_r3, 0, 4) OP(w_r2, 4, 16) OP(w_r1, 20, 4) OP(w_c1b, 24, 4) OP(w_c1a, 28, 8) OP(w_k2, 36, 4) OP(w_k1, 40, 8)     \
        OP(w_d2, 48, 4) OP(w_d1, 52, 8)
        __syncthreads();                                   // every wave is done with the weight fragments
        for (int w = 0; w < BWD_THREADS / 64; w++) {
            if (wave == w) {
                // (DIRS: tiles 60..63 lie past the two weight images, over the level table and LDS this kernel does not use)
                if (w == 0) {
#define NSR_RED_ST(arr, base, n) _Pragma("unroll") for (int i = 0; i < n; i++) red[((base) + i) * 64 + lane] = arr[i];
                    NSR_RED_ALL(NSR_RED_ST)
                    if constexpr (DIRS) { NSR_RED_ST(w_sh, 60, 4) }
#undef NSR_RED_ST
                } else {
#define NSR_RED_ADD(arr, base, n) _Pragma("unroll") for (int i = 0; i < n; i++) red[((base) + i) * 64 + lane] += arr[i];
                    NSR_RED_ALL(NSR_RED_ADD)
                    if constexpr (DIRS) { NSR_RED_ADD(w_sh, 60, 4) }
#undef NSR_RED_ADD
                }
            }
            __syncthreads();
        }
        if (wave == 0) {
#define NSR_RED_LD(arr, base, n) _Pragma("unroll") for (int i = 0; i < n; i++) arr[i] = red[((base) + i) * 64 + lane];
            NSR_RED_ALL(NSR_RED_LD)
            if constexpr (DIRS) { NSR_RED_LD(w_sh, 60, 4) }
#undef NSR_RED_LD
            float *gm = b.grad_mlp;
            if constexpr (DIRS) field_wgrad_flush<4, 1>(gm + P_SH, 16, 0, 64, w_sh, lane);
            field_wgrad_flush<1, 4>(gm + P_R3, 64, 0, 3, w_r3, lane);
            field_wgrad_flush<4, 4>(gm + P_R2, 64, 0, 64, w_r2, lane);
            field_wgrad_flush<4, 1>(gm + P_R1, 16, 0, 64, w_r1, lane);
            field_wgrad_flush<1, 4>(gm + P_C1B, 64, 0, 16, w_c1b, lane);
            field_wgrad_flush<4, 2>(gm + P_C1A, 32, 0, 64, w_c1a, lane);
            field_wgrad_flush<1, 4>(gm + P_K2, 64, CLASS_ROW_SHIFT, nc, w_k2, lane);
            field_wgrad_flush<4, 2>(gm + P_K1, 32, 0, 64, w_k1, lane);
            field_wgrad_flush<1, 4>(gm + P_D2, 64, 0, 1, w_d2, lane);
            field_wgrad_flush<4, 2>(gm + P_D1, 32, 0, 64, w_d1, lane);
        }
#undef NSR_RED_ALL
    }
}

// Colour-table-only form of the gradients-out backward: the stylisation stage trains `x_color_embedder` alone (trainers/style.py:25),
// so no weight gradient is wanted (grad_mlp == NULL) and nothing behind the density output either.  What is left of the chain is
// the forward recompute of the class and colour nets (for the ReLU masks) and their input gradients -- 60 of the full kernel's
// ~190 MFMAs, none of its 240 accumulators, so the kernel runs at four waves per SIMD (512-thread workgroups around one 60 KB weight image) instead of one
// (1008x756 stylisation iteration, 24 patches on four streams: 41.1 -> 39.4 ms).  Same helper calls in the same order as the full kernel: the
// colour gradients are bit-identical to its.  gout's density components are written as zeros (the scatter ignores them).
// Weight-fragment reads run four ahead of the MFMA stream (mfma_tiles.h), as everywhere in this unit.
constexpr int COLOR_THREADS = 512;       // 8 waves share one 60 KB weight image: two workgroups per CU = four waves per SIMD (90 registers)
template <int CD, bool DIRS = false>
__global__ void __launch_bounds__(COLOR_THREADS)
k_field_bwd_color(FieldBwdArgsOf<DIRS> b) {
    constexpr int AHEAD = 4;
    const float *const dirs = field_dirs_of(b);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    short *wl = reinterpret_cast<short *>(smem);
    short *wt = wl + FW_IMAGE<DIRS>;
    const FieldArgs &a = b.f;
    field_build_fw<CD, false, DIRS>(wl, a.params);
    field_build_bw<CD>(wt, a.params);
    __syncthreads();
    const uint32_t Mc = FIELD_COUNT(a);
    const uint32_t ntiles = (Mc + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const uint32_t lb = field_logical_block();
    const uint32_t tpb = (ntiles + gridDim.x - 1) / gridDim.x;
    const uint32_t t_begin = lb * tpb;
    const uint32_t t_end = min(t_begin + tpb, ntiles);
    for (uint32_t tile = t_begin + wave; tile < t_end; tile += COLOR_THREADS / 64) {
        const uint32_t mpos = tile * 16 + s;
        const bool valid = mpos < Mc;
        const uint32_t m = a.perm[min(mpos, Mc - 1u)];
        const float u0 = field_unit(a.xyzs[(size_t)m * 3 + 0], a.bmin[0], a.bsize[0]);
        const float u1 = field_unit(a.xyzs[(size_t)m * 3 + 1], a.bmin[1], a.bsize[1]);
        const float u2 = field_unit(a.xyzs[(size_t)m * 3 + 2], a.bmin[2], a.bsize[2]);
        const bool live = valid && field_in_unit_cube(u0, u1, u2);
        float grgb[4];
        {
            const float *gp = b.grad_rgbs + (size_t)m * a.C_ch;
            if (a.C_ch == 8) {
                const float4 t4 = reinterpret_cast<const float4 *>(gp)[g & 1];
                grgb[0] = t4.x; grgb[1] = t4.y; grgb[2] = t4.z; grgb[3] = t4.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) grgb[e] = gp[(uint32_t)(4 * g + e) < a.C_ch ? 4 * g + e : 0];
            }
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (!(valid && (a.C_ch == 8 ? g < 2 : (uint32_t)(4 * g + e) < a.C_ch))) grgb[e] = 0.f;
        }
        const s8v xc[1] = {(reinterpret_cast<const s8v *>(a.feats) + ((size_t)tile * 64 + lane) * 2)[1]};
        // ---- forward recompute (rounded activations) ----
        f4v h[4];
        s8v hk[2], hc[2], hr1[2], hr2[2];
        f4v c1[1], rgb[1];
        mm_layer32<CD, 4, 1, AHEAD>(wl + FW_K1, lane, xc, h);
        mm_pack64<CD, true, true>(h, hk);
        mm_layer32<CD, 4, 1, AHEAD>(wl + FW_C1A, lane, xc, h);
        mm_pack64<CD, true, true>(h, hc);
        mm_layer32<CD, 1, 2, AHEAD>(wl + FW_C1B, lane, hc, c1);
        const s4v c1b = mm_round4<CD, false>(c1[0]);
        if constexpr (DIRS) {
            const s8v b1[1] = {mm_cat(c1b, field_sh_frag<CD>(dirs, m, valid, g))};
            mm_layer32<CD, 4, 1, AHEAD>(wl + FW_R1, lane, b1, h);
        } else {
            mm_layer16<CD, 4, AHEAD>(wl + FW_R1, lane, c1b, h);
        }
        mm_pack64<CD, true, true>(h, hr1);
        mm_layer32<CD, 4, 2, AHEAD>(wl + FW_R2, lane, hr1, h);
        mm_pack64<CD, true, true>(h, hr2);
        mm_layer32<CD, 1, 2, AHEAD>(wl + FW_R3, lane, hr2, rgb);
        // ---- upstream gradients in B-fragment form (row = 4g + e) ----
        s4v dyr, dyk;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int ch = 4 * g + e;
            float gr = 0.f, gk = 0.f;
            if (valid && (uint32_t)ch < a.C_ch) {
                if (ch < 3) {
                    const float sg = field_sigmoid(rgb[0][e]);
                    gr = grgb[e] * sg * (1.0f - sg);
                } else {
                    gk = grgb[e];
                }
            }
            dyr[e] = MM<CD>::cvt(gr);
            dyk[e] = MM<CD>::cvt(gk);
        }
        // ---- colour-2, colour-1, class: input gradients ----
        s8v g2[2], g1[2], gh[2];
        f4v t1[1], gxc[2];
        mm_layer16<CD, 4, AHEAD>(wt + BW_R3T, lane, dyr, h);
        field_mask_pack<CD, true>(h, hr2, g2);
        mm_layer32<CD, 4, 2, AHEAD>(wt + BW_R2T, lane, g2, h);
        field_mask_pack<CD, true>(h, hr1, g1);
        mm_layer32<CD, 1, 2, AHEAD>(wt + BW_R1T, lane, g1, t1);
        const s4v gc1 = mm_round4<CD, false>(t1[0]);
        mm_layer16<CD, 4, AHEAD>(wt + BW_C1BT, lane, gc1, h);
        field_mask_pack<CD, true>(h, hc, gh);
        mm_layer32<CD, 2, 2, AHEAD>(wt + BW_C1AT, lane, gh, gxc);
        mm_layer16<CD, 4, AHEAD>(wt + BW_K2T, lane, dyk, h);
        field_mask_pack<CD, true>(h, hk, gh);
        mm_layer32_acc<CD, 2, 2, AHEAD>(wt + BW_K1T, lane, gh, gxc);
        if (valid) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int t = i >> 1, e0 = 2 * (i & 1);
                const int lv_i = (i < 2 ? 2 * g : 8 + 2 * g) + (i & 1);
                b.gout[(size_t)m * 16 + lv_i] = live ? make_float4(0.f, 0.f, gxc[t][e0], gxc[t][e0 + 1]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
}
template <int CD>
static int field_bwd_launch_color(const FieldBwdArgs &b, hipStream_t s, const float *dirs) {
    const size_t lds = (size_t)(FW_IMAGE<false> + BW_TOTAL) * 2, lds_dirs = (size_t)(FW_IMAGE<true> + BW_TOTAL) * 2;
    // two resident workgroups per CU; >= 8 tiles per wave so that the weight-image build amortises
    const uint32_t ntiles = (b.f.M + 15) / 16;
    uint32_t nb = (ntiles + 63) / 64;
    if (nb > 512) nb = 512;
    if (nb == 0) nb = 1;
    if (dirs) {
        const FieldBwdDirsArgs bd = field_bwd_with_dirs(b, dirs);
        return nsr_launch_lds<k_field_bwd_color<CD, true>>(lds_dirs, dim3(nb), dim3(COLOR_THREADS), lds_dirs, s, bd);
    }
    return nsr_launch_lds<k_field_bwd_color<CD>>(lds, dim3(nb), dim3(COLOR_THREADS), lds, s, b);
}

int nsr_field_bwd_launch_gout(const FieldBwdArgs &b, int table_dtype, int compute_dtype, bool feats, dim3 grid, hipStream_t s,
                              const float *dirs) {
    if (b.grad_mlp == nullptr && !b.train_density && b.train_color && feats && b.f.perm != nullptr) {
        if (compute_dtype == NSR_F16) return field_bwd_launch_color<NSR_F16>(b, s, dirs);
        if (compute_dtype == NSR_BF16) return field_bwd_launch_color<NSR_BF16>(b, s, dirs);
    }
    return field_bwd_dispatch(table_dtype, compute_dtype, feats, [&](auto tt, auto cd, auto ft) {
        if (dirs) {
            const FieldBwdDirsArgs bd = field_bwd_with_dirs(b, dirs);
            return nsr_launch_lds<k_field_bwd_gout<decltype(tt), cd(), ft(), true>>(BWD_LDS_BYTES_DIRS, grid, dim3(BWD_THREADS),
                                                                                    BWD_LDS_BYTES_DIRS, s, bd);
        }
        return nsr_launch_lds<k_field_bwd_gout<decltype(tt), cd(), ft()>>(BWD_LDS_BYTES, grid, dim3(BWD_THREADS), BWD_LDS_BYTES, s, b);
    });
}
