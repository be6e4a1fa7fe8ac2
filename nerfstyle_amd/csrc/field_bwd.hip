// Fused field backward: the C entry point, and the kernel that scatters the table gradients itself (the fused run tracker).
// What it shares with the gradients-out kernels (field_bwd_gout.hip) is in field_bwd.h.
#include "field_bwd.h"

// ---- table scatter ----------------------------------------------------------------------------
// Global float atomics are priced per 64-byte request at the memory side (21 G requests/s chip wide,
// tools/atomic_*_bench.hip), not per byte: 64 lanes adding one dword each to 64 different rows cost 64
// requests.  The naive scatter (4 dword atomics per corner per lane) is 512 requests per sample and ran the
// whole backward at 21 M samples/s.  What is done instead, exact up to fp32 summation order:
//   1. consecutive samples of a ray share table rows (same cell, or the face shared with the next cell) on
//      all but the finest levels: field_scatter_seq keeps every corner's open run in registers and emits one
//      record {row, d0, d1, c0, c1} per finished run (128 corner touches -> ~30 records per sample);
//   2. records go through a per-wave LDS ring and are drained 16 per wave-instruction with 4 lanes per
//      record: the four dwords of an interleaved row leave as ONE 16-byte request, and the two x corners
//      of a lane, adjacent in the ring, usually share a 64-byte line (one request);
//   3. the ring is drained in small paced bursts spread over the NEXT tile's dgrad / wgrad section
//      (SCQ_PACE): atomics are fire-and-forget, but a burst of ~45 back-to-back wave-instructions blocks
//      at issue once the memory side is saturated, and with one wave per SIMD a blocked wave is an idle
//      SIMD; and nothing may wait on vmcnt while fresh atomics are in flight (see the loop comment).
constexpr int SCQ_CAP = 1024;    // records per wave (power of two)
constexpr int SCQ_MASK = SCQ_CAP - 1;
struct ScatterQueue {
    uint32_t *rows;              // [SCQ_CAP]
    float4 *vals;                // [SCQ_CAP]
    int head, tail;              // wave-uniform, monotonically increasing record indices
};

// N full groups of 16 records: all LDS reads first, then the N atomic wave-instructions (4 lanes per
// record: the 4 dwords of an interleaved row leave as ONE 16-byte request).  With one wave per SIMD an
// LDS round trip per instruction would be fully exposed.  Ring rows are stored +1 (see the scatter):
// gt1 = grad_tables - 4 floats.
template <int N>
__device__ __forceinline__ void scq_drain(ScatterQueue &q, float *__restrict__ gt1, int t, int i, bool on) {
    uint32_t row[N];
    float v[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int slot = (q.head + 16 * k + t) & SCQ_MASK;
        row[k] = q.rows[slot];
        v[k] = reinterpret_cast<const float *>(q.vals)[slot * 4 + i];
    }
    if (on) {
#pragma unroll
        for (int k = 0; k < N; k++) atomicAdd(gt1 + (size_t)row[k] * 4 + i, v[k]);
    }
    q.head += 16 * N;
}

// Issues up to `max_instr` atomic wave-instructions of 16 records.  Only full groups unless `flush`.
__device__ __forceinline__ void scq_pace(ScatterQueue &q, float *__restrict__ gt1, int lane, bool td, bool tc, int max_instr,
                                         bool flush) {
    __builtin_amdgcn_wave_barrier();
    const int t = lane >> 2, i = lane & 3;
    const bool on = (i < 2) ? td : tc;
    int full = (q.tail - q.head) >> 4;
    if (full > max_instr) full = max_instr;
    for (; full >= 4; full -= 4) scq_drain<4>(q, gt1, t, i, on);
    if (full >= 2) { scq_drain<2>(q, gt1, t, i, on); full -= 2; }
    if (full >= 1) scq_drain<1>(q, gt1, t, i, on);
    if (flush) {
        const int n = q.tail - q.head;          // < 16 when max_instr did not bound the loop above
        if (t < n && on) {
            const int slot = (q.head + t) & SCQ_MASK;
            atomicAdd(gt1 + (size_t)q.rows[slot] * 4 + i, reinterpret_cast<const float *>(q.vals)[slot * 4 + i]);
        }
        q.head += n < 16 ? n : 16;
    }
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------------------------
// Sequential run tracker.  Lane = (level l = lane >> 2,
// y/z corner pair p = lane & 3) owns the two x corners of that pair as two STREAMS A (x0) and B (x0 + 1) and
// walks the tile's 16 samples in order, keeping for each stream the open run {row key, 4 gradient sums} in
// registers -- across tiles too, a wave's tiles being consecutive samples.  A sample that stays in the cell
// adds to both runs; one that moves exactly one cell along one axis hands the still-needed runs over in
// registers (x: between the lane's own two streams; y, z: from the quad neighbour lane p^1 / p^2 by DPP
// quad_perm) -- the decision is geometric (same grid corner => same row), identical in the four lanes of a
// level, so every finished run is emitted exactly once; anything else closes both runs.  Per sample step
// ~180 instructions for 128 corner touches (the first version of this kernel, a DPP segmented scan over the 16
// samples of a level with a hashed "row still in the ring" table, needed ~4000 per tile more).
constexpr int SEQ_K = 4;      // sample steps per ring push
struct SeqState {
    uint32_t c0, c1, c2;     // cell of the previous sample at this lane's level
    uint32_t kA, kB;         // row + 1 of the open runs (0: none)
    float4 aA, aB;           // their gradient sums {d0, d1, c0, c1}
};

__device__ __forceinline__ float4 seq_quad(const float4 &v, bool n1) {
    // value of quad neighbour p^1 (n1) or p^2
    float4 r;
    if (n1) {
        r.x = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v.x), 0xB1, 0xF, 0xF, true));
        r.y = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v.y), 0xB1, 0xF, 0xF, true));
        r.z = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v.z), 0xB1, 0xF, 0xF, true));
        r.w = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v.w), 0xB1, 0xF, 0xF, true));
    } else {
        r.x = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v.x), 0x4E, 0xF, 0xF, true));
        r.y = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v.y), 0x4E, 0xF, 0xF, true));
        r.z = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v.z), 0x4E, 0xF, 0xF, true));
        r.w = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v.w), 0x4E, 0xF, 0xF, true));
    }
    return r;
}

__device__ __forceinline__ float4 seq_sel(bool c, const float4 &a, const float4 &b) {
    return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

__device__ __forceinline__ bool seq_nonzero(const float4 &v) {
    return ((__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z) | __float_as_uint(v.w)) << 1) != 0u;
}

// pushes the (up to NREC, adjacent) records of every lane, lane-major
template <int NREC>
__device__ __forceinline__ void seq_push(ScatterQueue &q, const bool (&p)[NREC], const uint32_t (&k)[NREC], const float4 (&v)[NREC]) {
    int below = 0, total = 0;
#pragma unroll
    for (int r = 0; r < NREC; r++) {
        const unsigned long long m = __ballot(p[r]);
        below += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        total += (int)__popcll(m);
    }
    int idx = q.tail + below;
#pragma unroll
    for (int r = 0; r < NREC; r++) {
        if (p[r]) { const int slot = idx & SCQ_MASK; q.rows[slot] = k[r]; q.vals[slot] = v[r]; }
        idx += p[r] ? 1 : 0;
    }
    q.tail += total;
}

// One tile.  G: this wave's [16 levels][16 samples] float4 staging buffer in LDS; (u0,u1,u2): this lane's
// SAMPLE (lane & 15) position, 0 for dead samples; sg[i]: its gradients for level lvl[i] (zero when dead).
__device__ __forceinline__ void field_scatter_seq(SeqState &st, const NsrLevel *__restrict__ lds_lv, float4 *__restrict__ G,
                                                  ScatterQueue &q, float *__restrict__ gt1, float u0, float u1, float u2,
                                                  const float4 (&sg)[4], int lane, bool td, bool tc) {
    const int s = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; i++) G[field_lane_level(g, i) * 16 + s] = sg[i];
    __builtin_amdgcn_wave_barrier();
    // this lane's level
    const int l = lane >> 2, py = lane & 1, pz = (lane >> 1) & 1;
    const NsrLevel lv = lds_lv[l];
    const bool hashed = lv.use_hash != 0;
    const uint32_t mulY = hashed ? 2654435761u : lv.mul[1], mulZ = hashed ? 805459861u : lv.mul[2];     // field_corner_yz's
    const uint32_t off1 = lv.offset + 1u;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gnext = G[l * 16];
    // The records of SEQ_K consecutive samples are pushed together, lane-major: a level's records of
    // neighbouring samples (x-neighbouring rows, often one 64-byte line) then sit next to each other in the ring
    // and leave in the same atomic instruction (tools/scatter_sim.py: 21.8 -> 19.6 requests/sample for K = 2).
    bool rp[2 * SEQ_K];
    uint32_t rk[2 * SEQ_K];
    float4 rv[2 * SEQ_K];
    for (int step0 = 0; step0 < 16; step0 += SEQ_K) {
#pragma unroll
    for (int sk = 0; sk < SEQ_K; sk++) {
        const int step = step0 + sk;
        const float4 gr = gnext;
        gnext = G[l * 16 + ((step + 1) & 15)];
        const float su0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, u0), step));
        const float su1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, u1), step));
        const float su2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, u2), step));
        float f0, f1, f2;
        uint32_t c0, c1, c2;
        nsr_grid_locate(su0, lv.resolution, 1, f0, c0);
        nsr_grid_locate(su1, lv.resolution, 1, f1, c1);
        nsr_grid_locate(su2, lv.resolution, 1, f2, c2);
        // ---- how did the cell move? (same answer in the 4 lanes of a level) ----
        const int d0 = (int)(c0 - st.c0), d1 = (int)(c1 - st.c1), d2 = (int)(c2 - st.c2);
        const bool same = (d0 | d1 | d2) == 0;
        const bool sx = (d1 | d2) == 0 && (d0 == 1 || d0 == -1);
        const bool sy = (d0 | d2) == 0 && (d1 == 1 || d1 == -1);
        const bool sz = (d0 | d1) == 0 && (d2 == 1 || d2 == -1);
        const bool sxp = sx && d0 == 1, sxm = sx && d0 == -1;
        // y step up: the lanes of the LOW y corner (py = 0) continue the runs their quad neighbour (py = 1) held
        const bool takeY = sy && (py == (d1 > 0 ? 0 : 1)), giveY = sy && !takeY;
        const bool takeZ = sz && (pz == (d2 > 0 ? 0 : 1)), giveZ = sz && !takeZ;
        // ---- records that end here ----
        const bool emitA = !same && !sxm && !giveY && !giveZ && seq_nonzero(st.aA);
        const bool emitB = !same && !sxp && !giveY && !giveZ && seq_nonzero(st.aB);
        rp[2 * sk] = emitA; rk[2 * sk] = st.kA; rv[2 * sk] = st.aA;
        rp[2 * sk + 1] = emitB; rk[2 * sk + 1] = st.kB; rv[2 * sk + 1] = st.aB;
        // ---- runs that continue: where from ----
        const float4 nA = seq_quad(st.aA, true), nB = seq_quad(st.aB, true);
        const float4 mA = seq_quad(st.aA, false), mB = seq_quad(st.aB, false);
        const float4 baseA = seq_sel(same, st.aA, seq_sel(sxp, st.aB, seq_sel(takeY, nA, seq_sel(takeZ, mA, zero4))));
        const float4 baseB = seq_sel(same, st.aB, seq_sel(sxm, st.aA, seq_sel(takeY, nB, seq_sel(takeZ, mB, zero4))));
        // ---- this sample's contribution: (wx*wy)*wz, the product order of the forward interpolation ----
        const float wy = py ? f1 : 1 - f1, wz = pz ? f2 : 1 - f2;
        const float wA = ((1 - f0) * wy) * wz, wB = (f0 * wy) * wz;
        st.aA = make_float4(fmaf(wA, gr.x, baseA.x), fmaf(wA, gr.y, baseA.y), fmaf(wA, gr.z, baseA.z), fmaf(wA, gr.w, baseA.w));
        st.aB = make_float4(fmaf(wB, gr.x, baseB.x), fmaf(wB, gr.y, baseB.y), fmaf(wB, gr.z, baseB.z), fmaf(wB, gr.w, baseB.w));
        // ---- keys of the (possibly unchanged) cell: field_corner_yz / field_corner_row<false> (field_common.h) restated for both x corners ----
        if (!same) {
            const uint32_t ty = (c1 + (uint32_t)py) * mulY, tz = (c2 + (uint32_t)pz) * mulZ;
            const uint32_t comb = hashed ? (ty ^ tz) : (ty + tz);
            const uint32_t iA = hashed ? (c0 ^ comb) : (c0 * lv.mul[0] + comb);
            const uint32_t iB = hashed ? ((c0 + 1u) ^ comb) : ((c0 + 1u) * lv.mul[0] + comb);
            const uint32_t tA = __umulhi(lv.magic, iA), tB = __umulhi(lv.magic, iB);
            const uint32_t qA = (tA + ((iA - tA) >> lv.sh1)) >> lv.sh2, qB = (tB + ((iB - tB) >> lv.sh1)) >> lv.sh2;
            st.kA = off1 + (iA - qA * lv.size);
            st.kB = off1 + (iB - qB * lv.size);
            st.c0 = c0; st.c1 = c1; st.c2 = c2;
        }
    }
        if (q.tail - q.head > SCQ_CAP - 128 * SEQ_K) scq_pace(q, gt1, lane, td, tc, 16 * SEQ_K, false);
        seq_push<2 * SEQ_K>(q, rp, rk, rv);
    }
}

template <int CD>
__device__ __forceinline__ void field_tr2(const s8v (&x)[1], s4v ident, s4v (&out)[2]) {
    out[0] = mm_transpose16<CD>(mm_lo(x[0]), ident);
    out[1] = mm_transpose16<CD>(mm_hi(x[0]), ident);
}
template <int CD>
__device__ __forceinline__ void field_tr4(const s8v (&x)[2], s4v ident, s4v (&out)[4]) {
    out[0] = mm_transpose16<CD>(mm_lo(x[0]), ident);
    out[1] = mm_transpose16<CD>(mm_hi(x[0]), ident);
    out[2] = mm_transpose16<CD>(mm_lo(x[1]), ident);
    out[3] = mm_transpose16<CD>(mm_hi(x[1]), ident);
}

// wgrad of one layer (field_bwd.h): the compiler's own choice of registers for the accumulators.  Pinned to AGPRs with
// every other MFMA in VGPR form, as in the gradients-out kernel, this kernel was slower (49 -> 52 ms: its paced atomic
// drains are tuned to this schedule).
template <int CD, int NG, int NA>
__device__ __forceinline__ void field_wgrad(f4v (&acc)[NG * NA], const s4v (&Gt)[NG], const s4v (&At)[NA]) {
#pragma unroll
    for (int ot = 0; ot < NG; ot++) {
#pragma unroll
        for (int it = 0; it < NA; it++) acc[ot * NA + it] = MM<CD>::k16(Gt[ot], At[it], acc[ot * NA + it]);
    }
}

// One wave per SIMD (its 240 weight-gradient accumulators).  The schedule of the MLP section is the one measured fastest
// for this kernel on the bench frame (48.6 M samples): one net at a time (49.0 -> 48.0 ms); plain ReLU (packed v_pk_max_f16:
// 49.0 -> 49.5 ms); weight fragments read at the point of use (the scatter already separates loads from their use, and the
// read-ahead costs registers: 49.4 -> 51.2 ms); the next tile's inputs loaded right before the scatter.
template <typename TT, int CD, bool FEATS, bool DIRS = false>
__global__ void __launch_bounds__(BWD_THREADS)
k_field_bwd_tracker(FieldBwdArgsOf<DIRS> b) {
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const TT *tables = reinterpret_cast<const TT *>(a.tables);
    const uint32_t lb = field_logical_block();
    const uint32_t tpb = (ntiles + gridDim.x - 1) / gridDim.x;
    const uint32_t t_begin = lb * tpb;
    const uint32_t t_end = min(t_begin + tpb, ntiles);
    const s4v ident = mm_identity_frag<CD>(lane);
    const int nc = (int)b.nc;
    ScatterQueue q;
    char *qbase = smem + (size_t)(FWT + BW_TOTAL) * 2 + 16 * sizeof(NsrLevel) + (size_t)wave * BWD_QUEUE_BYTES_PER_WAVE;
    q.vals = reinterpret_cast<float4 *>(qbase);
    q.rows = reinterpret_cast<uint32_t *>(qbase + SCQ_CAP * 16);
    q.head = q.tail = 0;
    for (int k = lane; k < SCQ_CAP; k += 64) q.rows[k] = 0u;        // keys are row + 1: 0 matches nothing
    SeqState seq;
    seq.c0 = seq.c1 = seq.c2 = 0x7FFFFFF0u;
    seq.kA = seq.kB = 0u;
    seq.aA = seq.aB = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 *const seqG = reinterpret_cast<float4 *>(qbase + SCQ_CAP * 20);        // [16 levels][16 samples] float4 staging, 4 KB
    const bool td = b.train_density != 0, tc = b.train_color != 0;
    float *const gt1 = b.grad_tables - 4;      // ring rows are stored +1 (field_scatter_seq)
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

    // Software rotation around the in-order vmcnt counter: a tile's records are pushed to the LDS ring
    // by its (atomic-free) scatter phase, the next tile's inputs are loaded right after it, and the
    // atomics are issued by pace points inside the NEXT tile's dgrad / wgrad section, where no load
    // result is consumed.  In the straightforward order every load-use waits for a full trip of
    // freshly issued atomics to the memory-side atomic unit (41 % of the wave's cycles, SQ_WAIT_ANY).
    // Each wave walks a CONTIGUOUS quarter of the block's tiles: consecutive tiles continue the same ray,
    // so the rows of its coarse and middle levels recur and merge with records still held in the ring.
    const uint32_t wchunk = (t_end > t_begin ? (t_end - t_begin + BWD_THREADS / 64 - 1) / (BWD_THREADS / 64) : 0u);
    const uint32_t w_begin = min(t_begin + wave * wchunk, t_end), w_end = min(w_begin + wchunk, t_end);
    // A tile's raw inputs: loads only, nothing here consumes a loaded value (a use would make the compiler wait for the
    // whole memory round trip inside the prefetch).
    struct TileIn {
        float x0, x1, x2;
        s8v xd, xc;
        float gsig;        // grad_sigmas[m] (used by the g == 0 lanes)
        float grgb[4];     // grad_rgbs[m, 4g .. 4g+3]
    };
    // position `16 * tile + s` of the walk is that sample of the buffers (sample 0, always in bounds, for lanes past the count)
    auto fetch_idx = [&](uint32_t tile) -> uint32_t {
        const uint32_t m = tile * 16 + s;
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
    TileIn cur;
    if (w_begin < w_end) cur = load_tile(w_begin, fetch_idx(w_begin));
    for (uint32_t tile = w_begin; tile < w_end; tile++) {
        const uint32_t m = tile * 16 + s;
        const bool valid = m < Mc;
        const float u0 = valid ? field_unit(cur.x0, a.bmin[0], a.bsize[0]) : 0.f;
        const float u1 = valid ? field_unit(cur.x1, a.bmin[1], a.bsize[1]) : 0.f;
        const float u2 = valid ? field_unit(cur.x2, a.bmin[2], a.bsize[2]) : 0.f;
        const bool live = valid && field_in_unit_cube(u0, u1, u2);
        const float cur_gsig = valid ? cur.gsig : 0.f;
        float cur_grgb[4];
#pragma unroll
        for (int e = 0; e < 4; e++)
            cur_grgb[e] = (valid && (a.C_ch == 8 ? g < 2 : (uint32_t)(4 * g + e) < a.C_ch)) ? cur.grgb[e] : 0.f;
        // no saved features: gather them now (dependent loads, the slow path)
        if (!FEATS) field_encode<TT, CD, false>(lds_lv, tables, u0, u1, u2, live, g, cur.xd, cur.xc, a.fast_levels);

        // DIRS: this tile's direction is requested here, not a tile ahead with the other inputs (three registers the 64
        // accumulator tiles do not leave): its first use, color2's first layer, is two nets away
        float dv[3] = {0.f, 0.f, 0.f};
        if constexpr (DIRS) {
            if (valid) { dv[0] = dirs[(size_t)m * 3 + 0]; dv[1] = dirs[(size_t)m * 3 + 1]; dv[2] = dirs[(size_t)m * 3 + 2]; }
        }
        TileIn nxt{};
        f4v gxd[2], gxc[2];        // d L / d (density, colour) features of this lane's levels
        // paced drain of the previous tile's records: SCQ_PACE(n) issues <= n atomic wave-instructions
#define SCQ_PACE(n) scq_pace(q, gt1, lane, td, tc, (n), false)
        // ================= one net at a time: forward recompute -> dgrad -> wgrad, then its activations are dead ===========
        // (The straight order -- all four forwards, then all backwards -- keeps hd, hk, hc, hr1, hr2 alive together: 40
        // registers that the accumulator-heavy kernel does not have; the compiler then parks MFMA results in AGPRs and
        // copies them back, ~400 v_accvgpr_read per tile.)
        s8v xd[1] = {cur.xd}, xc[1] = {cur.xc};
        f4v h[4];
        s4v xct[2], xdt[2];
        // ---- density: 32 -> 64 -> 1 --------------------------------------------------------------------------------
        {
            s8v hd[2];
            f4v logit[1];
            mm_layer32<CD, 4, 1>(wl + FW_D1, lane, xd, h);
            mm_pack64<CD, true, false>(h, hd);
            mm_layer32<CD, 1, 2>(wl + FW_D2, lane, hd, logit);
            s4v dyd;
            {
                // sigma = exp(logit) * density_scale; trunc_exp backward clamps (tcnn_nerf.py:62-66)
                float gd = 0.f;
                if (valid && g == 0) gd = cur_gsig * a.density_scale * expf(fminf(fmaxf(logit[0][0], -15.0f), 15.0f));
                dyd[0] = MM<CD>::cvt(gd); dyd[1] = MM<CD>::cvt(0.f); dyd[2] = dyd[1]; dyd[3] = dyd[1];
            }
            s8v gh[2];
            s4v ght[4], hdt[4];
            mm_layer16<CD, 4>(wt + BW_D2T, lane, dyd, h);
            field_mask_pack<CD, false>(h, hd, gh);
            mm_layer32<CD, 2, 2>(wt + BW_D1T, lane, gh, gxd);
            SCQ_PACE(4);
            field_tr4<CD>(hd, ident, hdt);
            const s4v dydt[1] = {mm_transpose16<CD>(dyd, ident)};
            field_wgrad<CD>(w_d2, dydt, hdt);
            SCQ_PACE(4);
            field_tr2<CD>(xd, ident, xdt);
            field_tr4<CD>(gh, ident, ght);
            field_wgrad<CD>(w_d1, ght, xdt);
            SCQ_PACE(4);
        }
        field_tr2<CD>(xc, ident, xct);
        // ---- class: 32 -> 64 -> nc (rows 3..) ------------------------------------------------------------------------
        {
            s8v hk[2];
            mm_layer32<CD, 4, 1>(wl + FW_K1, lane, xc, h);
            mm_pack64<CD, true, false>(h, hk);
            s4v dyk;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int ch = 4 * g + e;
                dyk[e] = MM<CD>::cvt((valid && ch >= 3 && (uint32_t)ch < a.C_ch) ? cur_grgb[e] : 0.f);
            }
            s8v gh[2];
            s4v ght[4], hkt[4];
            mm_layer16<CD, 4>(wt + BW_K2T, lane, dyk, h);
            field_mask_pack<CD, false>(h, hk, gh);
            mm_layer32<CD, 2, 2>(wt + BW_K1T, lane, gh, gxc);
            SCQ_PACE(4);
            field_tr4<CD>(hk, ident, hkt);
            const s4v dykt[1] = {mm_transpose16<CD>(dyk, ident)};
            field_wgrad<CD>(w_k2, dykt, hkt);
            SCQ_PACE(4);
            field_tr4<CD>(gh, ident, ght);
            field_wgrad<CD>(w_k1, ght, xct);
            SCQ_PACE(4);
        }
        // ---- colour: 32 -> 64 -> 16 -> 64 -> 64 -> 3 (sigmoid) -------------------------------------------------------
        {
            s8v hc[2], hr1[2], hr2[2];
            f4v c1[1], rgb[1];
            mm_layer32<CD, 4, 1>(wl + FW_C1A, lane, xc, h);
            mm_pack64<CD, true, false>(h, hc);
            mm_layer32<CD, 1, 2>(wl + FW_C1B, lane, hc, c1);
            const s4v c1b = mm_round4<CD, false>(c1[0]);
            s4v shb = {};
            if constexpr (DIRS) {
                shb = mm_round4<CD, false>(field_sh4(g, dv[0], dv[1], dv[2]));
                const s8v b1[1] = {mm_cat(c1b, shb)};
                mm_layer32<CD, 4, 1>(wl + FW_R1, lane, b1, h);
            } else {
                mm_layer16<CD, 4>(wl + FW_R1, lane, c1b, h);
            }
            mm_pack64<CD, true, false>(h, hr1);
            mm_layer32<CD, 4, 2>(wl + FW_R2, lane, hr1, h);
            mm_pack64<CD, true, false>(h, hr2);
            SCQ_PACE(4);
            mm_layer32<CD, 1, 2>(wl + FW_R3, lane, hr2, rgb);
            s4v dyr;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int ch = 4 * g + e;
                float gr = 0.f;
                if (valid && ch < 3) {
                    const float sg = field_sigmoid(rgb[0][e]);
                    gr = cur_grgb[e] * sg * (1.0f - sg);
                }
                dyr[e] = MM<CD>::cvt(gr);
            }
            s8v g2[2], g1[2];
            s4v gc1;
            mm_layer16<CD, 4>(wt + BW_R3T, lane, dyr, h);
            field_mask_pack<CD, false>(h, hr2, g2);
            mm_layer32<CD, 4, 2>(wt + BW_R2T, lane, g2, h);
            field_mask_pack<CD, false>(h, hr1, g1);
            f4v t1[1];
            mm_layer32<CD, 1, 2>(wt + BW_R1T, lane, g1, t1);
            gc1 = mm_round4<CD, false>(t1[0]);
            {
                s4v hr2t[4], g2t[4];
                field_tr4<CD>(hr2, ident, hr2t);
                const s4v dyrt[1] = {mm_transpose16<CD>(dyr, ident)};
                field_wgrad<CD>(w_r3, dyrt, hr2t);
                SCQ_PACE(4);
                s4v hr1t[4];
                field_tr4<CD>(g2, ident, g2t);
                field_tr4<CD>(hr1, ident, hr1t);
                field_wgrad<CD>(w_r2, g2t, hr1t);
                SCQ_PACE(4);
            }
            {
                s4v g1t[4];
                field_tr4<CD>(g1, ident, g1t);
                const s4v c1t[1] = {mm_transpose16<CD>(c1b, ident)};
                field_wgrad<CD>(w_r1, g1t, c1t);
                if constexpr (DIRS) {
                    // the SH values sit in the lane layout of the color1 output tile: the same identity-MFMA transpose
                    const s4v sht[1] = {mm_transpose16<CD>(shb, ident)};
                    field_wgrad<CD>(w_sh, g1t, sht);
                }
                SCQ_PACE(4);
            }
            s8v gh[2];
            s4v ght[4], hct[4];
            mm_layer16<CD, 4>(wt + BW_C1BT, lane, gc1, h);
            field_mask_pack<CD, false>(h, hc, gh);
            mm_layer32_acc<CD, 2, 2>(wt + BW_C1AT, lane, gh, gxc);
            field_tr4<CD>(hc, ident, hct);
            const s4v gc1t[1] = {mm_transpose16<CD>(gc1, ident)};
            field_wgrad<CD>(w_c1b, gc1t, hct);
            SCQ_PACE(4);
            field_tr4<CD>(gh, ident, ght);
            field_wgrad<CD>(w_c1a, ght, xct);
            SCQ_PACE(4);
        }
#undef SCQ_PACE
        // Next tile's loads go out BEFORE this tile's scatter: the scatter touches LDS only (its records are
        // turned into atomics by the pace points of the next tile), so by the next loop top both these loads
        // and the atomics issued ahead of them (vmcnt retires in order) have had the whole scatter to land.
        // (exactly this shape -- moving the loads costs the tracker several ms)
        nxt = cur;
        if (tile + 1 < w_end) nxt = load_tile(tile + 1, fetch_idx(tile + 1));

        // ================= table scatter =======================================================
        // gxd[t][2*(i&1)+f] is d L / d feature f of level lvl[i] (t = i >> 1): same lane<->level map
        // as the forward encode.  The scatter is VALU + LDS only: its records go to the ring and leave as
        // atomics at the pace points of the NEXT tile's dgrad / wgrad section.
        if (td || tc) {
            float4 sg[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int t = i >> 1, e0 = 2 * (i & 1);
                sg[i] = live ? make_float4(gxd[t][e0], gxd[t][e0 + 1], gxc[t][e0], gxc[t][e0 + 1]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            field_scatter_seq(seq, lds_lv, seqG, q, gt1, live ? u0 : 0.f, live ? u1 : 0.f, live ? u2 : 0.f, sg, lane, td, tc);
        }
        cur = nxt;
    }
    if (td || tc) {
        // close the runs still open in registers
        if (q.tail - q.head > SCQ_CAP - 128) scq_pace(q, gt1, lane, td, tc, 16, false);
        const bool fp[2] = {seq_nonzero(seq.aA), seq_nonzero(seq.aB)};
        const uint32_t fk[2] = {seq.kA, seq.kB};
        const float4 fv[2] = {seq.aA, seq.aB};
        seq_push<2>(q, fp, fk, fv);
        scq_pace(q, gt1, lane, td, tc, 1 << 20, true);
    }
    if (b.grad_mlp) {
        f4v *const red = reinterpret_cast<f4v *>(smem);
#define NSR_RED_ALL(OP)                                                                                              \
        OP(w_r3, 0, 4) OP(w_r2, 4, 16) OP(w_r1, 20, 4) OP(w_c1b, 24, 4) OP(w_c1a, 28, 8) OP(w_k2, 36, 4) OP(w_k1, 40, 8)     \
        OP(w_d2, 48, 4) OP(w_d1, 52, 8)
        __syncthreads();                                   // every wave is done with the weight fragments
        for (int w = 0; w < BWD_THREADS / 64; w++) {
            if (wave == w) {
                // (DIRS: tiles 60..63 lie past the two weight images, over the level table and the head of wave 0's ring --
                // every wave has flushed its ring by now)
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

static int field_bwd_launch_tracker(const FieldBwdArgs &b, int table_dtype, int compute_dtype, bool feats, dim3 grid, hipStream_t s,
                                    const float *dirs) {
    return field_bwd_dispatch(table_dtype, compute_dtype, feats, [&](auto tt, auto cd, auto ft) {
        if (dirs) {
            const FieldBwdDirsArgs bd = field_bwd_with_dirs(b, dirs);
            return nsr_launch_lds<k_field_bwd_tracker<decltype(tt), cd(), ft(), true>>(BWD_LDS_BYTES_DIRS, grid, dim3(BWD_THREADS),
                                                                                       BWD_LDS_BYTES_DIRS, s, bd);
        }
        return nsr_launch_lds<k_field_bwd_tracker<decltype(tt), cd(), ft()>>(BWD_LDS_BYTES, grid, dim3(BWD_THREADS), BWD_LDS_BYTES, s, b);
    });
}

static int field_backward_any(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs, uint32_t M,
                              const int32_t *m_dev, const float *grad_sigmas, const float *grad_rgbs, float *grad_tables,
                              float *grad_mlp, int train_density_table, int train_color_table, const void *feats,
                              const uint32_t *perm, void *workspace, const float *dirs, nsr_stream_t stream);

extern "C" {

uint64_t nsr_field_backward_workspace_bytes(uint32_t M, int with_perm) {
    return with_perm ? (uint64_t)M * 16 * sizeof(float4) : 0;        // the [M][16] float4 encoder-gradient buffer
}

int nsr_field_backward(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs, uint32_t M,
                       const int32_t *m_dev, const float *grad_sigmas, const float *grad_rgbs, float *grad_tables,
                       float *grad_mlp, int train_density_table, int train_color_table, const void *feats,
                       const uint32_t *perm, void *workspace, nsr_stream_t stream) {
    return field_backward_any(desc, tables, mlp_params, xyzs, M, m_dev, grad_sigmas, grad_rgbs, grad_tables, grad_mlp,
                              train_density_table, train_color_table, feats, perm, workspace, nullptr, stream);
}

int nsr_field_backward_dirs(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs, uint32_t M,
                            const int32_t *m_dev, const float *grad_sigmas, const float *grad_rgbs, float *grad_tables,
                            float *grad_mlp, int train_density_table, int train_color_table, const void *feats,
                            const uint32_t *perm, void *workspace, const float *dirs, nsr_stream_t stream) {
    if (M == 0) return NSR_OK;
    NSR_CHECK_PTR(dirs);
    return field_backward_any(desc, tables, mlp_params, xyzs, M, m_dev, grad_sigmas, grad_rgbs, grad_tables, grad_mlp,
                              train_density_table, train_color_table, feats, perm, workspace, dirs, stream);
}

}   // extern "C"

static int field_backward_any(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs, uint32_t M,
                              const int32_t *m_dev, const float *grad_sigmas, const float *grad_rgbs, float *grad_tables,
                              float *grad_mlp, int train_density_table, int train_color_table, const void *feats,
                              const uint32_t *perm, void *workspace, const float *dirs, nsr_stream_t stream) {
    if (M == 0) return NSR_OK;
    NSR_CHECK_PTR(desc); NSR_CHECK_PTR(tables); NSR_CHECK_PTR(mlp_params); NSR_CHECK_PTR(xyzs);
    NSR_CHECK_PTR(grad_sigmas); NSR_CHECK_PTR(grad_rgbs);
    if ((train_density_table || train_color_table) && grad_tables == nullptr) return NSR_ERR_INVALID_ARG;
    FieldBwdArgs b;
    uint32_t nblocks;
    const int st = field_fill_args(desc, tables, mlp_params, b.f, M, nblocks);
    if (st != NSR_OK) return st;
    // 4-wave workgroups, one wave per SIMD (each wave needs the 512-register budget): one
    // workgroup per CU is resident, each walks a contiguous range of tiles
    const uint32_t ntiles = (M + 15) / 16;
    nblocks = (ntiles + 3) / 4;
    if (nblocks > 256) nblocks = 256;
    b.f.tiles_per_block = (ntiles + nblocks - 1) / nblocks;
    b.f.xyzs = xyzs; b.f.m_dev = m_dev; b.f.sigmas = nullptr; b.f.rgbs = nullptr;
    const bool gout = perm != nullptr && (train_density_table || train_color_table);
    // `feats` given together with `perm` were written by nsr_field_forward in perm's order (tile-major): the gradients-out
    // kernel walks the same order; the fused tracker kernel walks the buffers and cannot use them (it re-gathers)
    if (perm != nullptr && !gout) feats = nullptr;
    b.f.feats = const_cast<void *>(feats);
    b.f.perm = (gout && feats != nullptr) ? perm : nullptr;
    b.gout = nullptr;
    if (gout) {
        if (workspace == nullptr || ((uintptr_t)workspace & 15u)) return NSR_ERR_INVALID_ARG;
        if (!nsr_table_scatter_supported(b.f.lv)) return NSR_ERR_UNSUPPORTED;   // grid too fine for the 10-bit blocks: call without perm
        b.gout = (float4 *)workspace;
    }
    if (feats && ((uintptr_t)feats & 15u)) return NSR_ERR_INVALID_ARG;
    b.grad_sigmas = grad_sigmas; b.grad_rgbs = grad_rgbs; b.grad_tables = grad_tables; b.grad_mlp = grad_mlp;
    b.train_density = train_density_table; b.train_color = train_color_table; b.nc = desc->num_classes;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(nblocks);
    if (!gout) return field_bwd_launch_tracker(b, desc->table_dtype, desc->compute_dtype, feats != nullptr, grid, s, dirs);
    const int st1 = nsr_field_bwd_launch_gout(b, desc->table_dtype, desc->compute_dtype, feats != nullptr, grid, s, dirs);
    if (st1 != NSR_OK) return st1;
    // second kernel: the table scatter in the permutation's order, many waves per CU
    return nsr_table_scatter_launch(b.f.lv, b.f.bmin, b.f.bsize, xyzs, perm, m_dev, M, workspace, grad_tables, train_density_table,
                                    train_color_table, s);
}
