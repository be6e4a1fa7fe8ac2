// Stand-alone table scatter of the fused field backward, gfx950 (the spatially ordered path).
//
// nsr_field_backward with a `perm` (nsr_sample_order) runs the MLP backward kernel in "gradients out" mode -- it writes
// d loss / d (encoder output) of every sample, 256 B, instead of scattering -- and then THIS kernel, which walks the
// samples in the permutation's spatial order and accumulates the table gradient.  Why two kernels: the MLP backward
// needs one wave per SIMD (240 weight-gradient accumulators per lane), and the scatter is a chain of dependent LDS
// round trips and atomics that one wave per SIMD cannot hide (measured fused: MLP 13.8 ms + scatter 32 ms on the bench
// frame).  Here a wave needs 166 registers and ~11 KB of LDS, so three of them share a SIMD.
//
// Lattice accumulator.  The order's key is the sample's BLOCK: its encoder input quantised to 10 bits per axis (a 4^3
// group of finest-level cells for the reference's 16-level grid).  Consecutive samples -- of MANY rays -- share a block,
// and a block touches only a handful of cells on every level: at most ceil(res_l / 1024) + 1 per axis.  So the wave
// keeps, per level, a small LATTICE of corner gradients in LDS anchored at the cell of the block's origin (ceil(res / 1024)
// + 2 corners per axis: for the reference's LLFF grid -- 16 levels, resolutions 16 .. 4096 -- 5^3 on the two finest levels,
// 4^3 on the next two and 3^3 below, 702 float4 = 11 KB per wave; grids up to 6^3 per level and 960 slots in all are
// accepted).  Lane = (level l = lane >> 2, y/z corner pair p = lane & 3) walks the samples in order and adds its two x
// corners' contributions with a plain LDS read-modify-write: within a step the 64 lanes touch 128 different slots and
// steps are sequential, so no atomics are needed; the lattice is addressed by cell coordinates, so nothing is hashed per
// sample.
//
// When the walk enters a new block every level re-anchors.  A level whose anchor cell did not change (the coarse ones: a
// block is a fraction of their cell) keeps accumulating.  A level whose anchor moved by d <= S - 1 cells along +x ONLY --
// the walk is in Morton order with x as bit 0, so this is the step from an x-even block to its +x neighbour, every
// second block change where space is filled -- SHIFTS: the planes x < d leave the window and are flushed, the planes
// x >= d are corners of the new lattice as well and move down by d inside the same LDS slots, where the new block's
// samples join them before anything goes to memory.  Without that the shared face left as lonely rows (on the finest level
// the anchor is a multiple of 4 cells: corners 0..3 of an x-row fill a 64-byte line of the gradient table, corner 4 is alone
// in the next one) and came back one block later as part of a full line.  Every other move (y or z changed, a step
// backwards, a step past the window) flushes the whole lattice, and so does the end of the wave's range.  A flush is
// cooperative, one merged record per corner a block touched, and its atomic instructions carry whole x-rows, so the
// corners of a row that share a line leave as one request (lat_flush_level).  Requests per sample on the bench frame,
// model and counter: DESIGN.md, "(r4) requests per sample"; tools/sorted_scatter_sim.py is the model.
#include "field_common.h"
#include "lattice.h"
#include "table_scatter.h"


__device__ __forceinline__ bool seq_nonzero(const float4 &v) {
    return ((__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z) | __float_as_uint(v.w)) << 1) != 0u;
}

constexpr int TS_THREADS = 256;     // measured on the bench frame: 64 -> 35.6 ms, 128 -> 30.6, 256 -> 29.4 (A + B)
// float4 slots per wave, from the 64 KB of LDS a workgroup may ask for: level table + per wave (256 B + 16 B per slot), the
// slot count rounded up to 64 (4 waves: 960).  nsr_table_scatter_supported() and the launch share THIS bound, so a grid is
// rejected before anything is launched or never (round 2 rejected totals of 961..1024 after the MLP backward had run)
constexpr int LAT_MAX_SLOTS = (int)(((65536 - 16 * sizeof(NsrLevel)) / (TS_THREADS / 64) - 256) / 16 / 64 * 64);
struct LatState {
    uint32_t b0, b1, b2;     // anchor cell of this lane's level (LAT_NONE: nothing accumulated yet)
};

// Flushes the planes x < xl of level l's lattice, anchored at cell (b0, b1, b2), and moves the planes x >= xl down to x - xl
// (xl, like the anchor, is wave-uniform; xl == S: the whole lattice leaves and is cleared, nothing moves).
// A trip covers four groups of 16 / S whole x-rows (S = 3: 15 slots per group, 4: 16, 5: 15, 6: 12; the other lanes idle), so
// that no x-row is cut in two by an atomic instruction: the corners of a row are neighbours in the table (x is the index's
// lowest term, hashed or dense) and share their 64-byte lines only inside ONE instruction.  Four phases, so that nothing is
// computed four times and every LDS round trip is shared:
//   1. one lane per slot: read its float4, test it, and (touched slots of the leaving planes only) compute the table row
//      ONCE -> rows[lane];
//   2. the four groups, skipped when empty: lane (t = lane >> 2, i = lane & 3) reads component i of the group's slot t and
//      its row and issues the atomic -- the four dwords of a row leave as ONE 16-byte request;
//   3. the touched slots are cleared;
//   4. the touched slots of the staying planes are written back xl slots lower (same x-row, hence same trip; every lane
//      still holds its slot's value from phase 1, and the LDS executes a wave's accesses in order).
template <int S>
__device__ __forceinline__ void lat_flush_level(float4 *__restrict__ lat4, uint32_t *__restrict__ rows, uint32_t b0, uint32_t b1, uint32_t b2,
                                                const NsrLevel &lv, float *__restrict__ gt, int lane, bool td, bool tc, uint32_t xl) {
    constexpr int NC = S * S * S;
    constexpr int RS = (16 / S) * S;                                      // slots per 16-lane group: whole x-rows
    const int t = lane >> 2, i = lane & 3;
    const int g = lane >> 4, j = lane & 15;
    const bool on = (i < 2) ? td : tc;
    const float *lf = reinterpret_cast<const float *>(lat4);
#pragma unroll 1
    for (int k0 = 0; k0 < NC; k0 += 4 * RS) {
        const int k = k0 + g * RS + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < RS && k < NC) v = lat4[k];
        const bool nz = seq_nonzero(v);
        if (__ballot(nz) == 0ull) continue;                               // wave-uniform: nothing touched in these slots
        bool out = false;
        if (nz) {
            // k < 256: the divisions by S*S and S are 24-bit multiplies by 16-bit reciprocals (exact on this range); a 32-bit
            // integer multiply costs four issue slots on this machine and the scatter is issue bound
            constexpr uint32_t MZ = (65536u + S * S - 1u) / (S * S), MY = (65536u + S - 1u) / S;
            const uint32_t z = __umul24((uint32_t)k, MZ) >> 16, r = (uint32_t)k - __umul24(z, (uint32_t)(S * S));
            const uint32_t y = __umul24(r, MY) >> 16, x = r - __umul24(y, (uint32_t)S);
            out = x < xl;
            if (out) rows[lane] = lv.offset + lat_row(lv, b0 + x, b1 + y, b2 + z);
        }
        const unsigned long long m = __ballot(out);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (k0 + RS * q >= NC) break;
            if (((m >> (16 * q)) & 0xFFFFull) == 0ull) continue;          // wave-uniform
            const bool rec = (m >> (16 * q + t)) & 1ull;
            if (rec) {
                const float val = lf[(k0 + RS * q + t) * 4 + i];
                const uint32_t row = rows[16 * q + t];
                if (on) atomicAdd(gt + (size_t)row * 4 + i, val);
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (nz) lat4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        __builtin_amdgcn_wave_barrier();
        if (nz && !out) lat4[k - (int)xl] = v;                            // x >= xl: never for a whole-lattice flush
    }
}

// The geometry of level fl comes from the LDS copy of the level table (pad_ = S | shift << 4 | base << 8): a read from the
// kernel-argument segment here would be a vector-memory load, and waiting for it means waiting for every atomic in flight.
// xl_lane: the number of leaving x planes of the lane's own level (lat_flush_level's xl); the lanes of a level agree.
__device__ __forceinline__ void lat_flush_dispatch(float4 *__restrict__ lat, int fl, const LatState &st, uint32_t xl_lane,
                                                   const NsrLevel *__restrict__ lds_lv, float *__restrict__ gt, int lane, bool td, bool tc) {
    const uint32_t o0 = (uint32_t)__builtin_amdgcn_readlane((int)st.b0, fl * 4);
    if (o0 == LAT_NONE) return;
    const uint32_t o1 = (uint32_t)__builtin_amdgcn_readlane((int)st.b1, fl * 4);
    const uint32_t o2 = (uint32_t)__builtin_amdgcn_readlane((int)st.b2, fl * 4);
    const uint32_t xl = (uint32_t)__builtin_amdgcn_readlane((int)xl_lane, fl * 4);
    const NsrLevel flv = lds_lv[fl];
    float4 *lf = lat + (flv.pad_ >> 8);
    uint32_t *rows = reinterpret_cast<uint32_t *>(lat) - 64;                  // 64-entry row scratch in front of the lattices
    switch (flv.pad_ & 0xFu) {
    case 3: lat_flush_level<3>(lf, rows, o0, o1, o2, flv, gt, lane, td, tc, xl); break;
    case 4: lat_flush_level<4>(lf, rows, o0, o1, o2, flv, gt, lane, td, tc, xl); break;
    case 5: lat_flush_level<5>(lf, rows, o0, o1, o2, flv, gt, lane, td, tc, xl); break;
    default: lat_flush_level<6>(lf, rows, o0, o1, o2, flv, gt, lane, td, tc, xl); break;
    }
}


struct TableScatterArgs {
    const float *xyzs;
    const uint32_t *perm;
    const int32_t *m_dev;
    uint32_t M;
    const float4 *gin;            // [M][16] float4: d loss / d (density f0, f1, colour f0, f1) per level
    float *grad_tables;
    float bmin[3], bsize[3];
    int td, tc;
    uint32_t lat_slots;           // float4 slots per wave (multiple of 64)
    NsrLevel lv[16];              // pad_ = S | shift << 4 | base << 8
};

constexpr int TS_RING = 8;          // gradient rows in flight per wave
static_assert(TS_RING % 4 == 0, "a quad of steps (one locate pass) must not straddle two parts of the ring");

// v of lane (lane & ~3) + K of the caller's group of four lanes (DPP quad_perm: no LDS, no scalar round trip)
template <int K>
__device__ __forceinline__ int quad_lane(int v) {
    return __builtin_amdgcn_update_dpp(0, v, K * 0x55, 0xF, 0xF, true);      // every lane has a source: `old` is never taken
}
__device__ __forceinline__ int quad_lane_i(int v, int k) {
    switch (k & 3) {                                                  // k is a constant wherever this is called: the switch folds
    case 0: return quad_lane<0>(v);
    case 1: return quad_lane<1>(v);
    case 2: return quad_lane<2>(v);
    default: return quad_lane<3>(v);
    }
}
__device__ __forceinline__ float quad_lane_f(float v, int k) {
    return __builtin_bit_cast(float, quad_lane_i(__builtin_bit_cast(int, v), k));
}

static size_t ts_wave_bytes(uint32_t lat_slots) { return 256 + (size_t)lat_slots * 16; }

__global__ void __launch_bounds__(TS_THREADS)
k_table_scatter(TableScatterArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    NsrLevel *lds_lv = reinterpret_cast<NsrLevel *>(smem);
    if (threadIdx.x < 16) lds_lv[threadIdx.x] = a.lv[threadIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char *base = smem + 16 * sizeof(NsrLevel) + (size_t)wave * (256 + (size_t)a.lat_slots * 16);
    float4 *lat = reinterpret_cast<float4 *>(base + 256);               // the 64-entry row scratch sits in front of it
    for (uint32_t k = lane; k < a.lat_slots; k += 64) lat[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    const uint32_t Mc = FIELD_COUNT(a);
    if (Mc == 0) return;
    const uint32_t ntiles = (Mc + 15) / 16;
    const uint32_t nwaves = gridDim.x * (TS_THREADS / 64), gw = blockIdx.x * (TS_THREADS / 64) + wave;
    const uint32_t per = (ntiles + nwaves - 1) / nwaves;
    const uint32_t w_begin = min(gw * per, ntiles), w_end = min(w_begin + per, ntiles);
    if (w_begin >= w_end) return;
    const int s = lane & 15;
    const int l = lane >> 2, py = lane & 1, pz = (lane >> 1) & 1;
    const NsrLevel lv = lds_lv[l];
    const uint32_t S = lv.pad_ & 0xFu, ashift = (lv.pad_ >> 4) & 0xFu;
    float4 *const mylat = lat + (lv.pad_ >> 8) + ((uint32_t)pz * S + (uint32_t)py) * S;
    const bool td = a.td != 0, tc = a.tc != 0;
    float *const gt = a.grad_tables;
    const float kq = (float)(1 << LAT_KEY_BITS), rk = 1.0f / kq;
    LatState st;
    st.b0 = st.b1 = st.b2 = LAT_NONE;
    uint32_t cur_key = LAT_NONE;
    // Round 3: the per-step index arithmetic runs in fp32 (cells, anchors and lattice coordinates are integers < 2^24: exact),
    // which saves the three float->int conversions, the 24-bit integer multiplies and a quarter-rate 64-bit multiply-add of
    // the slot address; the corner weights of the lane's fixed (y, z) corner are one FMA each (w = f * s + o with (s, o) =
    // (1, 0) or (-1, 1)).  The kernel is instruction-issue bound: ~300 issue cycles per step per wave, 168 of them VALU.
    float bf0 = 0.f, bf1 = 0.f, bf2 = 0.f;                           // the anchor (st.b*) as floats
    const float lscale = (float)lv.resolution;                        // nsr_grid_locate with align_corners = 1
    const float lcmax = (float)(lv.resolution - 1u);
    const float Sf = (float)S, Sm2 = (float)(S - 2u);
    const float sy = py ? 1.0f : -1.0f, oy = py ? 0.0f : 1.0f, sz = pz ? 1.0f : -1.0f, oz = pz ? 0.0f : 1.0f;

    // position 16 * tile + s of the order -> buffer index; lanes past the count read the last valid entry (masked later)
    auto fetch_idx = [&](uint32_t tile) -> uint32_t { return a.perm[min(tile * 16 + (uint32_t)s, Mc - 1u)]; };
    uint32_t idx = fetch_idx(w_begin);
    uint32_t idx_next = w_begin + 1 < w_end ? fetch_idx(w_begin + 1) : idx;
    float x0 = a.xyzs[(size_t)idx * 3], x1 = a.xyzs[(size_t)idx * 3 + 1], x2 = a.xyzs[(size_t)idx * 3 + 2];
    // The per-level gradients of the next TS_RING samples, in registers: a 256-byte row gathered by sample index is a
    // full HBM round trip (~1 us under load), far longer than a step, so a row is requested 8 steps before its use (a
    // one-step-ahead prefetch was the first version).  ts_gin(v, ln): level l's row of the sample of lane ln's index v.
    auto ts_gin = [&](uint32_t v, int ln) { return a.gin[(size_t)(uint32_t)__builtin_amdgcn_readlane((int)v, ln) * 16 + l]; };
    float4 gq[TS_RING];
#pragma unroll
    for (int i = 0; i < TS_RING; i++) gq[i] = ts_gin(idx, i);

    // The locate of a (sample, level) pair -- cell, fractions, lattice slot -- is the same for the four lanes of a level, so
    // it runs once per QUAD of steps, not in every step: before steps 4q .. 4q + 3 lane (l, j = lane & 3) locates sample
    // 4q + j on its own level, 64 different records in one pass, and in step 4q + k the lanes of a level read theirs from
    // lane 4l + k (quad_lane_f).  A record: the slot relative to the lane-independent part of the level's lattice, the three
    // fractions, and one bit of rq_past ("fp32 rounding put the cell past the lattice", bit = the lane that holds the record).
    // The records are relative to the anchors: a re-anchor inside a quad runs the pass again.
    float rq_f0 = 0.f, rq_f1 = 0.f, rq_f2 = 0.f;
    uint32_t rq_slot = 0u;
    unsigned long long rq_past = 0ull;
    float us0 = 0.f, us1 = 0.f, us2 = 0.f;                            // this tile's u, 0 for a dead sample (see below)
    const int rq_lane4 = (lane & 3) * 4;
    auto locate_quad = [&](int q) {
        const int from = q * 16 + rq_lane4;                           // byte address of lane 4q + j, which holds sample 4q + j
        const float su0 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from, __builtin_bit_cast(int, us0)));
        const float su1 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from, __builtin_bit_cast(int, us1)));
        const float su2 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from, __builtin_bit_cast(int, us2)));
        // nsr_grid_locate (align_corners = 1) with the cell kept as a float: p = u * res, c = min(floor(p), res - 1), f = p - c
        float cf0, cf1, cf2;
        {
#pragma clang fp contract(off)
            const float p0 = su0 * lscale, p1 = su1 * lscale, p2 = su2 * lscale;
            cf0 = fminf(floorf(p0), lcmax); cf1 = fminf(floorf(p1), lcmax); cf2 = fminf(floorf(p2), lcmax);
            rq_f0 = p0 - cf0; rq_f1 = p1 - cf1; rq_f2 = p2 - cf2;
        }
        // cell relative to the anchor: 0 .. S - 2 by construction for a live sample (it lies in the block the anchor was taken
        // from; floor(u * res) is monotonic in u), where the median is min(d, S - 2).  The records of dead samples and of
        // samples in front of a re-anchor are never read; the lower bound only keeps their slot a number.
        const float d0 = cf0 - bf0, d1 = cf1 - bf1, d2 = cf2 - bf2;
        const float r0 = __builtin_amdgcn_fmed3f(d0, 0.0f, Sm2), r1 = __builtin_amdgcn_fmed3f(d1, 0.0f, Sm2),
                    r2 = __builtin_amdgcn_fmed3f(d2, 0.0f, Sm2);
        rq_slot = (uint32_t)fmaf(fmaf(r2, Sf, r1), Sf, r0);
        rq_past = __ballot(fmaxf(d0, fmaxf(d1, d2)) > Sm2);
    };

    for (uint32_t tile = w_begin; tile < w_end; tile++) {
        // next tile's inputs: the permutation entry was fetched one tile ahead, so these loads depend on nothing in flight
        float nx0 = x0, nx1 = x1, nx2 = x2;
        uint32_t idx_nn = idx_next;
        if (tile + 1 < w_end) {
            nx0 = a.xyzs[(size_t)idx_next * 3]; nx1 = a.xyzs[(size_t)idx_next * 3 + 1]; nx2 = a.xyzs[(size_t)idx_next * 3 + 2];
            if (tile + 2 < w_end) idx_nn = fetch_idx(tile + 2);
        }
        const bool valid = tile * 16 + (uint32_t)s < Mc;
        const float u0 = field_unit(x0, a.bmin[0], a.bsize[0]), u1 = field_unit(x1, a.bmin[1], a.bsize[1]),
                    u2 = field_unit(x2, a.bmin[2], a.bsize[2]);
        const bool live = valid && field_in_unit_cube(u0, u1, u2);
        const uint32_t live16 = (uint32_t)(__ballot(live) & 0xFFFFull);      // lanes 0..15 are samples 0..15
        // what locate_quad reads: a dead sample (outside the cube, NaN, behind the count) is located at u = 0, so that its
        // record -- which no step reads -- is made of numbers
        us0 = live ? u0 : 0.0f; us1 = live ? u1 : 0.0f; us2 = live ? u2 : 0.0f;
        // this lane's sample's block: the sort key's quantisation (sample_order.hip), 10 bits per axis
        const uint32_t q0 = (uint32_t)fminf(fmaxf(u0 * kq, 0.0f), kq - 1.0f), q1 = (uint32_t)fminf(fmaxf(u1 * kq, 0.0f), kq - 1.0f),
                       q2 = (uint32_t)fminf(fmaxf(u2 * kq, 0.0f), kq - 1.0f);
        const uint32_t bkey = q0 | (q1 << LAT_KEY_BITS) | (q2 << (2 * LAT_KEY_BITS));
        // steps at which the block key MAY differ from the previous live sample's: this sample's key against its left
        // neighbour's (lane 0: against the key the walk is in; dead samples carry a sentinel, so the live sample after one is
        // always flagged).  The exact test runs inside the flagged steps only -- one scalar bit test per step instead of a
        // cross-lane read and a compare.
        const uint32_t bkey_e = live ? bkey : LAT_NONE;
        const uint32_t bkey_l = (uint32_t)__builtin_amdgcn_update_dpp((int)cur_key, (int)bkey_e, 0x111, 0xF, 0xF, false);   // row_shr:1
        const uint32_t chg16 = (uint32_t)(__ballot(bkey_e != bkey_l) & 0xFFFFull);
#pragma unroll 1
        for (int part = 0; part < 16 / TS_RING; part++) {
            // refills: the rest of this tile first, then the head of the next one (its permutation entries are already here)
            const bool wrap = part == 16 / TS_RING - 1;
            const uint32_t src = wrap ? idx_next : idx;
            const int src_lane0 = wrap ? 0 : (part + 1) * TS_RING;
#pragma unroll
            for (int ri = 0; ri < TS_RING; ri++) {
                const int step = part * TS_RING + ri;
                const float4 gr = gq[ri];
                if ((ri & 3) == 0 && ((live16 >> step) & 0xFu)) locate_quad(step >> 2);       // wave-uniform
                if ((live16 >> step) & 1u) {                                       // wave-uniform
                    uint32_t key = cur_key;
                    if ((chg16 >> step) & 1u) key = (uint32_t)__builtin_amdgcn_readlane((int)bkey, step);       // wave-uniform
                    if (key != cur_key) {
                        // ---- the walk enters another block: re-anchor every level at the cell of the block's origin ----
                        cur_key = key;
                        // origin of the group of 2^ashift blocks (this lane's level) the block belongs to
                        const uint32_t kq0 = key & ((1u << LAT_KEY_BITS) - 1u), kq1 = (key >> LAT_KEY_BITS) & ((1u << LAT_KEY_BITS) - 1u),
                                       kq2 = key >> (2 * LAT_KEY_BITS);
                        const float o0 = (float)((kq0 >> ashift) << ashift) * rk, o1 = (float)((kq1 >> ashift) << ashift) * rk,
                                    o2 = (float)((kq2 >> ashift) << ashift) * rk;
                        float ff;
                        uint32_t n0, n1, n2;
                        nsr_grid_locate(o0, lv.resolution, 1, ff, n0);
                        nsr_grid_locate(o1, lv.resolution, 1, ff, n1);
                        nsr_grid_locate(o2, lv.resolution, 1, ff, n2);
                        const bool chg = (n0 != st.b0) | (n1 != st.b1) | (n2 != st.b2);
                        // Shift-carry: the anchor moved along +x only and by less than the lattice is wide (in Morton order
                        // with x as bit 0, the block after an x-even block is its +x neighbour whenever that one holds
                        // samples): the planes x >= n0 - b0 are corners of the new lattice too -- they stay, moved down,
                        // and only the planes that leave the window are flushed.  Anything else (y or z moved, a step
                        // backwards or past the window, no anchor yet) flushes the whole lattice.
                        const uint32_t dx = n0 - st.b0;
                        const bool carry = (st.b0 != LAT_NONE) & (n1 == st.b1) & (n2 == st.b2) & (dx - 1u < S - 1u);
                        const uint32_t xl = carry ? dx : S;
                        unsigned long long mm = __ballot(chg);
                        while (mm) {
                            const int fl = (int)(__builtin_ctzll(mm) >> 2);
                            mm &= ~(0xFull << (fl * 4));
                            lat_flush_dispatch(lat, fl, st, xl, lds_lv, gt, lane, td, tc);
                        }
                        if (chg) { st.b0 = n0; st.b1 = n1; st.b2 = n2; bf0 = (float)n0; bf1 = (float)n1; bf2 = (float)n2; }
                        // the quad's records were taken against the old anchors: again for this and the steps to come (if no
                        // level moved they come out the same; the steps before this one are done with theirs)
                        if (__ballot(chg)) locate_quad(step >> 2);
                    }
                    // this step's record of the lane's level, from the lane of the quad that located sample `step`
                    // (step & 3 == ri & 3, a constant of the unrolled loop: TS_RING is a multiple of 4)
                    const float f0 = quad_lane_f(rq_f0, ri), f1 = quad_lane_f(rq_f1, ri), f2 = quad_lane_f(rq_f2, ri);
                    const uint32_t rslot = (uint32_t)quad_lane_i((int)rq_slot, ri);
                    // this sample's contribution to the lane's two x corners
                    const float wyz = fmaf(f1, sy, oy) * fmaf(f2, sz, oz);
                    float wB = f0 * wyz, wA = wyz - wB;
                    if (rq_past & (0x1111111111111111ull << (ri & 3))) {           // wave-uniform: some level's cell is past its lattice
                        // fp32 rounding put the cell one past the lattice (u * res of a sample at the very end of its block can round
                        // up across a cell boundary that the block's real extent stops short of): this sample's two corners go
                        // straight to the table, exactly; the (clamped) lattice slots get nothing.  The absolute cell, as
                        // locate_quad computed it:
                        const float su0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, us0), step));
                        const float su1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, us1), step));
                        const float su2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, us2), step));
                        float cf0, cf1, cf2;
                        {
#pragma clang fp contract(off)
                            cf0 = fminf(floorf(su0 * lscale), lcmax); cf1 = fminf(floorf(su1 * lscale), lcmax);
                            cf2 = fminf(floorf(su2 * lscale), lcmax);
                        }
                        if ((rq_past >> ((lane & ~3) | (ri & 3))) & 1ull) {
                            const uint32_t c0 = (uint32_t)cf0, c1 = (uint32_t)cf1, c2 = (uint32_t)cf2;
                            const uint32_t rowA = lv.offset + lat_row(lv, c0, c1 + (uint32_t)py, c2 + (uint32_t)pz);
                            const uint32_t rowB = lv.offset + lat_row(lv, c0 + 1u, c1 + (uint32_t)py, c2 + (uint32_t)pz);
                            const float ga[4] = {gr.x, gr.y, gr.z, gr.w};
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                if ((i < 2 ? td : tc) && ga[i] != 0.0f) {
                                    atomicAdd(gt + (size_t)rowA * 4 + i, wA * ga[i]);
                                    atomicAdd(gt + (size_t)rowB * 4 + i, wB * ga[i]);
                                }
                            }
                            wA = 0.0f;
                            wB = 0.0f;
                        }
                    }
                    float4 *const slot = mylat + rslot;
                    float4 va = slot[0], vb = slot[1];
                    va.x = fmaf(wA, gr.x, va.x); va.y = fmaf(wA, gr.y, va.y); va.z = fmaf(wA, gr.z, va.z); va.w = fmaf(wA, gr.w, va.w);
                    vb.x = fmaf(wB, gr.x, vb.x); vb.y = fmaf(wB, gr.y, vb.y); vb.z = fmaf(wB, gr.z, vb.z); vb.w = fmaf(wB, gr.w, vb.w);
                    slot[0] = va;
                    slot[1] = vb;
                }
                // the slot's refill is issued AFTER the last use of its old value, so every ring slot stays in the same registers
                // (a refill issued earlier gets other registers, and the copies at the loop edge wait for every load in flight)
                asm volatile("" ::: "memory");
                gq[ri] = ts_gin(src, src_lane0 + ri);
            }
        }
        x0 = nx0; x1 = nx1; x2 = nx2;
        idx = idx_next;
        idx_next = idx_nn;
    }
    // every level's lattice leaves
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int fl = 0; fl < 16; fl++) lat_flush_dispatch(lat, fl, st, S, lds_lv, gt, lane, td, tc);
}

bool nsr_table_scatter_supported(const NsrLevel *lv) {
    LatGeom g;
    return lat_geometry(lv, g, (uint32_t)LAT_MAX_SLOTS);
}

int nsr_table_scatter_launch(const NsrLevel *levels, const float *bmin, const float *bsize, const float *xyzs, const uint32_t *perm,
                             const int32_t *m_dev, uint32_t M, const void *gin, float *grad_tables, int td, int tc, hipStream_t s) {
    TableScatterArgs a;
    LatGeom g;
    if (!lat_geometry(levels, g, (uint32_t)LAT_MAX_SLOTS)) return NSR_ERR_UNSUPPORTED;
    uint32_t total = 0;
    for (int l = 0; l < 16; l++) {
        a.lv[l] = levels[l];
        a.lv[l].pad_ = (uint32_t)g.S[l] | ((uint32_t)g.shift[l] << 4) | ((uint32_t)g.base[l] << 8);
        total = g.base[l] + (uint32_t)g.S[l] * g.S[l] * g.S[l];
    }
    a.lat_slots = (total + 63u) & ~63u;
    a.xyzs = xyzs; a.perm = perm; a.m_dev = m_dev; a.M = M; a.gin = (const float4 *)gin; a.grad_tables = grad_tables;
    for (int i = 0; i < 3; i++) { a.bmin[i] = bmin[i]; a.bsize[i] = bsize[i]; }
    a.td = td; a.tc = tc;
    const size_t lds = 16 * sizeof(NsrLevel) + (TS_THREADS / 64) * ts_wave_bytes(a.lat_slots);
    if (lds > 65536) return NSR_ERR_UNSUPPORTED;
    // 16 workgroups per CU (4 096 in all), although only 3-4 are resident at a time: the cost of a run of tiles depends on
    // how often its samples change block, and with one workgroup per resident slot the slowest run decides the launch
    // (bench frame, backward pair: 4 per CU 25.5 ms, 6 -> 24.2, 8 -> 23.9, 16 -> 23.55, 32 -> 23.6)
    uint32_t nblocks = 256u * 16u;
    const uint32_t ntiles = (M + 15) / 16;
    if (nblocks > (ntiles + 3) / 4) nblocks = (ntiles + 3) / 4;
    if (nblocks == 0) nblocks = 1;
    return nsr_launch_lds<k_table_scatter>(65536, dim3(nblocks), dim3(TS_THREADS), lds, s, a);
}
