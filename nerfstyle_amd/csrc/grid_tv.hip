// Total-variation regulariser on the hash-grid tables (torch-ngp's GridEncoder.grad_total_variation): the gradient of a
// squared-difference smoothness term between neighbouring lattice vertices, added straight into the table gradient after the
// backward and before the optimiser step, and optionally the term's value.  include/nsr.h ("Total variation") states the
// definition; tests/tv_ref.py restates it in NumPy.
//
// One thread per (level, draw): blockIdx.y is the level, the draws of a level are grid-strided over blockIdx.x.  A draw is one
// lattice vertex a -- vertex i of the level when the level is swept (x fastest, so a wave reads and adds to adjacent rows where
// the level is dense), a Philox draw otherwise -- and costs seven row reads from the fp32 masters (the vertex and its up to six
// neighbours; a row is one access of up to 16 bytes) and one fp32 atomic per lane with a non-zero weight, all to the vertex's
// own row.  No LDS but the value's block sum, no host read, nothing allocated: capture-safe.
//
// Rounding of one draw's add (what the tests' bound counts): the differences (one rounding each), their sum as
// ((x- + x+) + (y- + y+)) + (z- + z+) (each difference passes through at most three adds), c * scale, and the product.
#include "fixed_sum.h"
#include "philox.h"

#define TV_BLOCK 256
#define TV_WAVES (TV_BLOCK / 64)
#define TV_MAX_LANES 8

struct TvArgs {
    uint32_t n[NSR_MAX_LEVELS];                    // draws of the level; 0 = the level is masked off
    uint32_t sweep[NSR_MAX_LEVELS];                // the draws enumerate the vertices
    float c[NSR_MAX_LEVELS][TV_MAX_LANES];         // (float)(2 lambda_k / n_l)
    uint32_t seed_lo, seed_hi, sequence, stream_id;
    float scale_host;
};

template <int RF> struct TvRow { float v[RF]; };

template <int RF>
__device__ __forceinline__ TvRow<RF> tv_load(const float *__restrict__ tab, uint32_t row) {
    TvRow<RF> r;
    const float *p = tab + (size_t)row * RF;
    if (RF == 1) {
        r.v[0] = p[0];
    } else if (RF == 2) {
        const float2 q = *reinterpret_cast<const float2 *>(p);
        r.v[0] = q.x; r.v[1] = q.y;
    } else {
#pragma unroll
        for (int j = 0; j < RF / 4; j++) {
            const float4 q = reinterpret_cast<const float4 *>(p)[j];
            r.v[j * 4 + 0] = q.x; r.v[j * 4 + 1] = q.y; r.v[j * 4 + 2] = q.z; r.v[j * 4 + 3] = q.w;
        }
    }
    return r;
}

// partials: [level][blockIdx.x][RF] f64 when VALUE; grad may be NULL when VALUE (value only)
template <int RF, bool VALUE>
__global__ void __launch_bounds__(TV_BLOCK)
k_grid_tv(const float *__restrict__ tables, float *__restrict__ grad, NsrLevels levels, TvArgs a,
          const uint32_t *__restrict__ sequence_dev, const float *__restrict__ scale_dev, double *__restrict__ partials) {
    __shared__ double red[RF][TV_WAVES];
    const uint32_t level = blockIdx.y;
    const uint32_t n = a.n[level];
    if (n == 0u) return;                                               // the whole block: nobody waits at the barrier below
    const NsrLevel lv = levels.lv[level];
    const uint32_t res = lv.resolution, side = res + 1u;
    const bool sweep = a.sweep[level] != 0u;
    const uint32_t seq = a.sequence + (sequence_dev ? sequence_dev[0] : 0u);
    const float scale = a.scale_host * (scale_dev ? scale_dev[0] : 1.0f);
    float cs[RF];
    bool lane_on[RF];                                                  // lambda_k != 0: other lanes are neither summed nor written
#pragma unroll
    for (int k = 0; k < RF; k++) { cs[k] = a.c[level][k] * scale; lane_on[k] = a.c[level][k] != 0.0f; }
    const float *tab = tables + (size_t)lv.offset * RF;
    double acc[RF];
#pragma unroll
    for (int k = 0; k < RF; k++) acc[k] = 0.0;

    for (uint32_t i = blockIdx.x * TV_BLOCK + threadIdx.x; i < n; i += gridDim.x * TV_BLOCK) {
        uint32_t p[3];
        if (sweep) {
            const uint32_t q = i / side;
            p[0] = i - q * side;
            p[2] = q / side;
            p[1] = q - p[2] * side;
        } else {
            const OccU4 r = occ_philox(i, seq, 5u, (a.stream_id << 8) | level, a.seed_lo, a.seed_hi);
            p[0] = __umulhi(r.x, side); p[1] = __umulhi(r.y, side); p[2] = __umulhi(r.z, side);
        }
        const uint32_t row = nsr_grid_row(lv, p[0], p[1], p[2], 0u);
        const TvRow<RF> t = tv_load<RF>(tab, row);
        float pair[3][RF];                                             // (t - t[a - e_d]) + (t - t[a + e_d]) of the axis
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const bool has_lo = p[d] > 0u, has_hi = p[d] < res;
            uint32_t qlo[3] = {p[0], p[1], p[2]}, qhi[3] = {p[0], p[1], p[2]};
            if (has_lo) qlo[d] -= 1u;                                  // without the neighbour: the vertex itself, difference 0
            if (has_hi) qhi[d] += 1u;
            const TvRow<RF> lo = tv_load<RF>(tab, nsr_grid_row(lv, qlo[0], qlo[1], qlo[2], 0u));
            const TvRow<RF> hi = tv_load<RF>(tab, nsr_grid_row(lv, qhi[0], qhi[1], qhi[2], 0u));
#pragma unroll
            for (int k = 0; k < RF; k++) {
                const float dlo = has_lo ? t.v[k] - lo.v[k] : 0.0f;
                const float dhi = has_hi ? t.v[k] - hi.v[k] : 0.0f;
                pair[d][k] = dlo + dhi;
                if (VALUE && has_hi && lane_on[k]) {
                    const double e = (double)t.v[k] - (double)hi.v[k];
                    acc[k] += e * e;
                }
            }
        }
        if (grad) {
            float *g = grad + ((size_t)lv.offset + row) * RF;
#pragma unroll
            for (int k = 0; k < RF; k++)
                if (lane_on[k]) atomicAdd(g + k, cs[k] * ((pair[0][k] + pair[1][k]) + pair[2][k]));
        }
    }
    if (VALUE) {
        nsr_block_sum_stage(acc, red);
        if (threadIdx.x == 0) {
            double *out = partials + ((size_t)level * gridDim.x + blockIdx.x) * RF;
#pragma unroll
            for (int k = 0; k < RF; k++) out[k] = nsr_block_sum_col<TV_WAVES>(red[k]);
        }
    }
}

// one block per level: thread t adds the partials of blocks t, t + 256, ... in that order, then the block sum
template <int RF>
__global__ void __launch_bounds__(TV_BLOCK)
k_grid_tv_final(const double *__restrict__ partials, uint32_t nblocks, TvArgs a, double *__restrict__ value) {
    __shared__ double red[RF][TV_WAVES];
    const uint32_t level = blockIdx.x;
    const uint32_t n = a.n[level];
    double acc[RF];
#pragma unroll
    for (int k = 0; k < RF; k++) acc[k] = 0.0;
    if (n != 0u) {                                                     // block-uniform; a masked level wrote no partials
        for (uint32_t b = threadIdx.x; b < nblocks; b += TV_BLOCK) {
#pragma unroll
            for (int k = 0; k < RF; k++) acc[k] += partials[((size_t)level * nblocks + b) * RF + k];
        }
    }
    nsr_block_sum_stage(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < RF; k++) value[(size_t)level * RF + k] = n != 0u ? nsr_block_sum_col<TV_WAVES>(red[k]) / (double)n : 0.0;
    }
}

template <int RF>
static void tv_launch(const float *tables, float *grad, const NsrLevels &lv, const TvArgs &a, uint32_t L, uint32_t gx,
                      const uint32_t *sequence_dev, const float *scale_dev, double *value, double *partials, hipStream_t s) {
    if (value) {
        hipLaunchKernelGGL((k_grid_tv<RF, true>), dim3(gx, L), dim3(TV_BLOCK), 0, s, tables, grad, lv, a, sequence_dev, scale_dev, partials);
        hipLaunchKernelGGL((k_grid_tv_final<RF>), dim3(L), dim3(TV_BLOCK), 0, s, (const double *)partials, gx, a, value);
    } else {
        hipLaunchKernelGGL((k_grid_tv<RF, false>), dim3(gx, L), dim3(TV_BLOCK), 0, s, tables, grad, lv, a, sequence_dev, scale_dev, partials);
    }
}

// after the draws, on the same stream: never the drawing kernel, which reads the word (as frame_batch.hip's)
__global__ void k_tv_advance_sequence(uint32_t *__restrict__ sequence_dev) { sequence_dev[0] += 1u; }

extern "C" {

uint64_t nsr_grid_tv_workspace_bytes(uint32_t L, uint32_t n_samples, uint32_t row_floats) {
    const uint64_t bytes = (uint64_t)nsr_grid_1d(n_samples, TV_BLOCK) * L * row_floats * sizeof(double);
    return bytes ? bytes : sizeof(double);
}

int nsr_grid_tv(const float *tables, float *grad_tables, uint32_t row_floats, const float *lambda, const int32_t *offsets, uint32_t L,
                float S, uint32_t H, uint32_t gridtype, uint32_t level_mask, uint32_t n_samples, uint64_t seed, uint32_t sequence,
                uint32_t *sequence_dev, uint32_t stream_id, int advance, float scale_host, const float *scale_dev, double *value,
                void *workspace, nsr_stream_t stream) {
    NSR_CHECK_PTR(tables); NSR_CHECK_PTR(lambda); NSR_CHECK_PTR(offsets);
    if (row_floats != 1 && row_floats != 2 && row_floats != 4 && row_floats != 8) return NSR_ERR_INVALID_ARG;
    if (L == 0 || L > NSR_MAX_LEVELS || gridtype > 1 || n_samples == 0) return NSR_ERR_INVALID_ARG;
    if (advance && sequence_dev == nullptr) return NSR_ERR_INVALID_ARG;
    if (grad_tables == nullptr && value == nullptr) return NSR_ERR_INVALID_ARG;
    if (value != nullptr && workspace == nullptr) return NSR_ERR_INVALID_ARG;
    const uintptr_t row_align = (row_floats >= 4 ? 16u : row_floats * 4u) - 1u;
    if (((uintptr_t)tables & row_align) || ((uintptr_t)grad_tables & 3u) || ((uintptr_t)value & 7u) || ((uintptr_t)workspace & 7u))
        return NSR_ERR_INVALID_ARG;
    NsrLevels lv;
    nsr_fill_levels(&lv, offsets, L, S, H, gridtype);
    TvArgs a;
    uint32_t n_max = 0;
    for (uint32_t l = 0; l < L; l++) {
        const uint64_t side = (uint64_t)lv.lv[l].resolution + 1u;
        if (side > 0x7fffffffull || offsets[l] < 0 || offsets[l + 1] <= offsets[l]) return NSR_ERR_INVALID_ARG;
        // V = side^3 in 64 bits; a side past 2^21 has more vertices than any n_samples (and would overflow the product)
        const bool sweep = side <= (1u << 21) && (uint64_t)n_samples >= side * side * side;
        const uint32_t n = sweep ? (uint32_t)(side * side * side) : n_samples;
        const bool on = (level_mask >> l) & 1u;
        a.n[l] = on ? n : 0u;
        a.sweep[l] = sweep ? 1u : 0u;
        for (uint32_t k = 0; k < TV_MAX_LANES; k++)
            a.c[l][k] = k < row_floats ? (float)(2.0 * (double)lambda[k] / (double)n) : 0.0f;
        if (on && n > n_max) n_max = n;
    }
    for (uint32_t l = L; l < NSR_MAX_LEVELS; l++) {
        a.n[l] = 0u; a.sweep[l] = 0u;
        for (uint32_t k = 0; k < TV_MAX_LANES; k++) a.c[l][k] = 0.0f;
    }
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.sequence = sequence; a.stream_id = stream_id;
    a.scale_host = scale_host;
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t gx = nsr_grid_1d(n_max, TV_BLOCK);                  // <= nsr_grid_1d(n_samples): the workspace's block count
    double *partials = (double *)workspace;
    switch (row_floats) {
        case 1: tv_launch<1>(tables, grad_tables, lv, a, L, gx, sequence_dev, scale_dev, value, partials, s); break;
        case 2: tv_launch<2>(tables, grad_tables, lv, a, L, gx, sequence_dev, scale_dev, value, partials, s); break;
        case 4: tv_launch<4>(tables, grad_tables, lv, a, L, gx, sequence_dev, scale_dev, value, partials, s); break;
        default: tv_launch<8>(tables, grad_tables, lv, a, L, gx, sequence_dev, scale_dev, value, partials, s); break;
    }
    if (advance) hipLaunchKernelGGL(k_tv_advance_sequence, dim3(1), dim3(1), 0, s, sequence_dev);
    return nsr_launch_status();
}

}   // extern "C"
