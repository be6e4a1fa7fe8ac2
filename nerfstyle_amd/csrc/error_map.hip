// Error-map importance sampling of training rays (instant-ngp's error map), drawn on the device.  Per frame a coarse grid of
// cell x cell pixel cells holds the running squared error of the rays drawn there; pixels are drawn in proportion to it and every
// ray carries the weight (uniform pdf) / (pdf of its draw), so the weighted mean loss still estimates the uniform mean.
//     k_errmap_accumulate           per-ray errors into the cells' integer accumulators (a wave sums the rays that share a cell first)
//     k_errmap_fold_prefix          a workgroup per frame: accumulators into err, quantise, inclusive u64 prefix of the masses
//     k_errmap_frame_prefix         one workgroup: inclusive prefix of the frames' totals
//     k_draw_frame_batch_error      k_draw_frame_batch with the pixel (and optionally the frame) drawn from those prefixes
// Everything that decides a draw is integer arithmetic: sums of integers do not depend on the order the atomics arrive in, so
// two runs, two ranks and a NumPy restatement (tests/error_map_ref.py) reach the same bits.  Floats appear in the running
// error, its quantisation and the returned weight, each with contraction off and the operation order of include/nsr.h.
#include "fixed_sum.h"
#include "philox.h"

#define EM_BLOCK 256
#define EM_WAVES (EM_BLOCK / 64)
// fixed point of the accumulators: 2^20 per unit of squared error, one ray clamped to 4 (2^22), so a wave's 64 rays sum below
// 2^28 in 32 bits and a cell holds 2^42 rays' worth in 64
#define EM_ACC_SCALE 1048576.0f
#define EM_ACC_CLAMP 4194304.0f
// a cell's quantised error is at most 2^18: with 16 x 16 cells a mass stays below 2^26, a 1008 x 756 frame's total below 2^38
#define EM_Q_CLAMP 262144.0f
// the Philox domain word of the cell draw (0, 1: occupancy.hip; 2, 3: the frame and the pixel of frame_batch.hip)
#define EM_PHILOX_CELL 4u

struct EmGrid {
    uint32_t F, w, h, cell, gw, gh, G, P;
};

static inline EmGrid em_grid(uint32_t F, uint32_t w, uint32_t h, uint32_t cell) {
    EmGrid g;
    g.F = F; g.w = w; g.h = h; g.cell = cell;
    g.gw = nsr_div_up(w, cell); g.gh = nsr_div_up(h, cell);
    g.G = g.gw * g.gh; g.P = w * h;
    return g;
}

// F, w, h, cell >= 1, P and F * G inside 31 bits (cell keys and pixel ids are 32-bit)
static inline bool em_grid_ok(uint32_t F, uint32_t w, uint32_t h, uint32_t cell) {
    if (F == 0 || w == 0 || h == 0 || cell == 0 || F > 0x7fffffffu) return false;
    if ((uint64_t)w * h > 0x7fffffffull) return false;
    const uint64_t G = (uint64_t)nsr_div_up(w, cell) * nsr_div_up(h, cell);
    return (uint64_t)F * G <= 0x7fffffffull;
}

// real extent of the ragged edge cells
__device__ __forceinline__ uint32_t em_extent(uint32_t c, uint32_t cell, uint32_t size) { return min(cell, size - c * cell); }

// ---------------------------------------------------------------------------------------------
// accumulate
// ---------------------------------------------------------------------------------------------
// Thread per ray.  A full frame walked in 8 x 8 tiles puts all 64 lanes of a wave into one cell, and exact-duplicate addresses
// in one wave-instruction each cost their own request at the memory side: so the wave adds up first.  EM_ROUNDS rounds: the
// first lane still waiting names its cell, a ballot finds the lanes that share it, a masked xor tree sums the group (32-bit:
// 64 x 2^22 < 2^28) and the naming lane adds sum and count.  A tile inside a cell is done after one round, a tile across a
// cell corner after four; lanes still waiting then (a scattered batch: 64 cells in a wave) add their own values.  Integer sums:
// exact in any grouping.
#define EM_ROUNDS 4
__global__ void __launch_bounds__(EM_BLOCK)
k_errmap_accumulate(EmGrid g, const int32_t *__restrict__ seg_frame, const int32_t *__restrict__ pix, const float *__restrict__ ray_err,
                    uint32_t K, uint32_t N, unsigned long long *__restrict__ acc_sum, uint32_t *__restrict__ acc_cnt) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u;
    // whole waves walk together (the ballots below want every lane of the wave in the loop)
    const uint64_t n_round = ((uint64_t)N + 63u) & ~63ull;
    for (uint64_t n = blockIdx.x * EM_BLOCK + threadIdx.x; n < n_round; n += gridDim.x * EM_BLOCK) {
        uint32_t key = 0xffffffffu, a = 0u;
        if (n < N) {
            const uint32_t f = (uint32_t)seg_frame[n / K], p = (uint32_t)pix[n];
            const float e = ray_err[n];
            if (f < g.F && p < g.P && e >= 0.0f) {                      // NaN fails the comparison
                const uint32_t y = p / g.w, x = p - y * g.w;
                key = f * g.G + (y / g.cell) * g.gw + x / g.cell;
                a = (uint32_t)fminf(floorf(e * EM_ACC_SCALE), EM_ACC_CLAMP);
            }
        }
        uint64_t waiting = __ballot(key != 0xffffffffu);
        for (int round = 0; round < EM_ROUNDS && waiting; round++) {
            const uint32_t first = (uint32_t)__ffsll((long long)waiting) - 1u;
            const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)first);
            const uint64_t group = __ballot(key == k);
            waiting &= ~group;
            const uint32_t count = (uint32_t)__popcll(group);
            uint32_t sum = key == k ? a : 0u;
            if (count > 1u) sum = nsr_wave_sum(sum);                    // wave-uniform
            if (lane == first) {
                atomicAdd(acc_sum + k, (unsigned long long)sum);
                atomicAdd(acc_cnt + k, count);
            }
        }
        if ((waiting >> lane) & 1ull) {                                 // scattered rays: their own adds
            atomicAdd(acc_sum + key, (unsigned long long)a);
            atomicAdd(acc_cnt + key, 1u);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fold, quantise, prefix
// ---------------------------------------------------------------------------------------------
// Inclusive scan of one value per thread over the block, on top of `carry` (every thread's copy of what came before the
// chunk): shuffle scan inside the wave, the waves' totals through LDS.  Returns the thread's inclusive value and moves carry
// past the chunk.  Integer adds: exact.
__device__ __forceinline__ uint64_t em_block_scan(uint64_t v, uint64_t &carry) {
    __shared__ uint64_t wave_total[EM_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    v = nsr_wave_scan(v);
    __syncthreads();                                   // the previous chunk's totals have been read
    if (lane == 63u) wave_total[wave] = v;
    __syncthreads();
    uint64_t before = carry, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < EM_WAVES; k++) {
        const uint64_t t = wave_total[k];
        if (k < wave) before += t;
        all += t;
    }
    carry += all;
    return before + v;
}

__global__ void __launch_bounds__(EM_BLOCK)
k_errmap_fold_prefix(EmGrid g, float decay, float quant_scale, float *__restrict__ err, unsigned long long *__restrict__ acc_sum,
                     uint32_t *__restrict__ acc_cnt, unsigned long long *__restrict__ prefix) {
#pragma clang fp contract(off)
    const size_t row = (size_t)blockIdx.x * g.G;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < g.G; base += EM_BLOCK) {
        const uint32_t c = base + threadIdx.x;
        uint64_t mass = 0;
        if (c < g.G) {
            float e = err[row + c];
            const uint32_t cnt = acc_cnt[row + c];
            if (cnt != 0u) {
                const float mean = (float)((double)acc_sum[row + c] / (double)cnt * (1.0 / 1048576.0));
                const float d = mean - e;
                const float m = decay * d;
                e = e + m;
                err[row + c] = e;
                acc_sum[row + c] = 0ull;
                acc_cnt[row + c] = 0u;
            }
            const float t = e * quant_scale;
            const uint32_t q = t >= 0.0f ? (uint32_t)fminf(floorf(t), EM_Q_CLAMP) : 0u;        // NaN and negative: 0
            const uint32_t gy = c / g.gw, gx = c - gy * g.gw;
            mass = (uint64_t)(em_extent(gx, g.cell, g.w) * em_extent(gy, g.cell, g.h)) * q;
        }
        const uint64_t incl = em_block_scan(mass, carry);
        if (c < g.G) prefix[row + c] = incl;
    }
}

// the frames' totals are the last entries of their prefix rows
__global__ void __launch_bounds__(EM_BLOCK)
k_errmap_frame_prefix(EmGrid g, const unsigned long long *__restrict__ prefix, unsigned long long *__restrict__ frame_prefix) {
    uint64_t carry = 0;
    for (uint32_t base = 0; base < g.F; base += EM_BLOCK) {
        const uint32_t f = base + threadIdx.x;
        const uint64_t total = f < g.F ? prefix[(size_t)f * g.G + (g.G - 1u)] : 0ull;
        const uint64_t incl = em_block_scan(total, carry);
        if (f < g.F) frame_prefix[f] = incl;
    }
}

// ---------------------------------------------------------------------------------------------
// the draw
// ---------------------------------------------------------------------------------------------
// first index in [0, n) whose inclusive prefix exceeds target; target < prefix[n - 1], so there is one
__device__ __forceinline__ uint32_t em_upper_bound(const unsigned long long *__restrict__ prefix, uint32_t n, uint64_t target) {
    uint32_t lo = 0, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] > target) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

__device__ __forceinline__ uint64_t em_u64(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }

// 1 / (u + (1 - u) * (a * b) / c) in that order, the integers converted once
__device__ __forceinline__ float em_weight(float u, float a, float b, float c) {
#pragma clang fp contract(off)
    const float ab = a * b;
    const float m = (1.0f - u) * ab;
    const float r = m / c;
    const float d = u + r;
    return 1.0f / d;
}

struct EmDraw {
    EmGrid g;
    const unsigned long long *prefix, *frame_prefix;
    float uniform_mix;
    uint64_t thresh;                       // round(uniform_mix * 2^32): a 32-bit word below it takes the uniform branch
    int frames_by_error;
    uint32_t K, N, seed_lo, seed_hi, sequence;
    const uint32_t *sequence_dev;
    uint32_t stream_id;
    const int32_t *fixed_frames;
    int32_t *seg_frame, *pix;
    int64_t *rows;
    float *weights;
};

// Thread per ray; like k_draw_frame_batch every ray draws its segment's frame again and the segment's first ray stores it.
__global__ void __launch_bounds__(EM_BLOCK)
k_draw_frame_batch_error(EmDraw a) {
    const EmGrid g = a.g;
    const uint32_t seq = a.sequence + (a.sequence_dev ? a.sequence_dev[0] : 0u);
    const uint64_t grand = a.frame_prefix[g.F - 1u];
    for (uint32_t n = blockIdx.x * EM_BLOCK + threadIdx.x; n < a.N; n += gridDim.x * EM_BLOCK) {
        const uint32_t s = n / a.K;
        int32_t f;
        float wf = 1.0f;
        if (a.fixed_frames) {
            f = a.fixed_frames[s];
        } else {
            const OccU4 r = occ_philox(s, seq, 2u, a.stream_id, a.seed_lo, a.seed_hi);
            f = (int32_t)__umulhi(r.x, g.F);
            if (a.frames_by_error && grand != 0ull) {
                if ((uint64_t)r.y >= a.thresh) f = (int32_t)em_upper_bound(a.frame_prefix, g.F, __umul64hi(em_u64(r.z, r.w), grand));
                const uint64_t total_f = a.frame_prefix[f] - (f ? a.frame_prefix[f - 1] : 0ull);
                wf = em_weight(a.uniform_mix, (float)g.F, (float)total_f, (float)grand);
            }
        }
        // a fixed frame outside [0, F) stays in seg_frame (its rays become NaN): uniform pixels of weight 1, rows of frame 0
        const bool valid = (uint32_t)f < g.F;
        const uint32_t fr = valid ? (uint32_t)f : 0u;
        const unsigned long long *row = a.prefix + (size_t)fr * g.G;
        const uint64_t total = valid ? row[g.G - 1u] : 0ull;
        const OccU4 r = occ_philox(n, seq, 3u, a.stream_id, a.seed_lo, a.seed_hi);
        uint32_t p = __umulhi(r.x, g.P), c = 0u;
        float wp = 1.0f;
        if (total != 0ull) {
            if ((uint64_t)r.y >= a.thresh) {
                const OccU4 q = occ_philox(n, seq, EM_PHILOX_CELL, a.stream_id, a.seed_lo, a.seed_hi);
                c = em_upper_bound(row, g.G, __umul64hi(em_u64(q.x, q.y), total));
                const uint32_t gy = c / g.gw, gx = c - gy * g.gw;
                const uint32_t x = gx * g.cell + __umulhi(q.z, em_extent(gx, g.cell, g.w));
                const uint32_t y = gy * g.cell + __umulhi(q.w, em_extent(gy, g.cell, g.h));
                p = y * g.w + x;
            } else {
                const uint32_t y = p / g.w, x = p - y * g.w;
                c = (y / g.cell) * g.gw + x / g.cell;
            }
            // the weight is that of the mixture, whichever branch drew the pixel: q_c = mass / pixels of the cell, exactly
            const uint32_t gy = c / g.gw, gx = c - gy * g.gw;
            const uint64_t mass = row[c] - (c ? row[c - 1u] : 0ull);
            const uint32_t npix = em_extent(gx, g.cell, g.w) * em_extent(gy, g.cell, g.h);
            const uint32_t qc = (mass >> 32) ? (uint32_t)(mass / npix) : (uint32_t)mass / npix;
            wp = em_weight(a.uniform_mix, (float)qc, (float)g.P, (float)total);
        }
        if (n - s * a.K == 0u) a.seg_frame[s] = f;
        a.pix[n] = (int32_t)p;
        a.rows[n] = (int64_t)((uint64_t)fr * g.P + p);
        a.weights[n] = wp * wf;
    }
}

// after the draw, on the same stream (frame_batch.hip's k_advance_sequence)
__global__ void k_errmap_advance_sequence(uint32_t *__restrict__ sequence_dev) { sequence_dev[0] += 1u; }

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int nsr_error_map_accumulate(uint32_t F, uint32_t w, uint32_t h, uint32_t cell, const int32_t *seg_frame, const int32_t *pix,
                             const float *ray_err, uint32_t S, uint32_t K, uint64_t *acc_sum, uint32_t *acc_cnt, nsr_stream_t stream) {
    if (!em_grid_ok(F, w, h, cell)) return NSR_ERR_INVALID_ARG;
    const uint64_t N = (uint64_t)S * K;
    if (N > 0xffffffffull) return NSR_ERR_INVALID_ARG;
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(seg_frame); NSR_CHECK_PTR(pix); NSR_CHECK_PTR(ray_err); NSR_CHECK_PTR(acc_sum); NSR_CHECK_PTR(acc_cnt);
    if (((uintptr_t)acc_sum & 7u) != 0) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_errmap_accumulate, dim3(nsr_grid_1d(N, EM_BLOCK)), dim3(EM_BLOCK), 0, (hipStream_t)stream, em_grid(F, w, h, cell),
                       seg_frame, pix, ray_err, K, (uint32_t)N, (unsigned long long *)acc_sum, acc_cnt);
    return nsr_launch_status();
}

int nsr_error_map_rebuild(uint32_t F, uint32_t w, uint32_t h, uint32_t cell, float decay, float quant_scale, float *err,
                          uint64_t *acc_sum, uint32_t *acc_cnt, uint64_t *prefix, uint64_t *frame_prefix, nsr_stream_t stream) {
    if (!em_grid_ok(F, w, h, cell)) return NSR_ERR_INVALID_ARG;
    NSR_CHECK_PTR(err); NSR_CHECK_PTR(acc_sum); NSR_CHECK_PTR(acc_cnt); NSR_CHECK_PTR(prefix); NSR_CHECK_PTR(frame_prefix);
    if ((((uintptr_t)acc_sum | (uintptr_t)prefix | (uintptr_t)frame_prefix) & 7u) != 0) return NSR_ERR_INVALID_ARG;
    if (!(decay >= 0.0f && decay <= 1.0f) || !(quant_scale > 0.0f)) return NSR_ERR_INVALID_ARG;
    const EmGrid g = em_grid(F, w, h, cell);
    hipLaunchKernelGGL(k_errmap_fold_prefix, dim3(F), dim3(EM_BLOCK), 0, (hipStream_t)stream, g, decay, quant_scale, err,
                       (unsigned long long *)acc_sum, acc_cnt, (unsigned long long *)prefix);
    hipLaunchKernelGGL(k_errmap_frame_prefix, dim3(1), dim3(EM_BLOCK), 0, (hipStream_t)stream, g, (const unsigned long long *)prefix,
                       (unsigned long long *)frame_prefix);
    return nsr_launch_status();
}

int nsr_draw_frame_batch_error(uint32_t F, uint32_t w, uint32_t h, uint32_t cell, const uint64_t *prefix, const uint64_t *frame_prefix,
                               float uniform_mix, int frames_by_error, uint32_t S, uint32_t K, uint64_t seed, uint32_t sequence,
                               uint32_t *sequence_dev, uint32_t stream_id, const int32_t *fixed_frames, int advance, int32_t *seg_frame,
                               int32_t *pix, int64_t *rows, float *weights, nsr_stream_t stream) {
    if (advance && sequence_dev == nullptr) return NSR_ERR_INVALID_ARG;
    const uint64_t N = (uint64_t)S * K;
    if (N > 0xffffffffull) return NSR_ERR_INVALID_ARG;
    if (N == 0 && !advance) return NSR_OK;
    if (N != 0) {
        NSR_CHECK_PTR(prefix); NSR_CHECK_PTR(frame_prefix);
        NSR_CHECK_PTR(seg_frame); NSR_CHECK_PTR(pix); NSR_CHECK_PTR(rows); NSR_CHECK_PTR(weights);
        if (!em_grid_ok(F, w, h, cell) || !(uniform_mix >= 0.0f && uniform_mix <= 1.0f)) return NSR_ERR_INVALID_ARG;
        if ((((uintptr_t)prefix | (uintptr_t)frame_prefix) & 7u) != 0) return NSR_ERR_INVALID_ARG;
        EmDraw a;
        a.g = em_grid(F, w, h, cell);
        a.prefix = (const unsigned long long *)prefix; a.frame_prefix = (const unsigned long long *)frame_prefix;
        a.uniform_mix = uniform_mix;
        a.thresh = (uint64_t)llrint((double)uniform_mix * 4294967296.0);
        a.frames_by_error = frames_by_error;
        a.K = K; a.N = (uint32_t)N; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.sequence = sequence;
        a.sequence_dev = sequence_dev; a.stream_id = stream_id; a.fixed_frames = fixed_frames;
        a.seg_frame = seg_frame; a.pix = pix; a.rows = rows; a.weights = weights;
        hipLaunchKernelGGL(k_draw_frame_batch_error, dim3(nsr_grid_1d(N, EM_BLOCK)), dim3(EM_BLOCK), 0, (hipStream_t)stream, a);
    }
    if (advance) hipLaunchKernelGGL(k_errmap_advance_sequence, dim3(1), dim3(1), 0, (hipStream_t)stream, sequence_dev);
    return nsr_launch_status();
}

}   // extern "C"
