// Style image clustering: Lloyd k-means over pixel rows in (r, g, b, wxy x / m, wxy y / m) (include/nsr.h, "Style image
// clustering"; nerfstyle_amd/segment.py).  The per-row arithmetic is km_core.h, shared with the host.
//   nsr_kmeans_step   one fused Lloyd step: assign every row, write its label, count the changed labels, sum per cluster the row
//                     count and the features in 2^-32 fixed point, sum the inertia; a second launch adds the blocks' partials and
//                     writes counts, sums, the new centroids and (changed, inertia)
//   nsr_kmeans_init   deterministic maximin over at most 65536 candidate rows, one block looping over the K centres
//
// Sums.  The per-cluster sums are int64, so the order of additions does not matter and any mix of paths gives the same bits.  A
// wave slot (one row per lane) goes in two stages.  Label maps are piecewise constant, so most slots hold one or two labels, and
// 64 lanes adding to one LDS address would serialise: the label of the lowest remaining lane is summed over the wave with a
// butterfly and added by lanes 0..5 (count and five sums), twice at the most.  What is left after two rounds is a slot with many
// labels, whose lanes then sit on different addresses: they add their own six values with LDS u64 atomics.  The block's table is
// flushed as one partial per block.  The inertia is fp64 and goes through fixed_sum.h: thread, wave, block, then the partials in
// the second launch, all in a fixed order.
#include "color_common.h"
#include "km_core.h"

#define KM_ENTRY (KM_FEATS + 1)                     // count, five sums
#define KM_ROWS_PER_BLOCK (CM_BLOCK * CM_UNITS_PER_THREAD)
#define KM_BALLOT_ROUNDS 2
#define KM_TAB (NSR_COLOR_MAX_REGIONS * KM_ENTRY + 1)   // and the block's count of changed labels
#define KM_NO_PREV (-2)                             // no previous label: differs from every label, -1 included

// the grid depends on the row count alone, for either stride
static inline uint32_t km_blocks(uint64_t n) {
    uint64_t b = (n + KM_ROWS_PER_BLOCK - 1) / KM_ROWS_PER_BLOCK;
    if (b > CM_MAX_BLOCKS) b = CM_MAX_BLOCKS;
    return b == 0 ? 1u : (uint32_t)b;
}

// One slot of a wave: lane l holds the fixed-point feature q of a row of cluster k when `on`.  Every lane of the wave calls it.
__device__ __forceinline__ void km_wave_add(unsigned long long *tab, bool on, uint32_t k, const int64_t (&q)[KM_FEATS]) {
    const int lane = threadIdx.x & 63;
    uint64_t left = __ballot(on);
    for (int round = 0; round < KM_BALLOT_ROUNDS && left; round++) {     // wave-uniform
        const uint32_t kk = __shfl(k, __ffsll((unsigned long long)left) - 1, 64);
        const bool mine = on && k == kk;
        const uint64_t m = __ballot(mine);
        long long s[KM_FEATS];
#pragma unroll
        for (int j = 0; j < KM_FEATS; j++) s[j] = mine ? (long long)q[j] : 0ll;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int j = 0; j < KM_FEATS; j++) s[j] += __shfl_xor(s[j], off, 64);
        }
        long long v = (long long)__popcll(m);                            // lane 0: the count; lane j + 1: sum j
#pragma unroll
        for (int j = 0; j < KM_FEATS; j++)
            if (lane == j + 1) v = s[j];
        if (lane < KM_ENTRY) atomicAdd(&tab[kk * KM_ENTRY + lane], (unsigned long long)v);
        left &= ~m;
    }
    if ((left >> lane) & 1ull) {                                         // many labels in the slot: one address a lane, mostly
        atomicAdd(&tab[k * KM_ENTRY], 1ull);
#pragma unroll
        for (int j = 0; j < KM_FEATS; j++) atomicAdd(&tab[k * KM_ENTRY + 1 + j], (unsigned long long)q[j]);
    }
}

// row i of the slot -> its label (-1: unlabelled or no row); every lane of the wave calls it
__device__ __forceinline__ int32_t km_slot(const KmGeom &G, const double *cent, uint32_t K, unsigned long long *tab, bool active,
                                           uint32_t i, float r, float g, float b, double &inertia) {
#pragma clang fp contract(off)
    int32_t label = -1;
    int64_t q[KM_FEATS] = {0, 0, 0, 0, 0};
    const bool on = active && km_valid(r, g, b);
    if (on) {
        double f[KM_FEATS], d;
        km_feature(G, i, r, g, b, f);
        label = (int32_t)km_assign(f, cent, K, d);
        inertia = inertia + d;
#pragma unroll
        for (int j = 0; j < KM_FEATS; j++) q[j] = km_quant(f[j]);
    }
    km_wave_add(tab, on, (uint32_t)label, q);
    return label;
}

// partials: per block KM_ENTRY * K + 1 u64 (the table, then the changed count); pinertia: one double per block.
// prev may be NULL (every row counts as changed) and may be `labels` itself: a row's label is read and written by one thread.
template <int STRIDE>
__global__ void __launch_bounds__(CM_BLOCK)
k_kmeans_step(const float *__restrict__ rows, uint32_t n, KmGeom G, const double *__restrict__ centroids, uint32_t K,
              const int32_t *prev, int32_t *labels, uint32_t head, uint32_t ngroups, unsigned long long *__restrict__ partials,
              double *__restrict__ pinertia) {
    __shared__ double cent[NSR_COLOR_MAX_REGIONS * KM_FEATS];
    __shared__ unsigned long long tab[KM_TAB];
    __shared__ double red[CM_WAVES];
    const uint32_t entries = K * KM_ENTRY + 1;
    for (uint32_t e = threadIdx.x; e < K * KM_FEATS; e += CM_BLOCK) cent[e] = centroids[e];
    for (uint32_t e = threadIdx.x; e < entries; e += CM_BLOCK) tab[e] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t T = gridDim.x * CM_BLOCK;                             // <= 2^19, and n <= 2^27: u32 throughout
    const uint32_t wave0 = blockIdx.x * CM_BLOCK + (threadIdx.x & ~63u); // the wave's first unit: wave-uniform trips
    double inertia = 0.0;
    uint32_t changed = 0;
    if (STRIDE == 4) {
        // four rows a trip, T apart (every access of a wave is 1 KiB contiguous), loaded before they are assigned one after the other
        const float4 *q = reinterpret_cast<const float4 *>(rows);
        for (uint32_t i0 = wave0; i0 < n; i0 += 4 * T) {
            const uint32_t i = i0 + lane;
            float4 v[4];
            int32_t pl[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                pl[k] = KM_NO_PREV;
                if (i + k * T < n) {
                    v[k] = q[i + k * T];
                    if (prev) pl[k] = prev[i + k * T];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool active = i + k * T < n;
                const int32_t l = km_slot(G, cent, K, tab, active, i + k * T, v[k].x, v[k].y, v[k].z, inertia);
                if (active) {
                    labels[i + k * T] = l;
                    changed += l != pl[k];
                }
            }
        }
    } else {
        // rows [head, head + 4 * ngroups) as groups of four rows = three float4 (the host makes their first byte 16-byte aligned),
        // the other n - 4 * ngroups rows (head and tail) one float at a time: a trip is one group and one such row per lane
        const uint32_t nscalar = n - 4 * ngroups;
        const uint32_t trips = ngroups > nscalar ? ngroups : nscalar;
        const float4 *q = reinterpret_cast<const float4 *>(rows + (size_t)head * 3);
        int32_t *lg = labels + head;
        const int32_t *pg = prev ? prev + head : nullptr;
        const bool lvec = ((uintptr_t)lg & 15u) == 0, pvec = ((uintptr_t)pg & 15u) == 0;
        for (uint32_t g0 = wave0; g0 < trips; g0 += T) {
            const uint32_t g = g0 + lane;
            const bool ga = g < ngroups, sa = g < nscalar;
            const uint32_t srow = g < head ? g : g + 4 * ngroups;
            float c[12], sc[3] = {0.0f, 0.0f, 0.0f};
            int32_t p4[4] = {KM_NO_PREV, KM_NO_PREV, KM_NO_PREV, KM_NO_PREV}, sp = KM_NO_PREV;
#pragma unroll
            for (int j = 0; j < 12; j++) c[j] = 0.0f;
            if (ga) {
                const float4 v0 = q[(size_t)g * 3], v1 = q[(size_t)g * 3 + 1], v2 = q[(size_t)g * 3 + 2];
                c[0] = v0.x; c[1] = v0.y; c[2] = v0.z; c[3] = v0.w; c[4] = v1.x; c[5] = v1.y;
                c[6] = v1.z; c[7] = v1.w; c[8] = v2.x; c[9] = v2.y; c[10] = v2.z; c[11] = v2.w;
                if (pg) {
                    if (pvec) {
                        const int4 v = *reinterpret_cast<const int4 *>(pg + (size_t)g * 4);
                        p4[0] = v.x; p4[1] = v.y; p4[2] = v.z; p4[3] = v.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; j++) p4[j] = pg[(size_t)g * 4 + j];
                    }
                }
            }
            if (sa) {
                sc[0] = rows[(size_t)srow * 3]; sc[1] = rows[(size_t)srow * 3 + 1]; sc[2] = rows[(size_t)srow * 3 + 2];
                if (prev) sp = prev[srow];
            }
            int32_t l4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                l4[j] = km_slot(G, cent, K, tab, ga, head + 4 * g + j, c[j * 3], c[j * 3 + 1], c[j * 3 + 2], inertia);
                if (ga) changed += l4[j] != p4[j];
            }
            if (ga) {
                if (lvec) *reinterpret_cast<int4 *>(lg + (size_t)g * 4) = make_int4(l4[0], l4[1], l4[2], l4[3]);
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) lg[(size_t)g * 4 + j] = l4[j];
                }
            }
            const int32_t ls = km_slot(G, cent, K, tab, sa, srow, sc[0], sc[1], sc[2], inertia);
            if (sa) {
                labels[srow] = ls;
                changed += ls != sp;
            }
        }
    }
    changed = nsr_wave_sum(changed);
    if (lane == 0) atomicAdd(&tab[K * KM_ENTRY], (unsigned long long)changed);
    nsr_block_sum_stage(inertia, red);                                   // its barrier also closes the table
    for (uint32_t e = threadIdx.x; e < entries; e += CM_BLOCK) partials[(size_t)blockIdx.x * entries + e] = tab[e];
    if (threadIdx.x == 0) pinertia[blockIdx.x] = nsr_block_sum_col<CM_WAVES>(red);
}

// Block k < K: thread t adds cluster k's entries of the partials of blocks t, t + 256, ..., then the block sum; thread 0 writes
// counts[k], sums[k] and the new centroid.  Block K: the changed count and the inertia, the latter in that fixed order.
__global__ void __launch_bounds__(CM_BLOCK)
k_kmeans_final(const unsigned long long *__restrict__ partials, const double *__restrict__ pinertia, uint32_t nblocks, uint32_t K,
               const double *centroids, int64_t *__restrict__ counts, int64_t *__restrict__ sums, double *centroids_out,
               double *__restrict__ stats) {
    __shared__ long long red[KM_ENTRY][CM_WAVES];
    __shared__ double dred[CM_WAVES];
    const uint32_t entries = K * KM_ENTRY + 1, k = blockIdx.x;
    if (k == K) {
        long long ch = 0;
        double in = 0.0;
        for (uint32_t b = threadIdx.x; b < nblocks; b += CM_BLOCK) {
            ch += (long long)partials[(size_t)b * entries + K * KM_ENTRY];
            in += pinertia[b];
        }
        nsr_block_sum_stage(ch, red[0]);
        nsr_block_sum_stage(in, dred);
        if (threadIdx.x == 0) {
            stats[0] = (double)nsr_block_sum_col<CM_WAVES>(red[0]);
            stats[1] = nsr_block_sum_col<CM_WAVES>(dred);
        }
        return;
    }
    long long a[KM_ENTRY];
#pragma unroll
    for (int c = 0; c < KM_ENTRY; c++) a[c] = 0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += CM_BLOCK) {
#pragma unroll
        for (int c = 0; c < KM_ENTRY; c++) a[c] += (long long)partials[(size_t)b * entries + k * KM_ENTRY + c];
    }
    nsr_block_sum_stage(a, red);
    if (threadIdx.x == 0) {
        const long long cnt = nsr_block_sum_col<CM_WAVES>(red[0]);
        counts[k] = cnt;
#pragma unroll
        for (int j = 0; j < KM_FEATS; j++) {
            const long long s = nsr_block_sum_col<CM_WAVES>(red[j + 1]);
            sums[k * KM_FEATS + j] = s;
            if (centroids_out) centroids_out[k * KM_FEATS + j] = cnt > 0 ? (double)s / KM_FIXED_ONE / (double)cnt : centroids[k * KM_FEATS + j];
        }
    }
}

// ---- maximin init -------------------------------------------------------------------------------------------------------------
#define KM_INIT_BLOCK 1024
#define KM_INIT_WAVES (KM_INIT_BLOCK / 64)
#define KM_MAX_CANDIDATES 65536u
#define KM_NONE 0xffffffffu

// (d1, i1) before (d2, i2): the smaller d when `least`, else the larger; among equal d the lower index
__device__ __forceinline__ bool km_before(bool least, double d1, uint32_t i1, double d2, uint32_t i2) {
    return (least ? d1 < d2 : d1 > d2) || (d1 == d2 && i1 < i2);
}

// One block.  Candidate c is row c * step.  Round 0 takes the labelled candidate nearest to `mean`; round r the candidate with the
// largest distance md[c] to its nearest chosen centre.  md (global, one double a candidate) is read and written by the thread
// that owns the candidate (c % 1024) only: -1 marks an unlabelled or chosen candidate.
__global__ void __launch_bounds__(KM_INIT_BLOCK)
k_kmeans_init(const float *__restrict__ rows, uint32_t stride, KmGeom G, uint32_t step, uint32_t ncand, const double *__restrict__ mean,
              uint32_t K, double *__restrict__ centroids, int32_t *__restrict__ chosen, uint32_t *__restrict__ n_labelled,
              double *__restrict__ md) {
    __shared__ double cur[KM_FEATS];
    __shared__ double wd[KM_INIT_WAVES];
    __shared__ uint32_t wi[KM_INIT_WAVES];
    __shared__ uint32_t labelled;
    if (threadIdx.x < KM_FEATS) cur[threadIdx.x] = mean[threadIdx.x];
    if (threadIdx.x == 0) labelled = 0;
    __syncthreads();
    for (uint32_t r = 0; r < K; r++) {
        const bool least = r == 0;
        double bd = least ? INFINITY : -1.0;
        uint32_t bi = KM_NONE, mine = 0;
        for (uint32_t c = threadIdx.x; c < ncand; c += KM_INIT_BLOCK) {
            double m = least ? INFINITY : md[c];
            if (m < 0.0) continue;
            const float *p = rows + (size_t)c * step * stride;
            const float cr = p[0], cg = p[1], cb = p[2];
            if (least && !km_valid(cr, cg, cb)) { md[c] = -1.0; continue; }
            double f[KM_FEATS];
            km_feature(G, c * step, cr, cg, cb, f);
            const double d = km_dist(f, cur);
            if (!least && d < m) m = d;
            md[c] = m;
            mine++;
            const double key = least ? d : m;
            if (km_before(least, key, c, bd, bi)) { bd = key; bi = c; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(bd, off, 64);
            const uint32_t oi = __shfl_xor(bi, off, 64);
            if (km_before(least, od, oi, bd, bi)) { bd = od; bi = oi; }
        }
        if ((threadIdx.x & 63) == 0) { wd[threadIdx.x >> 6] = bd; wi[threadIdx.x >> 6] = bi; }
        if (least && mine) atomicAdd(&labelled, mine);
        __syncthreads();                                                 // everyone has read cur
        bd = wd[0]; bi = wi[0];
#pragma unroll
        for (int w = 1; w < KM_INIT_WAVES; w++)
            if (km_before(least, wd[w], wi[w], bd, bi)) { bd = wd[w]; bi = wi[w]; }
        if (bi != KM_NONE && (bi % KM_INIT_BLOCK) == threadIdx.x) {
            const float *p = rows + (size_t)bi * step * stride;
            double f[KM_FEATS];
            km_feature(G, bi * step, p[0], p[1], p[2], f);
#pragma unroll
            for (int j = 0; j < KM_FEATS; j++) { cur[j] = f[j]; centroids[r * KM_FEATS + j] = f[j]; }
            chosen[r] = (int32_t)(bi * step);
            md[bi] = -1.0;
        }
        if (bi == KM_NONE && threadIdx.x == 0) {                         // no candidate left: the centre before it once more
#pragma unroll
            for (int j = 0; j < KM_FEATS; j++) centroids[r * KM_FEATS + j] = cur[j];
            chosen[r] = -1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_labelled = labelled;
}

static inline bool km_bad_shape(uint64_t n, uint32_t stride, uint32_t H, uint32_t W, double wxy, uint32_t K) {
    if (n == 0 || n > KM_MAX_ROWS || (stride != 3 && stride != 4) || K == 0 || K > NSR_COLOR_MAX_REGIONS) return true;
    if (H == 0 || W == 0 || (uint64_t)H * W > n || n % ((uint64_t)H * W) != 0) return true;
    return !(wxy >= 0.0 && wxy <= 8.0);                                  // NaN is refused
}

extern "C" {

uint64_t nsr_kmeans_step_workspace_bytes(uint64_t n, uint32_t K) {
    if (n == 0 || n > KM_MAX_ROWS || K == 0 || K > NSR_COLOR_MAX_REGIONS) return 0;
    return (uint64_t)km_blocks(n) * ((uint64_t)K * KM_ENTRY + 2) * 8;
}

int nsr_kmeans_step(const float *rows, uint64_t n, uint32_t stride, uint32_t H, uint32_t W, double xy_weight, const double *centroids,
                    uint32_t K, const int32_t *prev_labels, int32_t *labels, int64_t *counts, int64_t *sums, double *centroids_out,
                    double *stats, void *workspace, nsr_stream_t stream) {
    NSR_CHECK_PTR(rows); NSR_CHECK_PTR(centroids); NSR_CHECK_PTR(labels); NSR_CHECK_PTR(counts); NSR_CHECK_PTR(sums);
    NSR_CHECK_PTR(stats); NSR_CHECK_PTR(workspace);
    if (km_bad_shape(n, stride, H, W, xy_weight, K)) return NSR_ERR_INVALID_ARG;
    const uintptr_t a = (uintptr_t)rows;
    if ((a & 3u) || ((uintptr_t)prev_labels & 3u) || ((uintptr_t)labels & 3u)) return NSR_ERR_INVALID_ARG;
    if (((uintptr_t)centroids & 7u) || ((uintptr_t)counts & 7u) || ((uintptr_t)sums & 7u) || ((uintptr_t)centroids_out & 7u) ||
        ((uintptr_t)stats & 7u) || ((uintptr_t)workspace & 7u))
        return NSR_ERR_INVALID_ARG;
    if (stride == 4 && (a & 15u)) return NSR_ERR_INVALID_ARG;
    const uint32_t nblocks = km_blocks(n);
    const hipStream_t s = (hipStream_t)stream;
    unsigned long long *partials = (unsigned long long *)workspace;
    double *pinertia = (double *)(partials + (size_t)nblocks * (K * KM_ENTRY + 1));
    const KmGeom G = km_geom(H, W, xy_weight);
    const dim3 grid(nblocks), block(CM_BLOCK);
    if (stride == 4) {
        hipLaunchKernelGGL(k_kmeans_step<4>, grid, block, 0, s, rows, (uint32_t)n, G, centroids, K, prev_labels, labels, 0u, 0u,
                           partials, pinertia);
    } else {
        // rows are 12 B: `head` rows bring a base at 4 * head bytes past a 16-byte boundary onto the next one
        uint32_t head = (uint32_t)((a >> 2) & 3u);
        if (head > n) head = (uint32_t)n;
        const uint32_t ngroups = ((uint32_t)n - head) / 4;
        hipLaunchKernelGGL(k_kmeans_step<3>, grid, block, 0, s, rows, (uint32_t)n, G, centroids, K, prev_labels, labels, head, ngroups,
                           partials, pinertia);
    }
    hipLaunchKernelGGL(k_kmeans_final, dim3(K + 1), block, 0, s, (const unsigned long long *)partials, (const double *)pinertia, nblocks,
                       K, centroids, counts, sums, centroids_out, stats);
    return nsr_launch_status();
}

uint64_t nsr_kmeans_init_workspace_bytes(uint64_t n) {
    if (n == 0 || n > KM_MAX_ROWS) return 0;
    const uint64_t step = (n + KM_MAX_CANDIDATES - 1) / KM_MAX_CANDIDATES;
    return (n + step - 1) / step * sizeof(double);
}

int nsr_kmeans_init(const float *rows, uint64_t n, uint32_t stride, uint32_t H, uint32_t W, double xy_weight, const double *mean,
                    uint32_t K, double *centroids, int32_t *chosen_rows, uint32_t *n_labelled, void *workspace, nsr_stream_t stream) {
    NSR_CHECK_PTR(rows); NSR_CHECK_PTR(mean); NSR_CHECK_PTR(centroids); NSR_CHECK_PTR(chosen_rows); NSR_CHECK_PTR(n_labelled);
    NSR_CHECK_PTR(workspace);
    if (km_bad_shape(n, stride, H, W, xy_weight, K)) return NSR_ERR_INVALID_ARG;
    if (((uintptr_t)rows & 3u) || ((uintptr_t)chosen_rows & 3u) || ((uintptr_t)n_labelled & 3u) || ((uintptr_t)mean & 7u) ||
        ((uintptr_t)centroids & 7u) || ((uintptr_t)workspace & 7u))
        return NSR_ERR_INVALID_ARG;
    const uint32_t step = (uint32_t)((n + KM_MAX_CANDIDATES - 1) / KM_MAX_CANDIDATES);
    const uint32_t ncand = (uint32_t)((n + step - 1) / step);
    hipLaunchKernelGGL(k_kmeans_init, dim3(1), dim3(KM_INIT_BLOCK), 0, (hipStream_t)stream, rows, stride, km_geom(H, W, xy_weight), step,
                       ncand, mean, K, centroids, chosen_rows, n_labelled, (double *)workspace);
    return nsr_launch_status();
}

}   // extern "C"
