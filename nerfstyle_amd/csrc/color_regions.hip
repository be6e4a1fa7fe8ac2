// Region-wise colour transfer: the two passes of color_match.hip with one set of moments and one transform per region.
//   nsr_color_region_moments   count, sum x and sum x x^T per region in fp64, in an order fixed by (n, stride, K, the labels)
//   nsr_color_region_apply     x -> A_k x + b_k with k the row's region, the f32 fma chain of nsr_color_apply
// A row's region is an explicit i32 label or, for stride-4 rows, the row's fourth float (the class id of a ResidentDataset
// target row); every row outside 0..K-1 falls into slot K.  The per-region eigen-solves are host code (color_match.py).
//
// Moments.  K x 10 fp64 accumulators do not fit in a thread's registers, and an LDS or global fp64 atomic would make the order
// of additions depend on timing.  So a wave sums one region at a time: per slot (one row per lane) it takes the region of its
// lowest remaining lane, the lanes of that region contribute their nine values and all others +0.0 to the fixed_sum.h butterfly,
// and lanes 0..9 add the count and the nine sums to the wave's own [K+1][10] fp64 table in LDS.  Label maps are piecewise
// constant, so a slot is one or two such rounds; a map with 64 regions in a wave takes 64 rounds and is still exact.  The
// tables are flushed as per-block partials and summed by a second launch, as in color_match.hip.
#include "color_common.h"

#define CR_ENTRY 10                                 // count, r, g, b, rr, rg, rb, gg, gb, bb
#define CR_SLOTS (NSR_COLOR_MAX_REGIONS + 1)        // regions 0..K-1 and slot K

__device__ __forceinline__ uint32_t cr_region(int32_t label, uint32_t K) { return (uint32_t)label < K ? (uint32_t)label : K; }

// the fourth float as a label: w == (float)k exactly for an integer 0 <= k < K (-0.0 == 0.0f: region 0), anything else -> K
__device__ __forceinline__ uint32_t cr_region(float w, uint32_t K) {
    const bool in = w >= 0.0f && w < (float)K;      // false for NaN
    const uint32_t k = in ? (uint32_t)w : 0u;
    return in && (float)k == w ? k : K;
}

// ---- moments -------------------------------------------------------------------------------------------------------------------
// One slot of a wave: lane l holds the row (rf, gf, bf) of region `reg` when `active`.  Every lane of the wave calls it.
__device__ __forceinline__ void cr_wave_add(double *tab, bool active, uint32_t reg, float rf, float gf, float bf) {
    const int lane = threadIdx.x & 63;
    uint64_t left = __ballot(active);
    while (left) {                                                       // wave-uniform
        const uint32_t k = __shfl(reg, __ffsll((unsigned long long)left) - 1, 64);
        const bool mine = active && reg == k;
        const uint64_t m = __ballot(mine);
        CmAcc a;
#pragma unroll
        for (int c = 0; c < 9; c++) a.s[c] = 0.0;
        cm_add(a, mine ? rf : 0.0f, mine ? gf : 0.0f, mine ? bf : 0.0f);   // the others: +0.0 in all nine
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int c = 0; c < 9; c++) a.s[c] += __shfl_xor(a.s[c], off, 64);
        }
        double v = (double)__popcll(m);                                  // lane 0: the count, exact; lane c + 1: sum c
#pragma unroll
        for (int c = 0; c < 9; c++)
            if (lane == c + 1) v = a.s[c];
        if (lane < CR_ENTRY) tab[k * CR_ENTRY + lane] += v;              // this wave's table: its LDS accesses stay in order
        left &= ~m;
    }
}

template <int STRIDE, bool FLOAT_LABELS>
__global__ void __launch_bounds__(CM_BLOCK)
k_color_region_moments(const float *__restrict__ rows, uint64_t n, const int32_t *__restrict__ labels, uint32_t K,
                       double *__restrict__ partials) {
    __shared__ double tab[CM_WAVES][CR_SLOTS * CR_ENTRY];
    const uint32_t entries = (K + 1) * CR_ENTRY;
    for (uint32_t e = threadIdx.x; e < entries; e += CM_BLOCK) {
#pragma unroll
        for (int w = 0; w < CM_WAVES; w++) tab[w][e] = 0.0;
    }
    __syncthreads();
    double *mytab = tab[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t T = (uint64_t)gridDim.x * CM_BLOCK;
    const uint64_t wave0 = (uint64_t)blockIdx.x * CM_BLOCK + (threadIdx.x & ~63u);      // the wave's first unit: wave-uniform trips
    if (STRIDE == 4) {
        // four rows a trip, T apart, loaded before they are added one slot after the other
        const float4 *q = reinterpret_cast<const float4 *>(rows);
        for (uint64_t i0 = wave0; i0 < n; i0 += 4 * T) {
            const uint64_t i = i0 + lane;
            float4 v[4];
            int32_t l[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                l[k] = 0;
                if (i + k * T < n) {
                    v[k] = q[i + k * T];
                    if (!FLOAT_LABELS) l[k] = labels[i + k * T];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t reg = FLOAT_LABELS ? cr_region(v[k].w, K) : cr_region(l[k], K);
                cr_wave_add(mytab, i + k * T < n, reg, v[k].x, v[k].y, v[k].z);
            }
        }
    } else {
        const uint64_t groups = (n + 3) / 4, full = n / 4;
        const bool vec = ((uintptr_t)rows & 15u) == 0;                   // a full group is 48 B of rows, 16 B of labels
        const bool lvec = ((uintptr_t)labels & 15u) == 0;
        for (uint64_t g0 = wave0; g0 < groups; g0 += T) {
            const uint64_t g = g0 + lane;
            float c[12];
            int32_t l[4] = {0, 0, 0, 0};
            uint32_t m = 0;
#pragma unroll
            for (int j = 0; j < 12; j++) c[j] = 0.0f;
            if (g < groups) {
                const float *p = rows + g * 12;
                const int32_t *pl = labels + g * 4;
                m = g < full ? 4u : (uint32_t)(n - g * 4);
                if (g < full && vec) {
                    const float4 *q = reinterpret_cast<const float4 *>(p);
                    const float4 v0 = q[0], v1 = q[1], v2 = q[2];
                    c[0] = v0.x; c[1] = v0.y; c[2] = v0.z; c[3] = v0.w; c[4] = v1.x; c[5] = v1.y;
                    c[6] = v1.z; c[7] = v1.w; c[8] = v2.x; c[9] = v2.y; c[10] = v2.z; c[11] = v2.w;
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++)
                        if (j < m) { c[j * 3] = p[j * 3]; c[j * 3 + 1] = p[j * 3 + 1]; c[j * 3 + 2] = p[j * 3 + 2]; }
                }
                if (g < full && lvec) {
                    const int4 v = *reinterpret_cast<const int4 *>(pl);
                    l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++)
                        if (j < m) l[j] = pl[j];
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) cr_wave_add(mytab, j < m, cr_region(l[j], K), c[j * 3], c[j * 3 + 1], c[j * 3 + 2]);
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < entries; e += CM_BLOCK) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < CM_WAVES; w++) s += tab[w][e];
        partials[(uint64_t)blockIdx.x * entries + e] = s;
    }
}

// block k: thread t adds region k's entry of the partials of blocks t, t + 256, ... in that order, then the block sum
__global__ void __launch_bounds__(CM_BLOCK)
k_color_region_moments_final(const double *__restrict__ partials, uint32_t nblocks, uint32_t K, double *__restrict__ moments) {
    __shared__ double red[CR_ENTRY][CM_WAVES];
    const uint32_t entries = (K + 1) * CR_ENTRY, k = blockIdx.x;
    double a[CR_ENTRY];
#pragma unroll
    for (int c = 0; c < CR_ENTRY; c++) a[c] = 0.0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += CM_BLOCK) {
#pragma unroll
        for (int c = 0; c < CR_ENTRY; c++) a[c] += partials[(uint64_t)b * entries + k * CR_ENTRY + c];
    }
    nsr_block_sum_stage(a, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < CR_ENTRY; c++) moments[k * CR_ENTRY + c] = nsr_block_sum_col<CM_WAVES>(red[c]);
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------
// The K + 1 transforms (rows 0..2 of each) sit in LDS, 48 B a region: a lane reads its row's with three 16-byte LDS loads.
__device__ __forceinline__ void cr_stage_tfs(float4 (*lds)[3], const float *__restrict__ tfs, uint32_t K) {
    float *f = reinterpret_cast<float *>(lds);                           // tfs is 4-byte aligned only: one float at a time
    for (uint32_t e = threadIdx.x; e < (K + 1) * 12; e += CM_BLOCK) f[e] = tfs[(e / 12) * 16 + e % 12];
    __syncthreads();
}

__device__ __forceinline__ void cr_map(const float4 (*lds)[3], uint32_t reg, int clamp, float &r, float &g, float &b) {
    CmTf t;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float4 v = lds[reg][c];
        t.m[c][0] = v.x; t.m[c][1] = v.y; t.m[c][2] = v.z; t.m[c][3] = v.w;
    }
    cm_map(t, clamp, r, g, b);
}

// stride 4: as k_color_apply4.  A row is read and written by the same thread, so dst == src is safe.
template <bool FLOAT_LABELS>
__global__ void __launch_bounds__(CM_BLOCK)
k_color_region_apply4(const float *src, float *dst, uint64_t n, const int32_t *__restrict__ labels, uint32_t K,
                      const float *__restrict__ tfs, int clamp) {
    __shared__ float4 lds[CR_SLOTS][3];
    cr_stage_tfs(lds, tfs, K);
    const float4 *s = reinterpret_cast<const float4 *>(src);
    float4 *d = reinterpret_cast<float4 *>(dst);
    const uint64_t T = (uint64_t)gridDim.x * CM_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * CM_BLOCK + threadIdx.x; i < n; i += 4 * T) {
        float4 v[4];
        int32_t l[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k * T < n) {
                v[k] = s[i + k * T];
                if (!FLOAT_LABELS) l[k] = labels[i + k * T];
            }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k * T < n) {
                const uint32_t reg = FLOAT_LABELS ? cr_region(v[k].w, K) : cr_region(l[k], K);
                cr_map(lds, reg, clamp, v[k].x, v[k].y, v[k].z);         // .w is carried as loaded
                d[i + k * T] = v[k];
            }
    }
}

// stride 3: as k_color_apply3 (rows [head, head + 4 * ngroups) as three float4 per four rows, the rest one float at a time)
__global__ void __launch_bounds__(CM_BLOCK)
k_color_region_apply3(const float *src, float *dst, uint64_t n, uint32_t head, uint64_t ngroups, const int32_t *__restrict__ labels,
                      uint32_t K, const float *__restrict__ tfs, int clamp) {
    __shared__ float4 lds[CR_SLOTS][3];
    cr_stage_tfs(lds, tfs, K);
    const uint64_t T = (uint64_t)gridDim.x * CM_BLOCK;
    const uint64_t tid = (uint64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    const float4 *s = reinterpret_cast<const float4 *>(src + (uint64_t)head * 3);
    float4 *d = reinterpret_cast<float4 *>(dst + (uint64_t)head * 3);
    const int32_t *lg = labels + head;
    const bool lvec = ((uintptr_t)lg & 15u) == 0;
    for (uint64_t g = tid; g < ngroups; g += T) {
        float4 v0 = s[g * 3], v1 = s[g * 3 + 1], v2 = s[g * 3 + 2];
        int4 l;
        if (lvec) l = *reinterpret_cast<const int4 *>(lg + g * 4);
        else l = make_int4(lg[g * 4], lg[g * 4 + 1], lg[g * 4 + 2], lg[g * 4 + 3]);
        cr_map(lds, cr_region(l.x, K), clamp, v0.x, v0.y, v0.z);
        cr_map(lds, cr_region(l.y, K), clamp, v0.w, v1.x, v1.y);
        cr_map(lds, cr_region(l.z, K), clamp, v1.z, v1.w, v2.x);
        cr_map(lds, cr_region(l.w, K), clamp, v2.y, v2.z, v2.w);
        d[g * 3] = v0; d[g * 3 + 1] = v1; d[g * 3 + 2] = v2;
    }
    const uint64_t nscalar = n - 4 * ngroups;
    for (uint64_t j = tid; j < nscalar; j += T) {
        const uint64_t row = j < head ? j : j + 4 * ngroups;
        float r = src[row * 3], g = src[row * 3 + 1], b = src[row * 3 + 2];
        cr_map(lds, cr_region(labels[row], K), clamp, r, g, b);
        dst[row * 3] = r; dst[row * 3 + 1] = g; dst[row * 3 + 2] = b;
    }
}

static inline bool cr_bad_k(uint32_t K) { return K == 0 || K > NSR_COLOR_MAX_REGIONS; }

extern "C" {

// enough for either stride: the stride-4 grid (one unit a row) is never the smaller one
uint64_t nsr_color_region_moments_workspace_bytes(uint64_t n, uint32_t K) {
    if (cr_bad_k(K)) return 0;
    return (uint64_t)cm_moment_blocks(n) * (K + 1) * CR_ENTRY * sizeof(double);
}

int nsr_color_region_moments(const float *rows, uint64_t n, uint32_t stride, const int32_t *labels, uint32_t K, double *moments,
                             void *workspace, nsr_stream_t stream) {
    NSR_CHECK_PTR(rows); NSR_CHECK_PTR(moments); NSR_CHECK_PTR(workspace);
    if (n == 0 || (stride != 3 && stride != 4) || cr_bad_k(K)) return NSR_ERR_INVALID_ARG;
    if (labels == nullptr && stride == 3) return NSR_ERR_INVALID_ARG;
    if (((uintptr_t)rows & 3u) || ((uintptr_t)labels & 3u) || ((uintptr_t)moments & 7u) || ((uintptr_t)workspace & 7u))
        return NSR_ERR_INVALID_ARG;
    if (stride == 4 && ((uintptr_t)rows & 15u)) return NSR_ERR_INVALID_ARG;
    const uint32_t nblocks = cm_moment_blocks(cm_moment_units(n, stride));
    const hipStream_t s = (hipStream_t)stream;
    double *partials = (double *)workspace;
    const dim3 grid(nblocks), block(CM_BLOCK);
    if (stride == 3) hipLaunchKernelGGL((k_color_region_moments<3, false>), grid, block, 0, s, rows, n, labels, K, partials);
    else if (labels) hipLaunchKernelGGL((k_color_region_moments<4, false>), grid, block, 0, s, rows, n, labels, K, partials);
    else hipLaunchKernelGGL((k_color_region_moments<4, true>), grid, block, 0, s, rows, n, labels, K, partials);
    hipLaunchKernelGGL(k_color_region_moments_final, dim3(K + 1), block, 0, s, (const double *)partials, nblocks, K, moments);
    return nsr_launch_status();
}

int nsr_color_region_apply(const float *src, float *dst, uint64_t n, uint32_t stride, const int32_t *labels, uint32_t K,
                           const float *tfs, int clamp, nsr_stream_t stream) {
    NSR_CHECK_PTR(src); NSR_CHECK_PTR(dst); NSR_CHECK_PTR(tfs);
    if (n == 0 || (stride != 3 && stride != 4) || cr_bad_k(K)) return NSR_ERR_INVALID_ARG;
    if (labels == nullptr && stride == 3) return NSR_ERR_INVALID_ARG;
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if ((a & 3u) || (b & 3u) || ((uintptr_t)labels & 3u) || ((uintptr_t)tfs & 3u)) return NSR_ERR_INVALID_ARG;
    if (n > (UINT64_MAX >> 8) / stride) return NSR_ERR_INVALID_ARG;
    const uint64_t bytes = n * stride * sizeof(float);
    if (a != b && a < b + bytes && b < a + bytes) return NSR_ERR_INVALID_ARG;       // in place or disjoint, nothing between
    const hipStream_t s = (hipStream_t)stream;
    if (stride == 4) {
        if ((a & 15u) || (b & 15u)) return NSR_ERR_INVALID_ARG;
        const dim3 grid(nsr_grid_1d((n + 3) / 4, CM_BLOCK)), block(CM_BLOCK);
        if (labels) hipLaunchKernelGGL(k_color_region_apply4<false>, grid, block, 0, s, src, dst, n, labels, K, tfs, clamp);
        else hipLaunchKernelGGL(k_color_region_apply4<true>, grid, block, 0, s, src, dst, n, labels, K, tfs, clamp);
    } else {
        // head and groups as in nsr_color_apply: the float4 path needs src and dst at the same offset from a 16-byte boundary
        uint32_t head = 0;
        uint64_t ngroups = 0;
        if ((a & 15u) == (b & 15u)) {
            head = (uint32_t)((a >> 2) & 3u);
            if (head > n) head = (uint32_t)n;
            ngroups = (n - head) / 4;
        }
        const uint64_t nscalar = n - 4 * ngroups;
        hipLaunchKernelGGL(k_color_region_apply3, dim3(nsr_grid_1d(ngroups > nscalar ? ngroups : nscalar, CM_BLOCK)), dim3(CM_BLOCK), 0, s,
                           src, dst, n, head, ngroups, labels, K, tfs, clamp);
    }
    return nsr_launch_status();
}

}   // extern "C"
