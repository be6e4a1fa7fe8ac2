// Occupancy-grid floater cull: connected components of the occupied cells, their statistics, and the pass that closes the
// components the caller does not keep (nsr_occ_components / nsr_occ_component_stats / nsr_occ_cull; include/nsr.h, "Occupancy
// components", states the definition).  No workspace and no host read in any of them: all three may be captured.
//
// One thread owns one bitfield byte = 8 consecutive cells of one cascade = one 2x2x2 Morton block (k_ou_mark's shape), in the
// labelling's init and union kernels, in the statistics and in the cull.
//
// Labelling, a lock-free union-find over the cells (uf_core.h; the edges come from occ_cc_core.h, which the host test runs too):
//   k_oc_init      labels[u] = u at an occupied cell, -1 elsewhere, as two 16-byte stores a thread
//   k_oc_union     a thread reads its byte and the bytes of the next block along +x, +y, +z and unites every occupied cell with
//                  its occupied +x, +y, +z neighbours.  A hook puts the LARGER root under the SMALLER id and path halving only
//                  stores ancestors, so the final root of a component is its smallest cell id whatever the interleaving.  Every
//                  read of parent[] is uf_core.h's relaxed agent-scope atomic load or a compare-and-swap's return value: the
//                  kernel holds no plain load of parent[].  The bitfield is constant input and read plainly.
//   k_oc_flatten   a launch of its own (the kernel boundary is the visibility), a thread a cell: labels[u] = find(u).
// The 12 edges inside a block are united as they come, not pre-merged in registers.
// Statistics (integer adds, mins and maxes: order-free, so atomics are allowed): a thread gathers runs of equal roots over its 8
// cells in registers, a block gathers them in a table of roots in LDS, and a root receives a few global atomics a BLOCK: a
// block's 256 bytes are one 16 x 16 x 8 brick of cells, which a large component fills with one root.
// Cull: the thread that reads the byte masks and writes it; the grid's 8 words go through registers as integers, and only the
// bytes that lose a bit touch the grid at all.
#include "nsr_common.h"
#include "fixed_sum.h"
#include "occ_cc_core.h"

#define OC_BLOCK 256
#define OC_NONE 0xffffffffu              // labels[u] of an unoccupied cell: -1
#define OC_SLOTS 128u                    // roots a block gathers in LDS
#define OC_PROBES 4u

// ---- labelling ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OC_BLOCK)
k_oc_init(const uint8_t *__restrict__ bitfield, uint32_t N, uint32_t *__restrict__ parent) {
    for (uint32_t n = blockIdx.x * OC_BLOCK + threadIdx.x; n < N; n += gridDim.x * OC_BLOCK) {
        const uint32_t bits = bitfield[n], u = n * 8u;
        uint32_t p[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) p[j] = ((bits >> j) & 1u) ? u + j : OC_NONE;
        uint4 *p4 = reinterpret_cast<uint4 *>(parent) + (size_t)n * 2;
        p4[0] = make_uint4(p[0], p[1], p[2], p[3]);
        p4[1] = make_uint4(p[4], p[5], p[6], p[7]);
    }
}

__global__ void __launch_bounds__(OC_BLOCK)
k_oc_union(const uint8_t *__restrict__ bitfield, uint32_t H, uint32_t N, uint32_t *parent) {
    for (uint32_t n = blockIdx.x * OC_BLOCK + threadIdx.x; n < N; n += gridDim.x * OC_BLOCK)
        occ_cc_unite_block(parent, occ_cc_block(bitfield, H, n));
}

__global__ void __launch_bounds__(OC_BLOCK)
k_oc_flatten(uint32_t *parent, uint32_t cells) {
    for (uint32_t u = blockIdx.x * OC_BLOCK + threadIdx.x; u < cells; u += gridDim.x * OC_BLOCK)
        if (uf_load(parent + u) != OC_NONE) uf_min(parent + u, uf_find(parent, u));      // the root is an ancestor: only a decrease
}

// ---- statistics -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OC_BLOCK)
k_oc_stats_init(uint32_t cells, int32_t H, uint32_t *__restrict__ n_cells, int32_t *__restrict__ lo, int32_t *__restrict__ hi) {
    for (uint32_t u = blockIdx.x * OC_BLOCK + threadIdx.x; u < cells; u += gridDim.x * OC_BLOCK) {
        n_cells[u] = 0u;
#pragma unroll
        for (int a = 0; a < 3; a++) lo[(size_t)u * 3 + a] = H, hi[(size_t)u * 3 + a] = -1;
    }
}

struct OcTable {
    uint32_t key[OC_SLOTS], n[OC_SLOTS];
    int32_t mn[OC_SLOTS * 3], mx[OC_SLOTS * 3];
};

__device__ __forceinline__ void oc_send_global(uint32_t r, uint32_t c, const int32_t *mn, const int32_t *mx, uint32_t *n_cells,
                                               int32_t *lo, int32_t *hi) {
    atomicAdd(n_cells + r, c);
#pragma unroll
    for (int a = 0; a < 3; a++) atomicMin(lo + (size_t)r * 3 + a, mn[a]), atomicMax(hi + (size_t)r * 3 + a, mx[a]);
}

// into the block's table; a root that finds no slot in OC_PROBES tries goes to global memory directly (the table is full of
// other roots, so the components here are small and their addresses their own)
__device__ __forceinline__ void oc_send(OcTable &t, uint32_t r, uint32_t c, const int32_t *mn, const int32_t *mx, uint32_t *n_cells,
                                        int32_t *lo, int32_t *hi) {
    const uint32_t h = (r * 2654435761u) >> 25;                                        // 7 bits: OC_SLOTS
    for (uint32_t probe = 0; probe < OC_PROBES; probe++) {
        const uint32_t slot = (h + probe) & (OC_SLOTS - 1u);
        const uint32_t seen = atomicCAS(&t.key[slot], OC_NONE, r);
        if (seen != OC_NONE && seen != r) continue;
        atomicAdd(&t.n[slot], c);
#pragma unroll
        for (int a = 0; a < 3; a++) atomicMin(&t.mn[slot * 3 + a], mn[a]), atomicMax(&t.mx[slot * 3 + a], mx[a]);
        return;
    }
    oc_send_global(r, c, mn, mx, n_cells, lo, hi);
}

__global__ void __launch_bounds__(OC_BLOCK)
k_oc_stats(const int32_t *__restrict__ labels, uint32_t H, uint32_t N, uint32_t *n_cells, int32_t *lo, int32_t *hi) {
    __shared__ OcTable t;
    for (uint32_t i = threadIdx.x; i < OC_SLOTS; i += OC_BLOCK) {
        t.key[i] = OC_NONE, t.n[i] = 0u;
#pragma unroll
        for (int a = 0; a < 3; a++) t.mn[i * 3 + a] = (int32_t)H, t.mx[i * 3 + a] = -1;
    }
    __syncthreads();
    const uint32_t cells = N * 8u, bytes_per_cas = H * H * H / 8u;
    for (uint32_t n = blockIdx.x * OC_BLOCK + threadIdx.x; n < N; n += gridDim.x * OC_BLOCK) {
        const uint4 *l4 = reinterpret_cast<const uint4 *>(labels) + (size_t)n * 2;
        const uint4 a4 = l4[0], b4 = l4[1];
        const uint32_t r[8] = {a4.x, a4.y, a4.z, a4.w, b4.x, b4.y, b4.z, b4.w};
        const uint32_t m = n % bytes_per_cas;
        const int32_t at[3] = {(int32_t)(2u * occ_cc_compact(m)), (int32_t)(2u * occ_cc_compact(m >> 1)),
                               (int32_t)(2u * occ_cc_compact(m >> 2))};
        uint32_t root = OC_NONE, count = 0u;
        int32_t mn[3], mx[3];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            if (r[j] >= cells) continue;                    // -1, or a label that is not this grid's: nothing is written through it
            const int32_t x[3] = {at[0] + (int32_t)(j & 1u), at[1] + (int32_t)((j >> 1) & 1u), at[2] + (int32_t)(j >> 2)};
            if (r[j] == root) {
                count++;
#pragma unroll
                for (int a = 0; a < 3; a++) mn[a] = min(mn[a], x[a]), mx[a] = max(mx[a], x[a]);
            } else {
                if (count) oc_send(t, root, count, mn, mx, n_cells, lo, hi);
                root = r[j], count = 1u;
#pragma unroll
                for (int a = 0; a < 3; a++) mn[a] = mx[a] = x[a];
            }
        }
        if (count) oc_send(t, root, count, mn, mx, n_cells, lo, hi);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < OC_SLOTS; i += OC_BLOCK)
        if (t.key[i] != OC_NONE) oc_send_global(t.key[i], t.n[i], t.mn + i * 3, t.mx + i * 3, n_cells, lo, hi);
}

// ---- cull -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_oc_zero(uint32_t *__restrict__ n_culled, uint32_t C) {
    if (threadIdx.x < C) n_culled[threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(OC_BLOCK)
k_oc_cull(uint32_t *__restrict__ grid, uint8_t *__restrict__ bitfield, const int32_t *__restrict__ labels,
          const uint8_t *__restrict__ keep, uint32_t bytes_per_cas, uint32_t N, uint32_t C, uint32_t *n_culled) {
    __shared__ uint32_t culled[8];           // this block's culled cells per cascade
    if (threadIdx.x < 8) culled[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t cells = N * 8u;
    for (uint32_t base = blockIdx.x * OC_BLOCK; base < N; base += gridDim.x * OC_BLOCK) {
        const uint32_t n = base + threadIdx.x;
        // bytes_per_cas = H^3 / 8 is a multiple of 64 from H = 8 on: the 64 bytes of a wave lie in one cascade
        const uint32_t cas = (n < N ? n : base) / bytes_per_cas;
        uint32_t clear = 0u;
        const uint32_t bits = n < N ? bitfield[n] : 0u;
        if (bits) {
            const uint4 *l4 = reinterpret_cast<const uint4 *>(labels) + (size_t)n * 2;
            const uint4 a4 = l4[0], b4 = l4[1];
            const uint32_t r[8] = {a4.x, a4.y, a4.z, a4.w, b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (uint32_t j = 0; j < 8; j++)              // a label outside the grid decides nothing and is not dereferenced
                if (((bits >> j) & 1u) && r[j] < cells && keep[r[j]] == 0) clear |= 1u << j;
        }
        if (clear) {
            if (grid) {
                uint4 *g4 = reinterpret_cast<uint4 *>(grid) + (size_t)n * 2;
                const uint4 lo = g4[0], hi = g4[1];
                uint32_t g[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                for (uint32_t j = 0; j < 8; j++)
                    if ((clear >> j) & 1u) g[j] = 0xBF800000u;                       // -1.0f; the others keep their bits
                g4[0] = make_uint4(g[0], g[1], g[2], g[3]);
                g4[1] = make_uint4(g[4], g[5], g[6], g[7]);
            }
            bitfield[n] = (uint8_t)(bits & ~clear);
        }
        if (n_culled) {
            const uint32_t s = nsr_wave_sum((uint32_t)__popc(clear));
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&culled[cas], s);
        }
    }
    if (n_culled) {
        __syncthreads();
        if (threadIdx.x < C && culled[threadIdx.x]) atomicAdd(n_culled + threadIdx.x, culled[threadIdx.x]);
    }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
// the shape rule of every nsr_occ_* call (occupancy.hip, occ_dims_ok)
static bool oc_dims_ok(uint32_t C, uint32_t H) {
    return C >= 1 && C <= 8 && H >= 8 && H <= 512 && (H & (H - 1u)) == 0u && (uint64_t)C * H * H * H < (1ull << 31);
}
static inline bool oc_misaligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1u)) != 0; }

extern "C" {

int nsr_occ_components(const uint8_t *bitfield, uint32_t C, uint32_t H, int32_t *labels, nsr_stream_t stream) {
    NSR_CHECK_PTR(bitfield); NSR_CHECK_PTR(labels);
    if (!oc_dims_ok(C, H) || oc_misaligned(labels, 16)) return NSR_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t N = C * (H * H * H / 8u), cells = N * 8u;
    uint32_t *parent = reinterpret_cast<uint32_t *>(labels);
    hipLaunchKernelGGL(k_oc_init, dim3(nsr_grid_1d(N, OC_BLOCK)), dim3(OC_BLOCK), 0, s, bitfield, N, parent);
    hipLaunchKernelGGL(k_oc_union, dim3(nsr_grid_1d(N, OC_BLOCK)), dim3(OC_BLOCK), 0, s, bitfield, H, N, parent);
    hipLaunchKernelGGL(k_oc_flatten, dim3(nsr_grid_1d(cells, OC_BLOCK)), dim3(OC_BLOCK), 0, s, parent, cells);
    return nsr_launch_status();
}

int nsr_occ_component_stats(const int32_t *labels, uint32_t C, uint32_t H, uint32_t *n_cells, int32_t *lo, int32_t *hi,
                            nsr_stream_t stream) {
    NSR_CHECK_PTR(labels); NSR_CHECK_PTR(n_cells); NSR_CHECK_PTR(lo); NSR_CHECK_PTR(hi);
    if (!oc_dims_ok(C, H)) return NSR_ERR_INVALID_ARG;
    if (oc_misaligned(labels, 16) || oc_misaligned(n_cells, 4) || oc_misaligned(lo, 4) || oc_misaligned(hi, 4)) return NSR_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t N = C * (H * H * H / 8u), cells = N * 8u;
    hipLaunchKernelGGL(k_oc_stats_init, dim3(nsr_grid_1d(cells, OC_BLOCK)), dim3(OC_BLOCK), 0, s, cells, (int32_t)H, n_cells, lo, hi);
    hipLaunchKernelGGL(k_oc_stats, dim3(nsr_grid_1d(N, OC_BLOCK)), dim3(OC_BLOCK), 0, s, labels, H, N, n_cells, lo, hi);
    return nsr_launch_status();
}

int nsr_occ_cull(float *density_grid, uint8_t *bitfield, const int32_t *labels, const uint8_t *keep, uint32_t C, uint32_t H,
                 uint32_t *n_culled, nsr_stream_t stream) {
    NSR_CHECK_PTR(bitfield); NSR_CHECK_PTR(labels); NSR_CHECK_PTR(keep);
    if (!oc_dims_ok(C, H)) return NSR_ERR_INVALID_ARG;
    if (oc_misaligned(density_grid, 16) || oc_misaligned(labels, 16) || oc_misaligned(n_culled, 4)) return NSR_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t bytes_per_cas = H * H * H / 8u, N = C * bytes_per_cas;
    if (n_culled) hipLaunchKernelGGL(k_oc_zero, dim3(1), dim3(64), 0, s, n_culled, C);
    hipLaunchKernelGGL(k_oc_cull, dim3(nsr_grid_1d(N, OC_BLOCK)), dim3(OC_BLOCK), 0, s, reinterpret_cast<uint32_t *>(density_grid),
                       bitfield, labels, keep, bytes_per_cas, N, C, n_culled);
    return nsr_launch_status();
}

}   // extern "C"
