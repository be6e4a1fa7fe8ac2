// Mesh cleaning: connected components of an indexed triangle mesh, their statistics, and the filter that drops whole components
// (nsr_mesh_components / nsr_mesh_component_stats / nsr_mesh_filter_count / nsr_mesh_filter_emit; include/nsr.h, "Mesh
// cleaning", states the definition).
//
// Labelling is a lock-free union-find over the faces (uf_core.h, shared with the host stress test):
//   k_mc_init      parent[v] = v, the bad-face counter = 0
//   k_mc_union     a thread a face: unite(a, b), unite(b, c).  A hook always puts the LARGER root under the SMALLER id (one
//                  compare-and-swap) and path halving only stores ancestors (atomic min), so parents only decrease and the final
//                  root of a component is its minimum vertex id whatever the interleaving: that is why the labels are a pure
//                  function of the input although the kernel races.  Every read of parent[] that can feed a retry is a relaxed
//                  agent-scope atomic load or the compare-and-swap's own return value (the XCDs' L2s are not coherent inside a
//                  kernel: a plain load could stay stale and the loop never end).  No fences in the kernel.
//   k_mc_flatten   a launch of its own (the kernel boundary is the visibility): labels[v] = find(v), in place, so every label
//                  is the root.  A face index outside [0, V) is tested BEFORE it is used anywhere: such a face is counted and
//                  skipped, here and in every kernel below.
// Statistics, indexed by the root's vertex id (integer adds, mins and maxes: order-free, so atomics are allowed):
//   k_mc_stats_init, k_mc_stats_verts (n_verts, the box as order-preserving uint keys of the f32 coordinates),
//   k_mc_stats_faces (n_faces), k_mc_stats_decode (keys -> f32).  Gathered on chip first (McAcc: a thread's registers, then
//   a table of roots in LDS), so the root of a large component receives a few global atomics a block, not one per vertex.
// Filter (block_scan.h: ballots and scanned block totals, no atomics; a block owns 256 consecutive vertices AND 256 consecutive
// faces, the totals are (kept vertices, kept faces)):
//   k_mc_count     -> totals[block]; k_bs_scan / k_bs_scan_add -> offsets, header {Vk, Fk, V, F}
//   k_mc_emit_verts  index_map[v] = new id or -1, verts_out
//   k_mc_emit_faces  a launch of its own (it reads other vertices' index_map): faces_out, re-indexed
#include <algorithm>

#include "block_scan.h"
#include "uf_core.h"

#define MC_BLOCK BS_BLOCK
#define MC_MAX 0x7fffffffu               // V, F < 2^31
#define MC_KEY_PINF 0xff800000u          // mc_key(+inf), mc_key(-inf): the empty box
#define MC_KEY_NINF 0x007fffffu

// ---- device helpers -------------------------------------------------------------------------------------------------------
// the face's three indices; false (and nothing may be dereferenced through them) when one lies outside [0, V)
__device__ __forceinline__ bool mc_face(const int32_t *__restrict__ faces, uint32_t f, uint32_t V, uint32_t &a, uint32_t &b,
                                        uint32_t &c) {
    const int32_t *p = faces + (size_t)f * 3;
    a = (uint32_t)p[0], b = (uint32_t)p[1], c = (uint32_t)p[2];      // a negative index is >= 2^31 > V
    return a < V && b < V && c < V;
}

// f32 -> uint32 whose unsigned order is the floats' order (-0 below +0)
__device__ __forceinline__ uint32_t mc_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float mc_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

// ---- labelling ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MC_BLOCK) k_mc_init(uint32_t *__restrict__ parent, uint32_t V, uint32_t *__restrict__ bad) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v < V) parent[v] = v;
    if (v == 0) *bad = 0u;
}

__global__ void __launch_bounds__(MC_BLOCK) k_mc_union(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, uint32_t *parent,
                                                       uint32_t *bad) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t a, b, c;
    if (!mc_face(faces, f, V, a, b, c)) {
        atomicAdd(bad, 1u);
        return;
    }
    if (a != b) uf_unite(parent, a, b);
    if (b != c) uf_unite(parent, b, c);
}

__global__ void __launch_bounds__(MC_BLOCK) k_mc_flatten(uint32_t *parent, uint32_t V) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v < V) uf_min(parent + v, uf_find(parent, v));     // the root is an ancestor: still only a decrease
}

// ---- statistics -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MC_BLOCK) k_mc_stats_init(uint32_t V, uint32_t *__restrict__ n_verts, uint32_t *__restrict__ n_faces,
                                                            uint32_t *__restrict__ lo, uint32_t *__restrict__ hi) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    n_verts[v] = 0u, n_faces[v] = 0u;
#pragma unroll
    for (int a = 0; a < 3; a++) lo[(size_t)v * 3 + a] = MC_KEY_PINF, hi[(size_t)v * 3 + a] = MC_KEY_NINF;
}

// Atomics to ONE global address are served one after the other, chip-wide, and a mesh is mostly a few large components whose
// vertex ids interleave (a surface-nets mesh numbers its vertices in cell order, across all its sheets), so the statistics are
// gathered on chip first, in two stages, and a root receives a few global atomics a BLOCK, not one per item:
//   registers  a thread gathers for one root.  Another root's item goes to the block's table, score--; at score == 0 what was
//              gathered goes to the table and the thread gathers for the new root; score = min(score + 1, MC_SCORE_CAP) on a hit
//   LDS table  MC_SLOTS roots a block, open addressing, LDS atomics; a root that finds no slot in MC_PROBES tries goes to global
//              memory directly (a small component: its addresses are its own)
// A block owns a contiguous range of the items, so its table holds the roots of that range; at its end it sends every slot once.
#define MC_STATS_BLOCKS 1024u
#define MC_STATS_ITEMS 16u                          // items a thread, at least, before the grid grows to MC_STATS_BLOCKS
#define MC_SCORE_CAP 4u
#define MC_NO_ROOT 0xffffffffu
#define MC_SLOTS 128u
#define MC_PROBES 4u

struct McTable {
    uint32_t key[MC_SLOTS], n[MC_SLOTS], mn[MC_SLOTS * 3], mx[MC_SLOTS * 3];
};

template <bool BOX>
struct McAcc {
    uint32_t root, count, score;
    uint32_t mn[3], mx[3];
    McTable &t;
    uint32_t *n, *lo, *hi;                          // the global arrays (n: n_verts or n_faces)

    // All threads of the block call it.
    __device__ __forceinline__ McAcc(McTable &t_, uint32_t *n_, uint32_t *lo_, uint32_t *hi_)
        : root(MC_NO_ROOT), count(0u), score(0u), t(t_), n(n_), lo(lo_), hi(hi_) {
#pragma unroll
        for (int a = 0; a < 3; a++) mn[a] = MC_KEY_PINF, mx[a] = MC_KEY_NINF;
        for (uint32_t i = threadIdx.x; i < MC_SLOTS; i += MC_BLOCK) {
            t.key[i] = MC_NO_ROOT, t.n[i] = 0u;
#pragma unroll
            for (int a = 0; a < 3; a++) t.mn[i * 3 + a] = MC_KEY_PINF, t.mx[i * 3 + a] = MC_KEY_NINF;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void send_global(uint32_t r, uint32_t c, const uint32_t *kmn, const uint32_t *kmx) const {
        atomicAdd(n + r, c);
        if (BOX) {
#pragma unroll
            for (int a = 0; a < 3; a++) atomicMin(lo + (size_t)r * 3 + a, kmn[a]), atomicMax(hi + (size_t)r * 3 + a, kmx[a]);
        }
    }
    __device__ __forceinline__ void send(uint32_t r, uint32_t c, const uint32_t *kmn, const uint32_t *kmx) const {
        const uint32_t h = (r * 2654435761u) >> 25;                                   // 7 bits: MC_SLOTS
        for (uint32_t probe = 0; probe < MC_PROBES; probe++) {
            const uint32_t slot = (h + probe) & (MC_SLOTS - 1u);
            const uint32_t seen = atomicCAS(&t.key[slot], MC_NO_ROOT, r);
            if (seen != MC_NO_ROOT && seen != r) continue;
            atomicAdd(&t.n[slot], c);
            if (BOX) {
#pragma unroll
                for (int a = 0; a < 3; a++) atomicMin(&t.mn[slot * 3 + a], kmn[a]), atomicMax(&t.mx[slot * 3 + a], kmx[a]);
            }
            return;
        }
        send_global(r, c, kmn, kmx);
    }
    __device__ __forceinline__ void add(uint32_t r, const uint32_t *k) {
        if (r == root) {
            count++;
            score = min(score + 1u, MC_SCORE_CAP);
#pragma unroll
            for (int a = 0; BOX && a < 3; a++) mn[a] = min(mn[a], k[a]), mx[a] = max(mx[a], k[a]);
        } else if (score == 0u) {
            if (count) send(root, count, mn, mx);
            root = r, count = 1u, score = 1u;
#pragma unroll
            for (int a = 0; BOX && a < 3; a++) mn[a] = mx[a] = k[a];
        } else {
            score--;
            send(r, 1u, k, k);
        }
    }
    // All threads of the block call it.
    __device__ __forceinline__ void finish() {
        if (count) send(root, count, mn, mx);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < MC_SLOTS; i += MC_BLOCK)
            if (t.key[i] != MC_NO_ROOT) send_global(t.key[i], t.n[i], t.mn + i * 3, t.mx + i * 3);
    }
};

// the block's contiguous range of n items: [begin, end)
__device__ __forceinline__ void mc_block_range(uint32_t n, uint64_t &begin, uint64_t &end) {
    const uint64_t chunk = ((uint64_t)n + gridDim.x - 1) / gridDim.x;
    begin = (uint64_t)blockIdx.x * chunk;
    end = begin + chunk < n ? begin + chunk : n;
}

__global__ void __launch_bounds__(MC_BLOCK) k_mc_stats_verts(const float *__restrict__ verts, const int32_t *__restrict__ labels,
                                                             uint32_t V, uint32_t *n_verts, uint32_t *lo, uint32_t *hi) {
    __shared__ McTable table;
    McAcc<true> acc(table, n_verts, lo, hi);
    uint64_t begin, end;
    mc_block_range(V, begin, end);
    for (uint64_t v = begin + threadIdx.x; v < end; v += MC_BLOCK) {
        const uint32_t r = (uint32_t)labels[v];
        if (r >= V) continue;                       // labels that are not this mesh's: nothing is written through them
        uint32_t k[3];
#pragma unroll
        for (int a = 0; a < 3; a++) k[a] = mc_key(verts[v * 3 + a]);
        acc.add(r, k);
    }
    acc.finish();
}

__global__ void __launch_bounds__(MC_BLOCK) k_mc_stats_faces(const int32_t *__restrict__ faces, const int32_t *__restrict__ labels,
                                                             uint32_t V, uint32_t F, uint32_t *n_faces) {
    __shared__ McTable table;
    McAcc<false> acc(table, n_faces, nullptr, nullptr);
    uint64_t begin, end;
    mc_block_range(F, begin, end);
    for (uint64_t f = begin + threadIdx.x; f < end; f += MC_BLOCK) {
        uint32_t a, b, c;
        if (!mc_face(faces, (uint32_t)f, V, a, b, c)) continue;
        const uint32_t r = (uint32_t)labels[a];
        if (r < V) acc.add(r, nullptr);
    }
    acc.finish();
}

// keys -> f32 in place; a vertex that is no root keeps the empty box (+inf, -inf)
__global__ void __launch_bounds__(MC_BLOCK) k_mc_stats_decode(uint32_t V, uint32_t *lo, uint32_t *hi) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const size_t i = (size_t)v * 3 + a;
        lo[i] = __float_as_uint(mc_unkey(lo[i]));
        hi[i] = __float_as_uint(mc_unkey(hi[i]));
    }
}

// ---- filter ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mc_keep_vertex(const int32_t *__restrict__ labels, const uint8_t *__restrict__ keep, uint32_t V,
                                               uint32_t v) {
    const uint32_t r = (uint32_t)labels[v];
    return r < V && keep[r] != 0;
}

// the face's indices when it is kept
__device__ __forceinline__ bool mc_keep_face(const int32_t *__restrict__ faces, const int32_t *__restrict__ labels,
                                             const uint8_t *__restrict__ keep, uint32_t V, uint32_t F, uint32_t f, uint32_t &a,
                                             uint32_t &b, uint32_t &c) {
    return f < F && mc_face(faces, f, V, a, b, c) && mc_keep_vertex(labels, keep, V, a);
}

__global__ void __launch_bounds__(MC_BLOCK) k_mc_count(const int32_t *__restrict__ faces, const int32_t *__restrict__ labels,
                                                       const uint8_t *__restrict__ keep, uint32_t V, uint32_t F,
                                                       uint2 *__restrict__ totals) {
    __shared__ uint32_t s_wave[MC_BLOCK / 64];
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t a, b, c;
    const uint32_t kv = (i < V && mc_keep_vertex(labels, keep, V, i)) ? 1u : 0u;
    const uint32_t kf = mc_keep_face(faces, labels, keep, V, F, i, a, b, c) ? 1u : 0u;
    uint32_t nv, nf;
    bs_block_rank(kv, s_wave, nv);
    bs_block_rank(kf, s_wave, nf);
    if (threadIdx.x == 0) totals[blockIdx.x] = make_uint2(nv, nf);
}

__global__ void __launch_bounds__(MC_BLOCK) k_mc_emit_verts(const float *__restrict__ verts, const int32_t *__restrict__ labels,
                                                            const uint8_t *__restrict__ keep, uint32_t V,
                                                            const uint2 *__restrict__ offsets, uint32_t Vk,
                                                            int32_t *__restrict__ index_map, float *__restrict__ verts_out) {
    __shared__ uint32_t s_wave[MC_BLOCK / 64];
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t kv = (v < V && mc_keep_vertex(labels, keep, V, v)) ? 1u : 0u;
    uint32_t total;
    const uint32_t id = offsets[blockIdx.x].x + bs_block_rank(kv, s_wave, total);
    if (v >= V) return;
    const bool emit = kv && id < Vk;                // id >= Vk: a Vk that is not this workspace's (refused on the host already)
    index_map[v] = emit ? (int32_t)id : -1;
    if (!emit) return;
    const float *src = verts + (size_t)v * 3;
    float *o = verts_out + (size_t)id * 3;
    o[0] = src[0], o[1] = src[1], o[2] = src[2];
}

__global__ void __launch_bounds__(MC_BLOCK) k_mc_emit_faces(const int32_t *__restrict__ faces, const int32_t *__restrict__ labels,
                                                            const uint8_t *__restrict__ keep, uint32_t V, uint32_t F,
                                                            const uint2 *__restrict__ offsets, uint32_t Fk,
                                                            const int32_t *__restrict__ index_map, int32_t *__restrict__ faces_out) {
    __shared__ uint32_t s_wave[MC_BLOCK / 64];
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t a = 0u, b = 0u, c = 0u;
    const uint32_t kf = mc_keep_face(faces, labels, keep, V, F, f, a, b, c) ? 1u : 0u;
    uint32_t total;
    const uint32_t id = offsets[blockIdx.x].y + bs_block_rank(kf, s_wave, total);
    if (!kf || id >= Fk) return;
    int32_t *o = faces_out + (size_t)id * 3;        // a kept face's vertices are of its component: all kept
    o[0] = index_map[a], o[1] = index_map[b], o[2] = index_map[c];
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
static inline bool mc_misaligned4(const void *p) { return ((uintptr_t)p & 3) != 0; }

// the block totals' levels: a block owns 256 vertices and 256 faces (an empty mesh still has one block)
static inline BsLevels mc_levels(uint32_t V, uint32_t F) {
    const uint32_t n = V > F ? V : F;
    return bs_levels(nsr_div_up(n ? n : 1u, MC_BLOCK));
}

extern "C" {

int nsr_mesh_components(const int32_t *faces, uint32_t V, uint32_t F, int32_t *labels, uint32_t *bad_faces, nsr_stream_t stream) {
    if (V > MC_MAX || F > MC_MAX) return NSR_ERR_INVALID_ARG;
    NSR_CHECK_PTR(bad_faces);
    if (V != 0) NSR_CHECK_PTR(labels);
    if (F != 0) NSR_CHECK_PTR(faces);
    if (mc_misaligned4(faces) || mc_misaligned4(labels) || mc_misaligned4(bad_faces)) return NSR_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    uint32_t *parent = (uint32_t *)labels;
    hipLaunchKernelGGL(k_mc_init, dim3(nsr_div_up(V ? V : 1u, MC_BLOCK)), dim3(MC_BLOCK), 0, st, parent, V, bad_faces);
    if (F != 0) hipLaunchKernelGGL(k_mc_union, dim3(nsr_div_up(F, MC_BLOCK)), dim3(MC_BLOCK), 0, st, faces, V, F, parent, bad_faces);
    if (V != 0 && F != 0) hipLaunchKernelGGL(k_mc_flatten, dim3(nsr_div_up(V, MC_BLOCK)), dim3(MC_BLOCK), 0, st, parent, V);
    return nsr_launch_status();
}

int nsr_mesh_component_stats(const float *verts, const int32_t *faces, const int32_t *labels, uint32_t V, uint32_t F,
                             uint32_t *n_verts, uint32_t *n_faces, float *lo, float *hi, nsr_stream_t stream) {
    if (V > MC_MAX || F > MC_MAX) return NSR_ERR_INVALID_ARG;
    if (V != 0) {
        NSR_CHECK_PTR(verts);
        NSR_CHECK_PTR(labels);
        NSR_CHECK_PTR(n_verts);
        NSR_CHECK_PTR(n_faces);
        NSR_CHECK_PTR(lo);
        NSR_CHECK_PTR(hi);
    }
    if (F != 0) NSR_CHECK_PTR(faces);
    if (mc_misaligned4(verts) || mc_misaligned4(faces) || mc_misaligned4(labels) || mc_misaligned4(n_verts) || mc_misaligned4(n_faces) ||
        mc_misaligned4(lo) || mc_misaligned4(hi))
        return NSR_ERR_INVALID_ARG;
    if (V == 0) return NSR_OK;                      // no vertex, so no good face and no root
    hipStream_t st = (hipStream_t)stream;
    const dim3 gv(nsr_div_up(V, MC_BLOCK)), blk(MC_BLOCK);
    uint32_t *klo = (uint32_t *)lo, *khi = (uint32_t *)hi;
    hipLaunchKernelGGL(k_mc_stats_init, gv, blk, 0, st, V, n_verts, n_faces, klo, khi);
    const auto ranges = [](uint32_t n) { return dim3(std::min(nsr_div_up(n, MC_BLOCK * MC_STATS_ITEMS), MC_STATS_BLOCKS)); };
    hipLaunchKernelGGL(k_mc_stats_verts, ranges(V), blk, 0, st, verts, labels, V, n_verts, klo, khi);
    if (F != 0) hipLaunchKernelGGL(k_mc_stats_faces, ranges(F), blk, 0, st, faces, labels, V, F, n_faces);
    hipLaunchKernelGGL(k_mc_stats_decode, gv, blk, 0, st, V, klo, khi);
    return nsr_launch_status();
}

uint64_t nsr_mesh_filter_workspace_bytes(uint32_t V, uint32_t F) {
    if (V > MC_MAX || F > MC_MAX) return 0;
    return mc_levels(V, F).end;
}

int nsr_mesh_filter_count(const int32_t *faces, const int32_t *labels, const uint8_t *keep, uint32_t V, uint32_t F, void *workspace,
                          uint32_t *counts_out, nsr_stream_t stream) {
    if (V > MC_MAX || F > MC_MAX) return NSR_ERR_INVALID_ARG;
    NSR_CHECK_PTR(workspace);
    NSR_CHECK_PTR(counts_out);
    if (V != 0) {
        NSR_CHECK_PTR(labels);
        NSR_CHECK_PTR(keep);
    }
    if (F != 0) NSR_CHECK_PTR(faces);
    if (mc_misaligned4(faces) || mc_misaligned4(labels) || mc_misaligned4(counts_out) || ((uintptr_t)workspace & 15))
        return NSR_ERR_INVALID_ARG;
    const BsLevels l = mc_levels(V, F);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    hipLaunchKernelGGL(k_mc_count, dim3(l.n[0]), dim3(MC_BLOCK), 0, st, faces, labels, keep, V, F, (uint2 *)(ws + l.off[0]));
    bs_scan_levels(ws, l, counts_out, make_uint3(V, F, 0u), st);      // header {Vk, Fk, V, F}
    return nsr_launch_status();
}

int nsr_mesh_filter_emit(const float *verts, const int32_t *faces, const int32_t *labels, const uint8_t *keep, uint32_t V,
                         uint32_t F, void *workspace, uint32_t Vk, uint32_t Fk, int32_t *index_map, float *verts_out,
                         int32_t *faces_out, nsr_stream_t stream) {
    if (V > MC_MAX || F > MC_MAX) return NSR_ERR_INVALID_ARG;
    NSR_CHECK_PTR(workspace);
    if (V != 0) {
        NSR_CHECK_PTR(verts);
        NSR_CHECK_PTR(labels);
        NSR_CHECK_PTR(keep);
        NSR_CHECK_PTR(index_map);
    }
    if (F != 0) NSR_CHECK_PTR(faces);
    if (Vk != 0) NSR_CHECK_PTR(verts_out);
    if (Fk != 0) NSR_CHECK_PTR(faces_out);
    if (mc_misaligned4(verts) || mc_misaligned4(faces) || mc_misaligned4(labels) || mc_misaligned4(index_map) ||
        mc_misaligned4(verts_out) || mc_misaligned4(faces_out) || ((uintptr_t)workspace & 15))
        return NSR_ERR_INVALID_ARG;
    if (Vk > V || Fk > F || (Vk == 0 && Fk != 0)) return NSR_ERR_INVALID_ARG;
    // Vk and Fk size the caller's outputs: they are checked against what the count left before anything is written through them
    hipStream_t st = (hipStream_t)stream;
    uint32_t header[4];
    if (hipMemcpyAsync(header, workspace, sizeof(header), hipMemcpyDeviceToHost, st) != hipSuccess) return NSR_ERR_LAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return NSR_ERR_LAUNCH;
    if (header[0] != Vk || header[1] != Fk || header[2] != V || header[3] != F) return NSR_ERR_INVALID_ARG;
    if (V == 0) return NSR_OK;

    const BsLevels l = mc_levels(V, F);
    const uint2 *offsets = (const uint2 *)((char *)workspace + l.off[0]);
    hipLaunchKernelGGL(k_mc_emit_verts, dim3(nsr_div_up(V, MC_BLOCK)), dim3(MC_BLOCK), 0, st, verts, labels, keep, V, offsets, Vk,
                       index_map, verts_out);
    if (Fk != 0)
        hipLaunchKernelGGL(k_mc_emit_faces, dim3(nsr_div_up(F, MC_BLOCK)), dim3(MC_BLOCK), 0, st, faces, labels, keep, V, F, offsets,
                           Fk, (const int32_t *)index_map, faces_out);
    return nsr_launch_status();
}

}  // extern "C"
