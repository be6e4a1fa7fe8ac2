// Naive surface nets (Gibson 1998) of a scalar volume: the iso-surface as a deterministic indexed triangle mesh, in two calls
// (nsr_surface_nets_count / nsr_surface_nets_emit; include/nsr.h, "Mesh export", states the definition).
//
// A workgroup of 256 threads owns 256 CONSECUTIVE cells of the linear cell order (cz fastest, as the volume's k), one thread a
// cell, so that the vertex ids -- the rank of a cell among the active ones in that order -- and the face order fall out of a
// block-local rank plus the scanned block totals, with no atomics anywhere:
//   k_sn_count     8 corner reads -> corner mask, active flag, owned quads (0..3); totals[block] = (vertices, quads)
//   k_bs_scan, k_bs_scan_add (block_scan.h)  the totals scanned into exclusive offsets, level by level: 1023^3 cells are
//                  4.2 M blocks -> 16 K -> 64 -> 1
//   k_sn_vertices  recomputes the mask and the in-block rank; verts[id], cell_vertex[cell] = id
//   k_sn_faces     a launch of its own (it reads its neighbours' ids): 4 corner reads, the owned edges' quads at their offsets
// In-block ranks (bs_block_rank): wave64 ballots and a popcount below the lane (two ballots for the 2-bit quad count), then the
// four wave totals through LDS.  Reads are coalesced along k; the four (x, y) rows a wave touches are re-read by its neighbours from L1/L2, they
// are not staged in LDS (a block's 256 cells wrap over rows of any length).  HBM traffic: the volume three times (count,
// vertices, faces), cell_vertex and the outputs once.
//
// The whole file is compiled with contraction off: tests/mesh_ref.py reaches the vertices' bits with NumPy f32.
#include "block_scan.h"

#pragma clang fp contract(off)

#define SN_BLOCK BS_BLOCK
#define SN_MAX_R 1024u                   // ceil(1023^3 / 256) = 4 181 880 block totals -> 16 336 -> 64 -> 1

struct SnShape {
    uint32_t R0, R1, R2;                 // lattice points an axis
    uint32_t n1, n2;                     // cells along y and z (R1 - 1, R2 - 1)
    uint32_t ncells;
};

struct SnLayout {                        // byte offsets into the workspace, each a multiple of 16
    BsLevels scan;                       // the header {V, Q, R0, R1, R2, 0, 0, 0} and the levels of block totals
    uint64_t cell_vertex;
    uint64_t bytes;
};

static bool sn_shape(uint32_t R0, uint32_t R1, uint32_t R2, SnShape *s) {
    if (R0 < 2 || R1 < 2 || R2 < 2 || R0 > SN_MAX_R || R1 > SN_MAX_R || R2 > SN_MAX_R) return false;
    s->R0 = R0, s->R1 = R1, s->R2 = R2;
    s->n1 = R1 - 1, s->n2 = R2 - 1;
    s->ncells = (R0 - 1) * s->n1 * s->n2;          // < 2^30
    return true;
}

static SnLayout sn_layout(const SnShape &s) {
    SnLayout l;
    l.scan = bs_levels(nsr_div_up(s.ncells, SN_BLOCK));
    l.cell_vertex = l.scan.end;
    l.bytes = l.cell_vertex + (((uint64_t)s.ncells * 4 + 15) & ~15ull);
    return l;
}

// ---- device helpers -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sn_inside(float v, float iso) { return v > iso; }      // NaN and v == iso: outside

__device__ __forceinline__ void sn_cell(const SnShape &s, uint32_t c, uint32_t &cx, uint32_t &cy, uint32_t &cz) {
    const uint32_t t = c / s.n2;
    cz = c - t * s.n2;
    cx = t / s.n1;
    cy = t - cx * s.n1;
}

// corner q = 4 dx + 2 dy + dz of cell (cx, cy, cz): the C order of vol[cx:cx+2, cy:cy+2, cz:cz+2]
__device__ __forceinline__ void sn_corners(const float *__restrict__ vol, const SnShape &s, uint32_t cx, uint32_t cy, uint32_t cz,
                                           float v[8]) {
    const size_t base = ((size_t)cx * s.R1 + cy) * s.R2 + cz;
    const size_t dy = s.R2, dx = (size_t)s.R1 * s.R2;
    v[0] = vol[base], v[1] = vol[base + 1];
    v[2] = vol[base + dy], v[3] = vol[base + dy + 1];
    v[4] = vol[base + dx], v[5] = vol[base + dx + 1];
    v[6] = vol[base + dx + dy], v[7] = vol[base + dx + dy + 1];
}

__device__ __forceinline__ uint32_t sn_mask(const float v[8], float iso) {
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) m |= sn_inside(v[q], iso) ? 1u << q : 0u;
    return m;
}

// bit a (0 = x, 1 = y, 2 = z): the cell owns a quad on the lattice edge that leaves its minimum corner along axis a
__device__ __forceinline__ uint32_t sn_quads(bool in0, bool inx, bool iny, bool inz, uint32_t cx, uint32_t cy, uint32_t cz) {
    uint32_t q = 0;
    if (in0 != inx && cy >= 1 && cz >= 1) q |= 1u;
    if (in0 != iny && cx >= 1 && cz >= 1) q |= 2u;
    if (in0 != inz && cx >= 1 && cy >= 1) q |= 4u;
    return q;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SN_BLOCK) k_sn_count(const float *__restrict__ vol, SnShape s, float iso, uint2 *__restrict__ totals) {
    __shared__ uint32_t s_wave[SN_BLOCK / 64];
    const uint32_t c = blockIdx.x * SN_BLOCK + threadIdx.x;
    uint32_t active = 0, nq = 0;
    if (c < s.ncells) {
        uint32_t cx, cy, cz;
        sn_cell(s, c, cx, cy, cz);
        float v[8];
        sn_corners(vol, s, cx, cy, cz, v);
        const uint32_t m = sn_mask(v, iso);
        active = (m != 0u && m != 0xffu) ? 1u : 0u;
        nq = (uint32_t)__popc(sn_quads(m & 1u, m & 16u, m & 4u, m & 2u, cx, cy, cz));
    }
    uint32_t nv_total, nq_total;
    bs_block_rank(active, s_wave, nv_total);
    bs_block_rank(nq, s_wave, nq_total);
    if (threadIdx.x == 0) totals[blockIdx.x] = make_uint2(nv_total, nq_total);
}

struct SnBox {
    float lo[3], step[3];
};

// coordinate i of the lattice along axis a
__device__ __forceinline__ float sn_coord(const SnBox &b, int a, uint32_t i) { return b.lo[a] + (float)i * b.step[a]; }

__global__ void __launch_bounds__(SN_BLOCK) k_sn_vertices(const float *__restrict__ vol, SnShape s, float iso, SnBox box,
                                                          const uint2 *__restrict__ offsets, uint32_t V,
                                                          float *__restrict__ verts, int32_t *__restrict__ cell_vertex) {
    __shared__ uint32_t s_wave[SN_BLOCK / 64];
    const uint32_t c = blockIdx.x * SN_BLOCK + threadIdx.x;
    uint32_t cx = 0, cy = 0, cz = 0, m = 0;
    float v[8];
    if (c < s.ncells) {
        sn_cell(s, c, cx, cy, cz);
        sn_corners(vol, s, cx, cy, cz, v);
        m = sn_mask(v, iso);
    }
    const uint32_t active = (m != 0u && m != 0xffu) ? 1u : 0u;
    uint32_t total;
    const uint32_t id = offsets[blockIdx.x].x + bs_block_rank(active, s_wave, total);
    if (!active || id >= V) return;                 // id >= V: a V that is not this workspace's (refused on the host already)

    // the lattice coordinates of the cell's two planes an axis
    const uint32_t ci[3] = {cx, cy, cz};
    float coord[3][2];
#pragma unroll
    for (int a = 0; a < 3; a++) coord[a][0] = sn_coord(box, a, ci[a]), coord[a][1] = sn_coord(box, a, ci[a] + 1u);
    float sum[3] = {0.0f, 0.0f, 0.0f};
    uint32_t n = 0;
    // the 12 edges in the header's order: along x (0,4) (1,5) (2,6) (3,7), along y (0,2) (1,3) (4,6) (5,7), along z (0,1) (2,3)
    // (4,5) (6,7); corner q sits at (cx + (q >> 2), cy + ((q >> 1) & 1), cz + (q & 1))
#pragma unroll
    for (int e = 0; e < 12; e++) {
        const int axis = e >> 2, j = e & 3;
        const int qa = axis == 0 ? j : axis == 1 ? ((j & 2) << 1) | (j & 1) : j << 1;     // the end at the cell's lower plane
        const int qb = qa | (4 >> axis);
        const bool ia = (m >> qa) & 1u, ib = (m >> qb) & 1u;
        if (ia == ib) continue;
        // a: the outside end, b: the inside end
        const float va = ia ? v[qb] : v[qa], vb = ia ? v[qa] : v[qb];
        float t = (iso - va) / (vb - va);
        if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;                                    // a NaN or -inf outside end: the midpoint
        float p[3];
#pragma unroll
        for (int a = 0; a < 3; a++) p[a] = coord[a][(qa >> (2 - a)) & 1];
        const float pa = ia ? coord[axis][1] : coord[axis][0], pb = ia ? coord[axis][0] : coord[axis][1];
        p[axis] = pa + t * (pb - pa);
#pragma unroll
        for (int a = 0; a < 3; a++) sum[a] = sum[a] + p[a];
        n++;
    }
    const float fn = (float)n;
    float *o = verts + (size_t)id * 3;
    o[0] = sum[0] / fn, o[1] = sum[1] / fn, o[2] = sum[2] / fn;
    cell_vertex[c] = (int32_t)id;
}

__global__ void __launch_bounds__(SN_BLOCK) k_sn_faces(const float *__restrict__ vol, SnShape s, float iso,
                                                       const uint2 *__restrict__ offsets, uint32_t Q,
                                                       const int32_t *__restrict__ cell_vertex, int32_t *__restrict__ faces) {
    __shared__ uint32_t s_wave[SN_BLOCK / 64];
    const uint32_t c = blockIdx.x * SN_BLOCK + threadIdx.x;
    uint32_t cx = 0, cy = 0, cz = 0, quads = 0;
    bool in0 = false;
    if (c < s.ncells) {
        sn_cell(s, c, cx, cy, cz);
        const size_t base = ((size_t)cx * s.R1 + cy) * s.R2 + cz;
        in0 = sn_inside(vol[base], iso);
        quads = sn_quads(in0, sn_inside(vol[base + (size_t)s.R1 * s.R2], iso), sn_inside(vol[base + s.R2], iso),
                         sn_inside(vol[base + 1], iso), cx, cy, cz);
    }
    uint32_t total;
    uint32_t q = offsets[blockIdx.x].y + bs_block_rank((uint32_t)__popc(quads), s_wave, total);
    if (!quads) return;
    // cells around the owned edge, counter-clockwise seen from the axis' positive end (normal +axis): the linear-index steps
    // back along the two other axes, in the cyclic order (y, z), (z, x), (x, y)
    const uint32_t sx = s.n1 * s.n2, sy = s.n2, sz = 1u;
    const uint32_t su[3] = {sy, sz, sx}, sv[3] = {sz, sx, sy};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (!((quads >> a) & 1u)) continue;
        if (q >= Q) return;                         // a Q that is not this workspace's (refused on the host already)
        const int32_t v0 = cell_vertex[c - su[a] - sv[a]], v1 = cell_vertex[c - sv[a]], v2 = cell_vertex[c],
                      v3 = cell_vertex[c - su[a]];
        // inside -> outside along +axis keeps the order; the other way round turns it
        const int32_t w1 = in0 ? v1 : v3, w3 = in0 ? v3 : v1;
        int32_t *o = faces + (size_t)q * 6;
        o[0] = v0, o[1] = w1, o[2] = v2;
        o[3] = v0, o[4] = v2, o[5] = w3;
        q++;
    }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
extern "C" {

uint64_t nsr_surface_nets_workspace_bytes(uint32_t R0, uint32_t R1, uint32_t R2) {
    SnShape s;
    if (!sn_shape(R0, R1, R2, &s)) return 0;
    return sn_layout(s).bytes;
}

int nsr_surface_nets_count(const float *vol, uint32_t R0, uint32_t R1, uint32_t R2, float iso, void *workspace,
                           uint32_t *counts_out, nsr_stream_t stream) {
    SnShape s;
    if (!sn_shape(R0, R1, R2, &s)) return NSR_ERR_INVALID_ARG;
    NSR_CHECK_PTR(vol);
    NSR_CHECK_PTR(workspace);
    NSR_CHECK_PTR(counts_out);
    if (((uintptr_t)vol & 3) || ((uintptr_t)counts_out & 3) || ((uintptr_t)workspace & 15)) return NSR_ERR_INVALID_ARG;
    const SnLayout l = sn_layout(s);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    hipLaunchKernelGGL(k_sn_count, dim3(l.scan.n[0]), dim3(SN_BLOCK), 0, st, vol, s, iso, (uint2 *)(ws + l.scan.off[0]));
    bs_scan_levels(ws, l.scan, counts_out, make_uint3(R0, R1, R2), st);   // the shape it was counted for beside the totals
    return nsr_launch_status();
}

int nsr_surface_nets_emit(const float *vol, uint32_t R0, uint32_t R1, uint32_t R2, float iso, const float *lo, const float *step,
                          void *workspace, uint32_t V, uint32_t Q, float *verts, int32_t *faces, nsr_stream_t stream) {
    SnShape s;
    if (!sn_shape(R0, R1, R2, &s)) return NSR_ERR_INVALID_ARG;
    NSR_CHECK_PTR(vol);
    NSR_CHECK_PTR(lo);
    NSR_CHECK_PTR(step);
    NSR_CHECK_PTR(workspace);
    if (V != 0) NSR_CHECK_PTR(verts);
    if (Q != 0) NSR_CHECK_PTR(faces);
    if (((uintptr_t)vol & 3) || ((uintptr_t)verts & 3) || ((uintptr_t)faces & 3) || ((uintptr_t)workspace & 15))
        return NSR_ERR_INVALID_ARG;
    if (V > s.ncells || Q > 3ull * s.ncells || (V == 0 && Q != 0)) return NSR_ERR_INVALID_ARG;
    // the one host read of the library: V and Q size the outputs, so they are checked against what the count left before
    // anything is written through them
    hipStream_t st = (hipStream_t)stream;
    uint32_t header[5];
    if (hipMemcpyAsync(header, workspace, sizeof(header), hipMemcpyDeviceToHost, st) != hipSuccess) return NSR_ERR_LAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return NSR_ERR_LAUNCH;
    if (header[0] != V || header[1] != Q || header[2] != R0 || header[3] != R1 || header[4] != R2) return NSR_ERR_INVALID_ARG;
    if (V == 0) return NSR_OK;

    const SnLayout l = sn_layout(s);
    char *ws = (char *)workspace;
    const uint2 *offsets = (const uint2 *)(ws + l.scan.off[0]);
    int32_t *cell_vertex = (int32_t *)(ws + l.cell_vertex);
    SnBox box;
    for (int a = 0; a < 3; a++) box.lo[a] = lo[a], box.step[a] = step[a];
    hipLaunchKernelGGL(k_sn_vertices, dim3(l.scan.n[0]), dim3(SN_BLOCK), 0, st, vol, s, iso, box, offsets, V, verts, cell_vertex);
    if (Q != 0)
        hipLaunchKernelGGL(k_sn_faces, dim3(l.scan.n[0]), dim3(SN_BLOCK), 0, st, vol, s, iso, offsets, Q,
                           (const int32_t *)cell_vertex, faces);
    return nsr_launch_status();
}

}  // extern "C"
