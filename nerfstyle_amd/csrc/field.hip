// Fused field kernels for gfx950: BBox.normalize -> hash encode (both tables, one interleaved
// gather) -> density / color1 / color2 / class MLPs on MFMA -> trunc_exp / sigmoid / cat, in one
// launch per direction (reference: networks/style_nerf.py:120-142 with use_dir=False, which is
// 2 encoder launches + 4 tcnn launches + exp + cat, each round-tripping [M,.] through HBM).
//
// Work decomposition: a wave owns a tile of 16 consecutive samples (consecutive samples of one
// ray share cells on the coarse levels, so their gathers coalesce).  Lane (s = lane&15,
// g = lane>>4) encodes levels {2g, 2g+1, 8+2g, 9+2g} of sample s for BOTH encoders -- exactly
// the 8 elements the K=32 MFMA B fragment wants from that lane (features 4g..4g+3 of k-block 0
// and of k-block 1) -- so encode output feeds the matrix cores with no data movement, and in the
// backward the MFMA-produced input gradient lands on the lane that owns those levels' scatter.
// The forward kernel keeps all 32 table gathers of a lane's four levels in flight before it consumes the first (125
// instead of 74 VGPRs, still 4 waves per SIMD): 8.2 -> 8.0 ms on the bench frame.  Forward only -- the backward's re-gather
// path shares field_encode and has no registers to spare.
#include "field_common.h"
#include "lattice.h"
#include "table_scatter.h"

// rgbs[m, 4g .. 4g + 3] = cat(sigmoid(rgb), classes)
__device__ __forceinline__ void field_store_channels(const FieldArgs &a, uint32_t m, int g, f4v rgb, f4v cls) {
    float v[4];
    field_cat(g, rgb, cls, v);
    float *dst = a.rgbs + (size_t)m * a.C_ch;
    if (a.C_ch == 8) {
        if (g < 2) reinterpret_cast<float4 *>(dst)[g] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if ((uint32_t)(4 * g + e) < a.C_ch) dst[4 * g + e] = v[e];
    }
}

// DIRS (nsr_field_forward_dirs): `dirs` [M,3] are the samples' viewing directions, indexed like xyzs; lane (s, g) evaluates
// SH coefficients 4g..4g+3 of sample s (the four g lanes load one address: one request) for color2's K = 32 first layer.
template <typename TT, int CD, bool SIGMA_ONLY, bool DIRS = false>
__global__ void __launch_bounds__(256)
k_field_fwd(FieldArgsOf<DIRS> a) {
    const float *const dirs = field_dirs_of(a);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    short *wl = reinterpret_cast<short *>(smem);
    NsrLevel *lds_lv = reinterpret_cast<NsrLevel *>(smem + (SIGMA_ONLY ? FW_SIGMA_TOTAL : FW_IMAGE<DIRS>) * 2);
    field_build_fw<CD, SIGMA_ONLY, DIRS>(wl, a.params);
    if (threadIdx.x < 16) lds_lv[threadIdx.x] = a.lv[threadIdx.x];
    __syncthreads();

    const uint32_t Mc = FIELD_COUNT(a);
    const uint32_t ntiles = (Mc + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const TT *tables = reinterpret_cast<const TT *>(a.tables);
    const uint32_t lb = field_logical_block();
    // split by the DEVICE-side sample count (M is only a capacity): every block gets work
    const uint32_t tpb = (ntiles + gridDim.x - 1) / gridDim.x;
    const uint32_t t_begin = lb * tpb;
    const uint32_t t_end = min(t_begin + tpb, ntiles);

    for (uint32_t tile = t_begin + wave; tile < t_end; tile += 4) {
        const uint32_t mpos = tile * 16 + s;
        const bool valid = mpos < Mc;
        // spatially ordered walk (nsr_sample_order): position `mpos` of the order is sample perm[mpos] of the buffers
        const uint32_t m = (a.perm && valid) ? a.perm[mpos] : mpos;
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        if (valid) {
            u0 = field_unit(a.xyzs[(size_t)m * 3 + 0], a.bmin[0], a.bsize[0]);
            u1 = field_unit(a.xyzs[(size_t)m * 3 + 1], a.bmin[1], a.bsize[1]);
            u2 = field_unit(a.xyzs[(size_t)m * 3 + 2], a.bmin[2], a.bsize[2]);
        }
        const bool live = valid && field_in_unit_cube(u0, u1, u2);
        s8v xd, xc;
        field_encode<TT, CD, SIGMA_ONLY, true>(lds_lv, tables, u0, u1, u2, live, g, xd, xc, a.fast_levels);
        if (!SIGMA_ONLY && a.feats) {
            s8v *fo = reinterpret_cast<s8v *>(a.feats) + ((size_t)tile * 64 + lane) * 2;
            fo[0] = xd;
            fo[1] = xc;
        }

        const f4v o = field_density_net<CD>(wl, lane, xd);
        if (valid && g == 0) a.sigmas[m] = expf(o[0]) * a.density_scale;   // tcnn_nerf.py:55-60, renderer.py:225
        if (SIGMA_ONLY) continue;

        f4v rgb, cls;
        if constexpr (DIRS) field_colour_nets<CD, true>(wl, lane, xc, rgb, cls, field_sh_frag<CD>(dirs, m, valid, g));
        else field_colour_nets<CD>(wl, lane, xc, rgb, cls);
        if (valid) field_store_channels(a, m, g, rgb, cls);
    }
}

// ---------------------------------------------------------------------------------------------
// Lattice gather on the spatial walk (perm != NULL, 16-bit tables, a level table the scatter's lattices fit).
//
// The samples of a tile lie in one or two blocks of nsr_sample_order, and on the levels whose cells are larger than a block
// every one of them reads the same 2^3 .. 3^3 corners.  For the levels in FWD_LAT_LEVELS the wave keeps the table rows of the
// level's S^3 lattice (lattice.h: the scatter's geometry, anchored at the origin of the level's block group) in LDS: filled
// cooperatively, one row index per slot, when the tile's first live sample enters another group; lane (s, g) then reads its
// eight corners from LDS at slot (c - anchor) instead of hashing and gathering them.  A lane whose cell lies outside the
// lattice (another group than the first sample's, a random permutation) takes the global gather for that level, so every
// row value, weight and sum is the one k_field_fwd forms: outputs are bit-identical.
// Which levels: tools/sorted_scatter_sim.py gather and DESIGN.md "(r7) forward: lattice gather" -- the calls of levels 0..7
// (one level per 16-lane group) find their cell in the lattice for 99.9 % of the samples at 0.13 fills per tile in all; on
// the fine levels a fifth of the samples lie outside, so nearly every tile would run both paths: the calls of levels 8..15
// keep the gather.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t FWD_LAT_LEVELS = 0x00FFu;
// anchors per wave, in front of its lattices: one per level, or with directions one per level of FWD_LAT_LEVELS only -- the 512 B
// that brings the 2 KB larger weight image back to four workgroups per CU (40 960 B exactly on the default grid)
template <bool DIRS> constexpr int FWD_LAT_ANCHORS = DIRS ? 8 : 16;
static_assert((FWD_LAT_LEVELS >> 8) == 0, "with directions only levels 0..7 have an anchor");

typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u2v lds_row;        // one 8-byte table row in a lattice

struct FieldLatArgs {
    uint32_t key_mask;        // block-key bits that can move an anchor of a level in FWD_LAT_LEVELS
    uint32_t wave_bytes;      // anchors + lattices of one wave
};

// Re-anchors the levels of FWD_LAT_LEVELS at the group of block `key` and fills the lattices whose anchor moved.
// lds_lv[l].pad_ = S | shift << 4 | first slot << 8.
template <int NANCH>
__device__ __forceinline__ void field_lat_refill(const NsrLevel *lds_lv, const uint2 *__restrict__ tables, uint4 *anch, uint2 *lat,
                                                 uint32_t key, int lane) {
    const uint32_t kmask = (1u << LAT_KEY_BITS) - 1u;
    const int l = lane & 15;
    const NsrLevel mlv = lds_lv[l];
    const uint32_t sh = (mlv.pad_ >> 4) & 0xFu;
    const float rk = 1.0f / (float)(1 << LAT_KEY_BITS);
    float ff;
    uint32_t n0, n1, n2;
    nsr_grid_locate((float)(((key & kmask) >> sh) << sh) * rk, mlv.resolution, 1, ff, n0);
    nsr_grid_locate((float)((((key >> LAT_KEY_BITS) & kmask) >> sh) << sh) * rk, mlv.resolution, 1, ff, n1);
    nsr_grid_locate((float)(((key >> (2 * LAT_KEY_BITS)) >> sh) << sh) * rk, mlv.resolution, 1, ff, n2);
    const uint4 old = anch[l & (NANCH - 1)];
    const bool chg = lane < 16 && ((FWD_LAT_LEVELS >> l) & 1u) && (n0 != old.x || n1 != old.y || n2 != old.z);
    if (chg) anch[l] = make_uint4(n0, n1, n2, 0u);
    uint32_t stale = (uint32_t)__ballot(chg);
    __builtin_amdgcn_wave_barrier();
    while (stale) {                                                   // wave-uniform
        const int fl = __builtin_ctz(stale);
        stale &= stale - 1u;
        const NsrLevel lv = lds_lv[fl];
        const uint4 an = anch[fl];
        const uint32_t S = lv.pad_ & 0xFu, NC = S * S * S;
        uint2 *dst = lat + (lv.pad_ >> 8);
        for (uint32_t k = lane; k < NC; k += 64) {
            const uint32_t z = k / (S * S), r = k - z * (S * S), y = r / S, x = r - y * S;
            // corners past the grid's last one are no cell's corner: the slot is never read, the fetch stays inside the level
            const uint32_t row = lv.offset + lat_row(lv, min(an.x + x, lv.resolution), min(an.y + y, lv.resolution),
                                                     min(an.z + z, lv.resolution));
            dst[k] = tables[row];
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// field_encode's batched gather with the calls of FWD_LAT_LEVELS read from the wave's lattices
template <int CD>
__device__ __forceinline__ void field_encode_lat(const NsrLevel *lds_lv, const uint2 *__restrict__ tables, const uint4 *anch,
                                                 const uint2 *lat, float u0, float u1, float u2, bool live, int g, s8v &xd, s8v &xc,
                                                 uint32_t fast_levels) {
    uint2 v[4][8];
    float w[4][8];
    if (live) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const NsrLevel lv = lds_lv[field_lane_level(g, i)];
            const bool fast = field_call_is_fast(fast_levels, i);
            uint32_t rows[8];
            if (field_call_is_fast(FWD_LAT_LEVELS, i)) {
                uint32_t c[3];
                field_level_cell(lv, u0, u1, u2, c, w[i]);
                const uint4 an = anch[field_lane_level(g, i)];
                const uint32_t S = lv.pad_ & 0xFu, d0 = c[0] - an.x, d1 = c[1] - an.y, d2 = c[2] - an.z;
                if (d0 < S - 1u && d1 < S - 1u && d2 < S - 1u) {
                    // an LDS-typed pointer: as generic loads the two branches are merged into one flat load per corner
                    const lds_row *p = (const lds_row *)(lat + (lv.pad_ >> 8) + __umul24(__umul24(d2, S) + d1, S) + d0);
                    const uint32_t S2 = __umul24(S, S), off[4] = {0u, S, S2, S2 + S};
#pragma unroll
                    for (int idx = 0; idx < 8; idx++) {
                        const u2v r = p[off[idx >> 1] + (idx & 1)];
                        v[i][idx] = make_uint2(r[0], r[1]);
                    }
                } else {
                    if (fast) field_cell_rows<true>(lv, c, rows);
                    else field_cell_rows<false>(lv, c, rows);
#pragma unroll
                    for (int idx = 0; idx < 8; idx++) v[i][idx] = tables[rows[idx]];
                }
            } else {
                if (fast) field_level_rows<true>(lv, u0, u1, u2, rows, w[i]);
                else field_level_rows<false>(lv, u0, u1, u2, rows, w[i]);
#pragma unroll
                for (int idx = 0; idx < 8; idx++) v[i][idx] = tables[rows[idx]];
            }
        }
    }
    field_mix_rows<CD>(v, w, live, xd, xc);
}

template <int CD, bool DIRS = false>
__global__ void __launch_bounds__(256)
k_field_fwd_lat(FieldArgsOf<DIRS> a, FieldLatArgs la) {
    const float *const dirs = field_dirs_of(a);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    short *wl = reinterpret_cast<short *>(smem);
    NsrLevel *lds_lv = reinterpret_cast<NsrLevel *>(smem + FW_IMAGE<DIRS> * 2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char *wbase = smem + FW_IMAGE<DIRS> * 2 + 16 * sizeof(NsrLevel) + (size_t)wave * la.wave_bytes;
    uint4 *anch = reinterpret_cast<uint4 *>(wbase);
    uint2 *lat = reinterpret_cast<uint2 *>(wbase + FWD_LAT_ANCHORS<DIRS> * sizeof(uint4));
    field_build_fw<CD, false, DIRS>(wl, a.params);
    if (threadIdx.x < 16) lds_lv[threadIdx.x] = a.lv[threadIdx.x];
    if (lane < FWD_LAT_ANCHORS<DIRS>) anch[lane] = make_uint4(LAT_NONE, LAT_NONE, LAT_NONE, 0u);
    __syncthreads();

    const uint32_t Mc = FIELD_COUNT(a);
    const uint32_t ntiles = (Mc + 15) / 16;
    const int s = lane & 15, g = lane >> 4;
    const uint2 *tables = reinterpret_cast<const uint2 *>(a.tables);
    const uint32_t lb = field_logical_block();
    const uint32_t tpb = (ntiles + gridDim.x - 1) / gridDim.x;
    const uint32_t t_begin = lb * tpb;
    const uint32_t t_end = min(t_begin + tpb, ntiles);
    const float kq = (float)(1 << LAT_KEY_BITS);
    uint32_t cur_key = LAT_NONE;                                      // wave-uniform: the block the lattices were anchored for

    for (uint32_t tile = t_begin + wave; tile < t_end; tile += 4) {
        const uint32_t mpos = tile * 16 + s;
        const bool valid = mpos < Mc;
        const uint32_t m = valid ? a.perm[mpos] : mpos;
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        if (valid) {
            u0 = field_unit(a.xyzs[(size_t)m * 3 + 0], a.bmin[0], a.bsize[0]);
            u1 = field_unit(a.xyzs[(size_t)m * 3 + 1], a.bmin[1], a.bsize[1]);
            u2 = field_unit(a.xyzs[(size_t)m * 3 + 2], a.bmin[2], a.bsize[2]);
        }
        const bool live = valid && field_in_unit_cube(u0, u1, u2);
        // the block of the tile's first live sample (k_order_keys' quantisation) anchors the lattices
        const unsigned long long lm = __ballot(live);
        if (lm) {
            const uint32_t bkey = (uint32_t)fminf(fmaxf(u0 * kq, 0.0f), kq - 1.0f) |
                                  ((uint32_t)fminf(fmaxf(u1 * kq, 0.0f), kq - 1.0f) << LAT_KEY_BITS) |
                                  ((uint32_t)fminf(fmaxf(u2 * kq, 0.0f), kq - 1.0f) << (2 * LAT_KEY_BITS));
            const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)bkey, (int)__builtin_ctzll(lm));
            if (cur_key == LAT_NONE || ((key ^ cur_key) & la.key_mask) != 0u) {
                cur_key = key;
                field_lat_refill<FWD_LAT_ANCHORS<DIRS>>(lds_lv, tables, anch, lat, key, lane);
            }
        }
        s8v xd, xc;
        field_encode_lat<CD>(lds_lv, tables, anch, lat, u0, u1, u2, live, g, xd, xc, a.fast_levels);
        if (a.feats) {
            s8v *fo = reinterpret_cast<s8v *>(a.feats) + ((size_t)tile * 64 + lane) * 2;
            fo[0] = xd;
            fo[1] = xc;
        }

        const f4v o = field_density_net<CD>(wl, lane, xd);
        if (valid && g == 0) a.sigmas[m] = expf(o[0]) * a.density_scale;   // tcnn_nerf.py:55-60, renderer.py:225

        f4v rgb, cls;
        if constexpr (DIRS) field_colour_nets<CD, true>(wl, lane, xc, rgb, cls, field_sh_frag<CD>(dirs, m, valid, g));
        else field_colour_nets<CD>(wl, lane, xc, rgb, cls);
        if (valid) field_store_channels(a, m, g, rgb, cls);
    }
}

// stand-alone SH encoding (the tcnn.Encoding stand-in of SHEncoder): out[m, 0..15], fp32, not rounded
__global__ void __launch_bounds__(256)
k_sh_encode(const float *__restrict__ dirs, uint32_t M, float *__restrict__ out) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < M * 4u; i += gridDim.x * 256u) {
        const uint32_t m = i >> 2;
        const f4v c = field_sh4((int)(i & 3u), dirs[(size_t)m * 3 + 0], dirs[(size_t)m * 3 + 1], dirs[(size_t)m * 3 + 2]);
        reinterpret_cast<float4 *>(out)[i] = make_float4(c[0], c[1], c[2], c[3]);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The lattice kernel's launch geometry for a level table, written into b.lv[].pad_ and la; returns its LDS bytes, or 0 where the
// walk keeps the gather (a grid the scatter's lattices do not fit, or one that needs more than a quarter of a CU's LDS).
template <bool DIRS>
static size_t field_lat_plan(NsrLevel (&lv)[16], FieldLatArgs &la) {
    if (!nsr_table_scatter_supported(lv)) return 0;
    // lattices of FWD_LAT_LEVELS, packed: pad_ = S | shift << 4 | first slot << 8 (the other levels' pad_ is not read)
    LatGeom geo;
    lat_geometry(lv, geo, 1024u);
    uint32_t slots = 0, min_shift = LAT_KEY_BITS;
    for (int l = 0; l < 16; l++) {
        if (!((FWD_LAT_LEVELS >> l) & 1u)) continue;
        lv[l].pad_ = (uint32_t)geo.S[l] | ((uint32_t)geo.shift[l] << 4) | (slots << 8);
        slots += (uint32_t)geo.S[l] * geo.S[l] * geo.S[l];
        if (geo.shift[l] < min_shift) min_shift = geo.shift[l];
    }
    const uint32_t axis = ((1u << LAT_KEY_BITS) - 1u) & ~((1u << min_shift) - 1u);
    la.key_mask = axis | (axis << LAT_KEY_BITS) | (axis << (2 * LAT_KEY_BITS));
    la.wave_bytes = FWD_LAT_ANCHORS<DIRS> * (uint32_t)sizeof(uint4) + ((slots * (uint32_t)sizeof(uint2) + 15u) & ~15u);
    const size_t lds = FW_IMAGE<DIRS> * 2 + 16 * sizeof(NsrLevel) + 4 * (size_t)la.wave_bytes;
    return lds <= 40960 ? lds : 0;      // four workgroups per CU, as k_field_fwd; a grid that needs more keeps the gather
}

template <typename TT, int CD, bool DIRS = false>
static int field_launch_fwd(const FieldArgs &a, uint32_t nblocks, bool sigma_only, hipStream_t s, const float *dirs = nullptr) {
    if (DIRS && sigma_only) return NSR_ERR_INVALID_ARG;      // the sigma-only branch has no direction-taking form
    if constexpr (sizeof(TT) == 2) {
        if (!sigma_only && a.perm) {
            FieldArgsOf<DIRS> b;
            static_cast<FieldArgs &>(b) = a;
            if constexpr (DIRS) b.dirs = dirs;
            FieldLatArgs la;
            const size_t lds = field_lat_plan<DIRS>(b.lv, la);
            if (lds) {
                hipLaunchKernelGGL((k_field_fwd_lat<CD, DIRS>), dim3(nblocks), dim3(256), lds, s, b, la);
                return nsr_launch_status();
            }
        }
    }
    if constexpr (DIRS) {
        const size_t lds = FW_TOTAL_DIRS * 2 + 16 * sizeof(NsrLevel);
        FieldDirsArgs b;
        static_cast<FieldArgs &>(b) = a;
        b.dirs = dirs;
        hipLaunchKernelGGL((k_field_fwd<TT, CD, false, true>), dim3(nblocks), dim3(256), lds, s, b);
    } else if (sigma_only) {
        const size_t lds = FW_SIGMA_TOTAL * 2 + 16 * sizeof(NsrLevel);
        hipLaunchKernelGGL((k_field_fwd<TT, CD, true>), dim3(nblocks), dim3(256), lds, s, a);
    } else {
        const size_t lds = FW_TOTAL * 2 + 16 * sizeof(NsrLevel);
        hipLaunchKernelGGL((k_field_fwd<TT, CD, false>), dim3(nblocks), dim3(256), lds, s, a);
    }
    return nsr_launch_status();
}

// the one launcher behind nsr_field_forward and nsr_field_forward_dirs (dirs != NULL: the direction-taking instantiations)
static int field_forward_any(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs, uint32_t M,
                             const int32_t *m_dev, float *sigmas, float *rgbs, void *feats, const uint32_t *perm, const float *dirs,
                             nsr_stream_t stream) {
    if (M == 0) return NSR_OK;
    NSR_CHECK_PTR(desc); NSR_CHECK_PTR(tables); NSR_CHECK_PTR(mlp_params); NSR_CHECK_PTR(xyzs); NSR_CHECK_PTR(sigmas);
    FieldArgs a;
    uint32_t nblocks;
    const int st = field_fill_args(desc, tables, mlp_params, a, M, nblocks);
    if (st != NSR_OK) return st;
    if (rgbs && a.C_ch == 8 && ((uintptr_t)rgbs & 15u)) return NSR_ERR_INVALID_ARG;
    if (feats && ((uintptr_t)feats & 15u)) return NSR_ERR_INVALID_ARG;
    a.xyzs = xyzs; a.m_dev = m_dev; a.sigmas = sigmas; a.rgbs = rgbs; a.feats = feats; a.perm = perm;
    const bool so = rgbs == nullptr;
    hipStream_t s = (hipStream_t)stream;
    return field_dispatch(desc->table_dtype, desc->compute_dtype, [&](auto tt, auto cd) {
        if (dirs) return field_launch_fwd<decltype(tt), cd(), true>(a, nblocks, false, s, dirs);
        return field_launch_fwd<decltype(tt), cd()>(a, nblocks, so, s);
    });
}

extern "C" {

int nsr_field_forward(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs, uint32_t M,
                      const int32_t *m_dev, float *sigmas, float *rgbs, void *feats, const uint32_t *perm, nsr_stream_t stream) {
    return field_forward_any(desc, tables, mlp_params, xyzs, M, m_dev, sigmas, rgbs, feats, perm, nullptr, stream);
}

uint32_t nsr_field_mlp_param_count(int with_dirs) { return with_dirs ? P_TOTAL_DIRS : P_TOTAL; }

int nsr_field_forward_uses_lattice(const nsr_field_desc *desc, int with_perm, int with_dirs) {
    if (desc == nullptr) return 0;
    FieldArgs a;
    uint32_t nblocks;
    if (field_fill_args(desc, nullptr, nullptr, a, 16, nblocks) != NSR_OK) return 0;
    if (!with_perm || desc->table_dtype != NSR_F16) return 0;
    FieldLatArgs la;
    return (with_dirs ? field_lat_plan<true>(a.lv, la) : field_lat_plan<false>(a.lv, la)) != 0;
}

int nsr_sh_encode(const float *dirs, uint32_t M, float *out, nsr_stream_t stream) {
    if (M == 0) return NSR_OK;
    NSR_CHECK_PTR(dirs); NSR_CHECK_PTR(out);
    if (((uintptr_t)out & 15u) || M > 0x3FFFFFFFu) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_sh_encode, dim3(nsr_grid_1d((uint64_t)M * 4, 256)), dim3(256), 0, (hipStream_t)stream, dirs, M, out);
    return nsr_launch_status();
}

int nsr_field_forward_dirs(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs, uint32_t M,
                           const int32_t *m_dev, float *sigmas, float *rgbs, void *feats, const uint32_t *perm, const float *dirs,
                           nsr_stream_t stream) {
    // the sigma-only branch never reads directions (nor the SH columns): it is nsr_field_forward's
    if (rgbs == nullptr) dirs = nullptr;
    else if (M != 0) NSR_CHECK_PTR(dirs);
    return field_forward_any(desc, tables, mlp_params, xyzs, M, m_dev, sigmas, rgbs, feats, perm, dirs, stream);
}

}   // extern "C"
