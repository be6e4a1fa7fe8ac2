// Density gradient of the fused field for gfx950, in FORWARD mode: sigma and d sigma / d position of every sample in one
// launch (normal maps: n = -grad sigma / |grad sigma|).  A translation unit of its own on the shared helpers of
// field_common.h / mfma_tiles.h, whose operation order is pinned (DESIGN.md "Shared encode helpers": tools/kernel_stats.py).
//
// Work decomposition: k_field_fwd's.  A wave owns 16 consecutive samples; lane (s = lane&15, g = lane>>4) encodes levels
// {2g, 2g+1, 8+2g, 9+2g} of sample s from the DENSITY half of the eight corner rows -- the value pair, with the weights and
// the summation order of field_encode_level, and its three partial derivatives with respect to the encoder input u
// (gridencoder.cu:196-227: per axis the four corner pairs, weight = product of the two other axes' weights).  That is four
// K=32 B fragments per lane: the value and one tangent per axis.
//
// Value chain: field_density_net, unchanged -> sigma is bit-identical to nsr_field_forward with rgbs == NULL.
// Tangent chains: dh_k = W1 * t_k, masked by h > 0 of the value chain, rounded to the compute type, dlogit_k = W2 * dh_k.
// The chain is linear in t_k: nothing is saved, there is no backward pass, no scatter and no atomic.
// The mask is taken from the fp32 accumulator h (the same MFMAs as the value chain), BEFORE mm_pack64 rounds it: ReLU's own
// derivative, which is what autograd through the rounding-emulating restatement (straight-through rounding) applies.  After
// the rounding a positive h below half the smallest f16 subnormal (2.98e-8) is zero; on a fresh checkpoint (tables +-1e-4,
// h of order 2e-5) that is several of the 64 x M hidden units per hundred samples, each of which would drop a full-sized
// term: measured rel-L2 2.3e-2 against the 5e-3 bar with the mask after the rounding (DESIGN.md "Position gradients").
//
// f16 range of the tangents.  d feature / du = res_l * (row difference): 16 .. 4096 times a difference that is 1e-4 on a
// fresh table and of order 1 on a trained one.  No fixed power-of-two prescale serves both.  The tangents are therefore
// carried in CELL units (without res_l: they have the magnitude of the features, which the value chain already carries in
// the same type) and the factor goes into the weights: a second LDS image of W1 whose column of level l is multiplied by
// res_l / res_15 (<= 1, >= 2^-8 here; built once per workgroup), and res_15 comes back in fp32 at the end.  bf16 would not
// need it and takes the same path.
//
// Output: grad_x sigma_k = density_scale * exp(clamp(logit, -15, 15)) * dlogit_k * du_k/dx_k with du_k/dx_k =
// 1 / (2 * bbox_size[k]) (field_unit) -- the trunc_exp rule of the backward (tcnn_nerf.py:62-66).  normalize: the unit normal
// -grad / |grad| for every gradient with finite components; a zero gradient gives a zero vector.  Samples whose encoder input
// is outside [0,1] or NaN get sigma as the forward gives it and a zero gradient; slots at or past *m_dev keep their sigma and get a zero gradient.
#include "field_common.h"

constexpr int DG_W1C = FW_SIGMA_TOTAL;              // W1 with res_l / res_15 in its columns: four frag32 (shorts)
constexpr int DG_TOTAL = FW_SIGMA_TOTAL + 2048;

struct DensityGradArgs {
    FieldArgs f;
    float *grads;             // [M,3]
    int normalize;
    float out_scale[3];       // res_15 * du_k/dx_k
    float cell_scale[16];     // res_l / res_15
};

// mm_build_frags' frag32 image of the 64 x 32 first layer, column k (feature k of level k >> 1) times cell_scale[k >> 1]
template <int CD>
__device__ __forceinline__ void dg_build_w1_cells(short *lds, const float *__restrict__ W, const float (&cell_scale)[16]) {
    for (int idx = threadIdx.x; idx < 2048; idx += blockDim.x) {
        const int e = idx & 7, lane = (idx >> 3) & 63, m = idx >> 9;
        const int g = lane >> 4, r = lane & 15;
        const int k = 16 * (e >> 2) + 4 * g + (e & 3);
        lds[idx] = MM<CD>::cvt(W[(16 * m + r) * 32 + k] * cell_scale[k >> 1]);
    }
}

// One level: the density feature pair (field_encode_level's SIGMA_ONLY sum, term for term) and its three partials in cell
// units.  Restates field_level_front (it also needs wx and wy alone) and, on two channels with pre-multiplied pair weights and
// no scale, the partials of k_grid_input_bwd (gridenc.hip): moving either changes this kernel's instruction count.  Corner idx: bit 0 = x, bit 1 = y, bit 2 = z.
template <typename TT, bool FAST>
__device__ __forceinline__ void dg_encode_level(const NsrLevel &lv, const TT *__restrict__ tables, float u0, float u1, float u2,
                                                bool live, float2 &val, float2 (&tan)[3]) {
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 3; k++) tan[k] = make_float2(0.f, 0.f);
    if (live) {
        float f[3];
        uint32_t c[3];
        nsr_grid_locate(u0, lv.resolution, 1, f[0], c[0]);
        nsr_grid_locate(u1, lv.resolution, 1, f[1], c[1]);
        nsr_grid_locate(u2, lv.resolution, 1, f[2], c[2]);
        const float wx[2] = {1 - f[0], f[0]}, wy[2] = {1 - f[1], f[1]}, wz[2] = {1 - f[2], f[2]};
        // (wx*wy)*wz: the reference's product order (gridencoder.cu:160-175)
        const float wxy[4] = {wx[0] * wy[0], wx[1] * wy[0], wx[0] * wy[1], wx[1] * wy[1]};
        uint32_t rows[8];
        field_cell_rows<FAST>(lv, c, rows);
        float2 v[8];
#pragma unroll
        for (int idx = 0; idx < 8; idx++) v[idx] = RowLd<TT>::dens(tables, rows[idx]);
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const float w = wxy[idx & 3] * wz[idx >> 2];
            acc.x += w * v[idx].x; acc.y += w * v[idx].y;
        }
        // gridencoder.cu:196-227 without `scale`: pair j, bit 0 = the first of the two other axes
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int b0 = j & 1, b1 = j >> 1;
            const float wa = wy[b0] * wz[b1], wb = wx[b0] * wz[b1], wc = wx[b0] * wy[b1];
            const int la = 2 * b0 + 4 * b1, lb = b0 + 4 * b1, lc = b0 + 2 * b1;
            tan[0].x += wa * (v[la + 1].x - v[la].x); tan[0].y += wa * (v[la + 1].y - v[la].y);
            tan[1].x += wb * (v[lb + 2].x - v[lb].x); tan[1].y += wb * (v[lb + 2].y - v[lb].y);
            tan[2].x += wc * (v[lc + 4].x - v[lc].x); tan[2].y += wc * (v[lc + 4].y - v[lc].y);
        }
    }
    val = acc;
}

// This lane's four levels -> the value B fragment and the three tangent B fragments (field_encode's element order)
template <typename TT, int CD>
__device__ __forceinline__ void dg_encode(const NsrLevel *lds_lv, const TT *__restrict__ tables, float u0, float u1, float u2,
                                          bool live, int g, s8v &xd, s8v (&td)[3], uint32_t fast_levels) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const NsrLevel lv = lds_lv[field_lane_level(g, i)];
        float2 val, tan[3];
        if (field_call_is_fast(fast_levels, i)) dg_encode_level<TT, true>(lv, tables, u0, u1, u2, live, val, tan);
        else dg_encode_level<TT, false>(lv, tables, u0, u1, u2, live, val, tan);
        xd[2 * i + 0] = MM<CD>::cvt(val.x);
        xd[2 * i + 1] = MM<CD>::cvt(val.y);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            td[k][2 * i + 0] = MM<CD>::cvt(tan[k].x);
            td[k][2 * i + 1] = MM<CD>::cvt(tan[k].y);
        }
    }
}

// tangent of the hidden layer -> B fragments of the second layer (mm_pack64's order): zero where the value chain's
// pre-activation is not > 0
template <int CD>
__device__ __forceinline__ void dg_mask_pack(const f4v (&dh)[4], const f4v (&h)[4], s8v (&out)[2]) {
    s4v r[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
#pragma unroll
        for (int e = 0; e < 4; e++) r[m][e] = MM<CD>::cvt(h[m][e] > 0.0f ? dh[m][e] : 0.0f);
    }
    out[0] = mm_cat(r[0], r[1]);
    out[1] = mm_cat(r[2], r[3]);
}

template <typename TT, int CD>
__global__ void __launch_bounds__(256)
k_field_density_grad(DensityGradArgs da) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FieldArgs &a = da.f;
    short *wl = reinterpret_cast<short *>(smem);
    NsrLevel *lds_lv = reinterpret_cast<NsrLevel *>(smem + DG_TOTAL * 2);
    field_build_fw<CD, true>(wl, a.params);
    dg_build_w1_cells<CD>(wl + DG_W1C, a.params + P_D1, da.cell_scale);
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

    for (uint32_t tile = t_begin + wave; tile < t_end; tile += 4) {
        const uint32_t m = tile * 16 + s;
        const bool valid = m < Mc;
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        if (valid) {
            u0 = field_unit(a.xyzs[(size_t)m * 3 + 0], a.bmin[0], a.bsize[0]);
            u1 = field_unit(a.xyzs[(size_t)m * 3 + 1], a.bmin[1], a.bsize[1]);
            u2 = field_unit(a.xyzs[(size_t)m * 3 + 2], a.bmin[2], a.bsize[2]);
        }
        const bool live = valid && field_in_unit_cube(u0, u1, u2);
        s8v xd, td[3];
        dg_encode<TT, CD>(lds_lv, tables, u0, u1, u2, live, g, xd, td, a.fast_levels);

        const f4v o = field_density_net<CD>(wl, lane, xd);
        // the value chain's hidden pre-activations once more (the same MFMAs as inside field_density_net): the mask
        f4v h[4];
        {
            const s8v b1[1] = {xd};
            mm_layer32<CD, 4, 1>(wl + FW_D1, lane, b1, h);
        }
        float dl[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            f4v dh[4], ok[1];
            s8v dhb[2];
            const s8v b1[1] = {td[k]};
            mm_layer32<CD, 4, 1>(wl + DG_W1C, lane, b1, dh);
            dg_mask_pack<CD>(dh, h, dhb);
            mm_layer32<CD, 1, 2>(wl + FW_D2, lane, dhb, ok);
            dl[k] = ok[0][0];
        }
        if (valid && g == 0) {
            if (a.sigmas) a.sigmas[m] = expf(o[0]) * a.density_scale;   // k_field_fwd's expression
            float gx = 0.f, gy = 0.f, gz = 0.f;
            if (live) {
                const float ds = a.density_scale * expf(fminf(fmaxf(o[0], -15.0f), 15.0f));
                gx = ds * (dl[0] * da.out_scale[0]);
                gy = ds * (dl[1] * da.out_scale[1]);
                gz = ds * (dl[2] * da.out_scale[2]);
                if (da.normalize) {
                    // |grad| through the largest component: no overflow or underflow of the squares
                    const float big = fmaxf(fmaxf(fabsf(gx), fabsf(gy)), fabsf(gz));
                    if (big > 0.f) {
                        const float rx = gx / big, ry = gy / big, rz = gz / big;
                        const float len = sqrtf(rx * rx + ry * ry + rz * rz);   // of the rescaled vector: in [1, sqrt 3]
                        const float norm = big * len;                           // |grad|: inf above FLT_MAX
                        if (norm >= 1e-20f && norm <= 3.402823466e+38f) {
                            const float inv = -1.0f / norm;
                            gx *= inv; gy *= inv; gz *= inv;
                        } else {
                            // a gradient below 1e-20 (a tiny density_scale) is still a direction, and so is one whose
                            // components are finite while its length is not: 1 / |grad| would overflow or vanish
                            const float inv = -1.0f / len;
                            gx = rx * inv; gy = ry * inv; gz = rz * inv;
                        }
                    } else {
                        gx = gy = gz = 0.f;                             // also turns -0 into +0
                    }
                }
            }
            float *dst = da.grads + (size_t)m * 3;
            dst[0] = gx; dst[1] = gy; dst[2] = gz;
        }
    }
    // slots at or past the device-side count: zero gradient (their sigma stays untouched, as in the forward)
    const size_t n_end = (size_t)a.M * 3, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)Mc * 3 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_end; i += stride) da.grads[i] = 0.f;
}

template <typename TT, int CD>
static int dg_launch(const DensityGradArgs &da, uint32_t nblocks, hipStream_t s) {
    const size_t lds = DG_TOTAL * 2 + 16 * sizeof(NsrLevel);
    hipLaunchKernelGGL((k_field_density_grad<TT, CD>), dim3(nblocks), dim3(256), lds, s, da);
    return nsr_launch_status();
}

extern "C" {

int nsr_field_density_gradient(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *xyzs,
                               uint32_t M, const int32_t *m_dev, float *sigmas, float *grads, int normalize, nsr_stream_t stream) {
    if (M == 0) return NSR_OK;
    NSR_CHECK_PTR(desc); NSR_CHECK_PTR(tables); NSR_CHECK_PTR(mlp_params); NSR_CHECK_PTR(xyzs); NSR_CHECK_PTR(grads);
    DensityGradArgs da;
    uint32_t nblocks;
    const int st = field_fill_args(desc, tables, mlp_params, da.f, M, nblocks);
    if (st != NSR_OK) return st;
    FieldArgs &a = da.f;
    a.xyzs = xyzs; a.m_dev = m_dev; a.sigmas = sigmas; a.rgbs = nullptr;
    a.feats = nullptr; a.perm = nullptr;
    da.grads = grads;
    da.normalize = normalize;
    const float res_top = (float)a.lv[15].resolution;
    for (int l = 0; l < 16; l++) da.cell_scale[l] = (float)a.lv[l].resolution / res_top;
    for (int k = 0; k < 3; k++) da.out_scale[k] = res_top * (1.0f / (2.0f * desc->bbox_size[k]));
    hipStream_t s = (hipStream_t)stream;
    return field_dispatch(desc->table_dtype, desc->compute_dtype,
                          [&](auto tt, auto cd) { return dg_launch<decltype(tt), cd()>(da, nblocks, s); });
}

}   // extern "C"
