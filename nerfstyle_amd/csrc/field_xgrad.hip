// Position gradient of the fused field for gfx950: d loss / d xyz of every sample from the encoder-output gradients that the
// ordered backward leaves in its workspace (nsr_field_backward with perm: [M][16] float4 = (density f0, density f1, colour f0,
// colour f1) per sample slot and level, field_bwd_gout.hip), contracted with the spatial partials of the trilinear interpolation.
// A translation unit of its own on the shared helpers of field_common.h, whose operation order is pinned (DESIGN.md "Shared
// encode helpers").  No MLP, no LDS beyond the level table, no atomics.
//
// Work decomposition: k_field_fwd's.  A wave owns 16 samples (16 consecutive slots, or 16 consecutive entries of perm: the
// gathers then hit in L2 as the forward's do); lane (s = lane&15, g = lane>>4) owns levels {2g, 2g+1, 8+2g, 9+2g} of sample s.
// Per level: the eight corner rows (one 8 B / 16 B row serves both encoders; all 32 gathers of the lane are issued before the
// first is used), per corner the dot product of the row with the level's float4, per axis the four signed corner-pair sums
// weighted by resolution * the two other axes' weights -- k_grid_input_bwd's arithmetic (gridenc.hip) on both encoders at
// once, in fp32.  Levels add up in ascending order: inside a lane (2g, then 2g+1), then the eight lane partials of a sample
// lo_0 .. lo_3, hi_0 .. hi_3 through cross-lane reads, in that order on every lane: two calls, and a call with and without
// perm, give the same bits per sample.
//
// Output: grad_xyzs[m, k] = sum * du_k/dx_k with du_k/dx_k = 1 / (2 * bbox_size[k]) (field_unit: BBox.normalize, then
// (x + 1) / 2).  A sample whose position is NaN or encodes outside [0,1] gets zeros, and so does every slot at or past *m_dev;
// the kernel tests both itself and never reads enc_grad there (slots past the count hold stale bytes).
#include "field_common.h"

struct XGradArgs {
    FieldArgs f;
    const float4 *enc_grad;   // [M][16]
    float *grads;             // [M,3]
    float out_scale[3];       // du_k/dx_k
};

template <typename TT> struct XgRow { typedef float4 raw; };
template <> struct XgRow<_Float16> { typedef h4v raw; };

__device__ __forceinline__ float xg_dot(const float4 &v, const float4 &e) { return ((v.x * e.x + v.y * e.y) + v.z * e.z) + v.w * e.w; }
__device__ __forceinline__ float xg_dot(const h4v &v, const float4 &e) {
    return (((float)v[0] * e.x + (float)v[1] * e.y) + (float)v[2] * e.z) + (float)v[3] * e.w;
}

template <typename TT>
__global__ void __launch_bounds__(256)
k_field_xgrad(XGradArgs xa) {
    typedef typename XgRow<TT>::raw Raw;
    __shared__ NsrLevel lds_lv[16];
    const FieldArgs &a = xa.f;
    if (threadIdx.x < 16) lds_lv[threadIdx.x] = a.lv[threadIdx.x];
    __syncthreads();

    const uint32_t Mc = FIELD_COUNT(a);
    const uint32_t ntiles = (Mc + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const Raw *tables = reinterpret_cast<const Raw *>(a.tables);
    const uint32_t lb = field_logical_block();
    const uint32_t tpb = (ntiles + gridDim.x - 1) / gridDim.x;
    const uint32_t t_begin = lb * tpb;
    const uint32_t t_end = min(t_begin + tpb, ntiles);

    for (uint32_t tile = t_begin + wave; tile < t_end; tile += 4) {
        const uint32_t j = tile * 16 + s;
        uint32_t m = j;
        bool valid = j < Mc;
        if (valid && a.perm) m = a.perm[j];
        valid = valid && m < Mc;                 // an entry of perm that names a slot past the count: the zero tail's
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        if (valid) {
            u0 = field_unit(a.xyzs[(size_t)m * 3 + 0], a.bmin[0], a.bsize[0]);
            u1 = field_unit(a.xyzs[(size_t)m * 3 + 1], a.bmin[1], a.bsize[1]);
            u2 = field_unit(a.xyzs[(size_t)m * 3 + 2], a.bmin[2], a.bsize[2]);
        }
        const bool live = valid && field_in_unit_cube(u0, u1, u2);     // outside: no gradient
        float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};      // levels 2g, 2g+1 and 8+2g, 9+2g
        if (live) {
            Raw v[4][8];
            float f[4][3], scale[4];
            float4 eg[4];
            const float4 *ep = xa.enc_grad + (size_t)m * 16;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const NsrLevel lv = lds_lv[field_lane_level(g, i)];
                uint32_t c[3], rows[8];
                nsr_grid_locate(u0, lv.resolution, 1, f[i][0], c[0]);
                nsr_grid_locate(u1, lv.resolution, 1, f[i][1], c[1]);
                nsr_grid_locate(u2, lv.resolution, 1, f[i][2], c[2]);
                scale[i] = (float)lv.resolution;
                if (field_call_is_fast(a.fast_levels, i)) field_cell_rows<true>(lv, c, rows);
                else field_cell_rows<false>(lv, c, rows);
#pragma unroll
                for (int idx = 0; idx < 8; idx++) v[i][idx] = tables[rows[idx]];
                eg[i] = ep[field_lane_level(g, i)];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                // sum over the four channels of grad * row, per corner (idx bit d = the upper corner on axis d)
                float gv[8];
#pragma unroll
                for (int idx = 0; idx < 8; idx++) gv[idx] = xg_dot(v[i][idx], eg[i]);
#pragma unroll
                for (int gd = 0; gd < 3; gd++) {
                    const int d0 = gd == 0 ? 1 : 0, d1 = gd == 2 ? 1 : 2;       // the two other axes, ascending
                    float r = 0.0f;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int b0 = q & 1, b1 = q >> 1;
                        float w = scale[i];
                        w *= b0 ? f[i][d0] : 1 - f[i][d0];
                        w *= b1 ? f[i][d1] : 1 - f[i][d1];
                        const int left = (b0 << d0) | (b1 << d1);
                        r += w * (gv[left | (1 << gd)] - gv[left]);
                    }
                    if (i < 2) lo[gd] += r; else hi[gd] += r;
                }
            }
        }
        // the sample's eight partials in ascending level order, the same sequence on each of its four lanes
        float out[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float acc = __shfl(lo[k], s, 64);
#pragma unroll
            for (int q = 1; q < 4; q++) acc += __shfl(lo[k], s + 16 * q, 64);
#pragma unroll
            for (int q = 0; q < 4; q++) acc += __shfl(hi[k], s + 16 * q, 64);
            out[k] = acc * xa.out_scale[k];
        }
        if (valid && g == 0) {
            float *dst = xa.grads + (size_t)m * 3;
            dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
        }
    }
    // slots at or past the device-side count: zero gradient
    const size_t n_end = (size_t)a.M * 3, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)Mc * 3 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_end; i += stride) xa.grads[i] = 0.f;
}

extern "C" {

int nsr_field_position_gradient(const nsr_field_desc *desc, const void *tables, const float *xyzs, uint32_t M, const int32_t *m_dev,
                                const void *enc_grad, const uint32_t *perm, float *grad_xyzs, nsr_stream_t stream) {
    if (M == 0) return NSR_OK;
    NSR_CHECK_PTR(desc); NSR_CHECK_PTR(tables); NSR_CHECK_PTR(xyzs); NSR_CHECK_PTR(enc_grad); NSR_CHECK_PTR(grad_xyzs);
    if (((uintptr_t)enc_grad & 15u) != 0) return NSR_ERR_INVALID_ARG;
    XGradArgs xa;
    uint32_t nblocks;
    const int st = field_fill_args(desc, tables, nullptr, xa.f, M, nblocks);
    if (st != NSR_OK) return st;
    FieldArgs &a = xa.f;
    a.xyzs = xyzs; a.m_dev = m_dev; a.sigmas = nullptr; a.rgbs = nullptr; a.feats = nullptr; a.perm = perm;
    xa.enc_grad = reinterpret_cast<const float4 *>(enc_grad);
    xa.grads = grad_xyzs;
    for (int k = 0; k < 3; k++) xa.out_scale[k] = 1.0f / (2.0f * desc->bbox_size[k]);
    hipStream_t s = (hipStream_t)stream;
    if (desc->table_dtype == NSR_F32) hipLaunchKernelGGL((k_field_xgrad<float>), dim3(nblocks), dim3(256), 0, s, xa);
    else if (desc->table_dtype == NSR_F16) hipLaunchKernelGGL((k_field_xgrad<_Float16>), dim3(nblocks), dim3(256), 0, s, xa);
    else return NSR_ERR_UNSUPPORTED;
    return nsr_launch_status();
}

}   // extern "C"
