// Inference side of the ray march for gfx950: the reference-style march / composite loop kernels
// (raymarching.cu:1004-1231) with the alive-ray compaction between their iterations, and the single-pass composite
// over the training-style march's compacted samples.  The training composite lives in composite.hip.
#include "rm_probe.h"

#define RM_MAXC 16

// Single-pass inference composite: the arithmetic of kernel_composite_rays (raymarching.cu:1133-1231)
// -- T = 1 - weight_sum, stop test on T BEFORE the sample (:1206), absolute t starting at near --
// applied to the compacted [offset, offset+count) samples of the training-style march instead of
// up to 1024 host-driven march_rays / composite_rays iterations (renderer.py:266-285).
template <int LPR>
__global__ void __launch_bounds__(RM_BLOCK)
k_composite_infer(const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                  const int32_t *__restrict__ rays, const float *__restrict__ nears, uint32_t M, uint32_t N, uint32_t C,
                  float T_thresh, float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image) {
    const uint32_t tid = blockIdx.x * RM_BLOCK + threadIdx.x;
    const uint32_t n = tid / LPR, ch = tid % LPR;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num_steps = (uint32_t)rays[n * 3 + 2];
    const bool has_ch = ch < C;
    float acc = 0.0f, ws = 0.0f, d = 0.0f;
    if (!(num_steps == 0 || offset + num_steps >= M)) {
        float t_phy = nears[index];
        const float *s = sigmas + offset;
        const float *rgb = rgbs + (size_t)offset * C + (has_ch ? ch : 0);
        const float *dl = deltas + (size_t)offset * 4;
        for (uint32_t step = 0; step < num_steps; step++) {
            const float2 dd = *reinterpret_cast<const float2 *>(dl + step * 4);
            const float alpha = 1.0f - __expf(-s[step] * dd.x);
            const float T = 1 - ws;
            const float weight = alpha * T;
            ws += weight;
            t_phy += dd.y;
            d += weight * t_phy;
            if (has_ch) acc += weight * rgb[(size_t)step * C];
            if (T < T_thresh) break;   // :1206
        }
    }
    if (ch == 0) {
        weights_sum[index] = ws;
        depth[index] = d;
    }
    if (has_ch) image[(size_t)index * C + ch] = acc;
}

// ---------------------------------------------------------------------------------------------
// inference march / composite (raymarching.cu:1004-1120, 1133-1231)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RM_BLOCK)
k_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *__restrict__ rays_alive, const float *__restrict__ rays_t,
             const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ z_hats,
             float bound, float dt_gamma, uint32_t max_steps, int is_ndc, uint32_t C, uint32_t H,
             const uint8_t *__restrict__ grid, const float *__restrict__ fars, float *__restrict__ xyzs,
             float *__restrict__ dirs, float *__restrict__ deltas, const float *__restrict__ noises) {
    const uint32_t n = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (n >= n_alive) return;
    const int index = rays_alive[n];
    const RmCfg c = rm_cfg(bound, dt_gamma, max_steps, C, H, grid);
    const RmRay r = rm_load_ray(rays_o, rays_d, (uint32_t)index);
    float *pxyz = xyzs + (size_t)n * n_step * 3;
    float *pdir = dirs ? dirs + (size_t)n * n_step * 3 : nullptr;
    float *pdel = deltas + (size_t)n * n_step * 4;
    const float t_alive = rays_t[(size_t)index * (is_ndc ? 2 : 1)];
    const float far = fars[index];
    float t = rm_start_t(c, t_alive, noises ? noises[n] : 0.0f);   // :1053
    uint32_t step = 0;
    float last_t = t;
    float last_z;
    {
#pragma clang fp contract(off)
        last_z = rm_clamp(r.oz + t * r.dz, -bound, bound);     // (contracted to an fma it is not the oracle's float)
    }
    float x, y, z, dt, tt;
    while (t < far && step < n_step) {
        if (rm_probe(r, c, t, x, y, z, dt, tt)) {
#pragma clang fp contract(off)
            pxyz[0] = x; pxyz[1] = y; pxyz[2] = z;
            if (pdir) { pdir[0] = r.dx; pdir[1] = r.dy; pdir[2] = r.dz; pdir += 3; }
            t += dt;
            pdel[0] = dt;
            pdel[1] = t - last_t;
            if (is_ndc) {
                const float new_z = rm_clamp(r.oz + t * r.dz, -bound, bound);
                const float zh = z_hats[index];
                pdel[2] = (2 / (new_z - 1) - 2 / (z - 1)) / zh;
                pdel[3] = (2 / (new_z - 1) - 2 / (last_z - 1)) / zh;
                last_z = new_z;
            }
            last_t = t;
            pxyz += 3; pdel += 4;
            step++;
        } else {
            rm_skip(c, t, tt);
        }
    }
    // The reference relies on the caller zero-filling deltas (raymarching.py:409-412) so that an
    // unused tail reads delta == 0 (= "ray terminated", :1178).  Write the terminator here so the
    // caller does not have to memset [n_alive*n_step, 4] floats per iteration.
    for (; step < n_step; step++) {
        pdel[0] = 0.0f;
        pdel += 4;
    }
}

__global__ void __launch_bounds__(RM_BLOCK)
k_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *__restrict__ rays_alive,
                 float *__restrict__ rays_t, const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                 const float *__restrict__ deltas, uint32_t C, int is_ndc, float *__restrict__ weights_sum,
                 float *__restrict__ depth, float *__restrict__ image) {
    const uint32_t n = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (n >= n_alive) return;
    const int index = rays_alive[n];
    const float *s = sigmas + (size_t)n * n_step;
    const float *rgb = rgbs + (size_t)n * n_step * C;
    const float *dl = deltas + (size_t)n * n_step * 4;
    float *rt = rays_t + (size_t)index * (is_ndc ? 2 : 1);
    float *img = image + (size_t)index * C;
    float t_rm = 0.0f, t_phy;
    if (is_ndc) { t_rm = rt[0]; t_phy = rt[1]; } else { t_phy = rt[0]; }
    float weight_sum = weights_sum[index];
    float d = depth[index];
    float acc[RM_MAXC];
#pragma unroll
    for (int i = 0; i < RM_MAXC; i++) acc[i] = (uint32_t)i < C ? img[i] : 0.0f;
    uint32_t step = 0;
    while (step < n_step) {
        if (dl[0] == 0) break;   // :1178
        const float alpha = 1.0f - __expf(-s[0] * (is_ndc ? dl[2] : dl[0]));
        const float T = 1 - weight_sum;
        const float weight = alpha * T;
        weight_sum += weight;
        if (is_ndc) { t_rm += dl[1]; t_phy += dl[3]; } else { t_phy += dl[1]; }
        d += weight * t_phy;
#pragma unroll
        for (int i = 0; i < RM_MAXC; i++)
            if ((uint32_t)i < C) acc[i] += weight * rgb[i];
        if (T < T_thresh) break;   // :1206
        s++; rgb += C; dl += 4; step++;
    }
    if (step < n_step) {
        rays_alive[n] = -1;
    } else {
        if (is_ndc) { rt[0] = t_rm; rt[1] = t_phy; } else { rt[0] = t_phy; }
    }
    weights_sum[index] = weight_sum;
    depth[index] = d;
#pragma unroll
    for (int i = 0; i < RM_MAXC; i++)
        if ((uint32_t)i < C) img[i] = acc[i];
}

// ---------------------------------------------------------------------------------------------
// alive-ray compaction (replaces rays_alive[rays_alive >= 0], renderer.py:284)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RM_BLOCK)
k_alive_count(const int32_t *__restrict__ rays_alive, uint32_t n_alive, uint32_t *__restrict__ block_sums) {
    __shared__ uint32_t wave_sums[RM_BLOCK / 64];
    const uint32_t n = blockIdx.x * RM_BLOCK + threadIdx.x;
    const uint32_t keep = (n < n_alive && rays_alive[n] >= 0) ? 1u : 0u;
    // one ballot per wave instead of a shuffle scan: popcount of the 64-bit mask
    const unsigned long long mask = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) wave_sums[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < RM_BLOCK / 64; w++) t += wave_sums[w];
        block_sums[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(RM_BLOCK)
k_alive_write(const int32_t *__restrict__ rays_alive, uint32_t n_alive, const uint32_t *__restrict__ block_bases,
              int32_t *__restrict__ out) {
    __shared__ uint32_t wave_sums[RM_BLOCK / 64];
    const uint32_t n = blockIdx.x * RM_BLOCK + threadIdx.x;
    const int32_t v = n < n_alive ? rays_alive[n] : -1;
    const bool keep = v >= 0;
    const unsigned long long mask = __ballot(keep);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_sums[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t base = block_bases[blockIdx.x];
    for (uint32_t w = 0; w < wave; w++) base += wave_sums[w];
    if (keep) out[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = v;
}

__global__ void k_store_scan_total(const int32_t *__restrict__ counter2, int32_t *__restrict__ n_out) {
    n_out[0] = counter2[0];
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int nsr_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                   const float *rays_d, const float *z_hats, float bound, float dt_gamma, uint32_t max_steps, int is_ndc,
                   uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, float *xyzs,
                   float *dirs, float *deltas, const float *noises, nsr_stream_t stream) {
    if (n_alive == 0 || n_step == 0) return NSR_OK;
    NSR_CHECK_PTR(rays_alive); NSR_CHECK_PTR(rays_t); NSR_CHECK_PTR(rays_o); NSR_CHECK_PTR(rays_d); NSR_CHECK_PTR(grid);
    NSR_CHECK_PTR(fars); NSR_CHECK_PTR(xyzs); NSR_CHECK_PTR(deltas);
    (void)nears;
    if (is_ndc && z_hats == nullptr) return NSR_ERR_INVALID_ARG;
    if (max_steps == 0 || C == 0 || C > 8 || !rm_grid_size_ok(H)) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_march_rays, dim3(nsr_div_up(n_alive, RM_BLOCK)), dim3(RM_BLOCK), 0, (hipStream_t)stream, n_alive,
                       n_step, rays_alive, rays_t, rays_o, rays_d, z_hats, bound, dt_gamma, max_steps, is_ndc, C, H, grid, fars,
                       xyzs, dirs, deltas, noises);
    return nsr_launch_status();
}

int nsr_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t,
                       const float *sigmas, const float *rgbs, const float *deltas, uint32_t C, int is_ndc,
                       float *weights_sum, float *depth, float *image, nsr_stream_t stream) {
    if (n_alive == 0 || n_step == 0) return NSR_OK;
    NSR_CHECK_PTR(rays_alive); NSR_CHECK_PTR(rays_t); NSR_CHECK_PTR(sigmas); NSR_CHECK_PTR(rgbs); NSR_CHECK_PTR(deltas);
    NSR_CHECK_PTR(weights_sum); NSR_CHECK_PTR(depth); NSR_CHECK_PTR(image);
    if (C == 0 || C > RM_MAXC) return NSR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_composite_rays, dim3(nsr_div_up(n_alive, RM_BLOCK)), dim3(RM_BLOCK), 0, (hipStream_t)stream, n_alive,
                       n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, C, is_ndc, weights_sum, depth, image);
    return nsr_launch_status();
}

int nsr_composite_rays_infer(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, const float *nears,
                             uint32_t M, uint32_t N, uint32_t C, float T_thresh, float *weights_sum, float *depth, float *image,
                             nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(sigmas); NSR_CHECK_PTR(rgbs); NSR_CHECK_PTR(deltas); NSR_CHECK_PTR(rays); NSR_CHECK_PTR(nears);
    NSR_CHECK_PTR(weights_sum); NSR_CHECK_PTR(depth); NSR_CHECK_PTR(image);
    if (C == 0 || C > RM_MAXC) return NSR_ERR_UNSUPPORTED;
    if (((uintptr_t)deltas & 7u) != 0) return NSR_ERR_INVALID_ARG;
    hipStream_t hs = (hipStream_t)stream;
#define NSR_CI(LPR)                                                                                                 \
    hipLaunchKernelGGL((k_composite_infer<LPR>), dim3(nsr_div_up((uint64_t)N * LPR, RM_BLOCK)), dim3(RM_BLOCK), 0, hs, \
                       sigmas, rgbs, deltas, rays, nears, M, N, C, T_thresh, weights_sum, depth, image)
    if (C <= 4) NSR_CI(4); else if (C <= 8) NSR_CI(8); else NSR_CI(16);
#undef NSR_CI
    return nsr_launch_status();
}

uint64_t nsr_compact_alive_workspace_bytes(uint32_t n_alive) {
    const uint64_t nblocks = (n_alive + RM_BLOCK - 1) / RM_BLOCK;
    return (nblocks + 64) * sizeof(uint32_t);
}

int nsr_compact_alive(const int32_t *rays_alive, uint32_t n_alive, int32_t *out, int32_t *n_out, void *workspace,
                      nsr_stream_t stream) {
    NSR_CHECK_PTR(n_out);
    hipStream_t s = (hipStream_t)stream;
    if (n_alive == 0) {
        return hipMemsetAsync(n_out, 0, sizeof(int32_t), s) == hipSuccess ? NSR_OK : NSR_ERR_LAUNCH;
    }
    NSR_CHECK_PTR(rays_alive); NSR_CHECK_PTR(out); NSR_CHECK_PTR(workspace);
    const uint32_t nblocks = (n_alive + RM_BLOCK - 1) / RM_BLOCK;
    uint32_t *block_sums = (uint32_t *)workspace;
    int32_t *counter2 = (int32_t *)(block_sums + nblocks);   // scratch {total, unused}
    if (hipMemsetAsync(counter2, 0, 2 * sizeof(int32_t), s) != hipSuccess) return NSR_ERR_LAUNCH;
    hipLaunchKernelGGL(k_alive_count, dim3(nblocks), dim3(RM_BLOCK), 0, s, rays_alive, n_alive, block_sums);
    rm_scan_block_sums(block_sums, nblocks, counter2, 0u, s);
    hipLaunchKernelGGL(k_alive_write, dim3(nblocks), dim3(RM_BLOCK), 0, s, rays_alive, n_alive, block_sums, out);
    hipLaunchKernelGGL(k_store_scan_total, dim3(1), dim3(1), 0, s, counter2, n_out);
    return nsr_launch_status();
}

}   // extern "C"
