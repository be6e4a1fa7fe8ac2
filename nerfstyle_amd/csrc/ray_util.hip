// What is neither march nor composite: near/far against the AABB, morton codes, the occupancy bitfield, device ray
// generation, and the library's identity functions (ABI version, status strings, target).
#include "rm_probe.h"
#include "ray_pose.h"

// ---------------------------------------------------------------------------------------------
// utilities
// ---------------------------------------------------------------------------------------------
// raymarching.cu:190-244
__global__ void k_near_far_from_aabb(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                     const float *__restrict__ aabb, uint32_t N, float min_near,
                                     float *__restrict__ nears, float *__restrict__ fars) {
#pragma clang fp contract(off)
    const float a0 = aabb[0], a1 = aabb[1], a2 = aabb[2], a3 = aabb[3], a4 = aabb[4], a5 = aabb[5];
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        const RmRay r = rm_load_ray(rays_o, rays_d, n);
        const float big = 3.402823466e+38f;
        float near = (a0 - r.ox) * r.rdx, far = (a3 - r.ox) * r.rdx;
        if (near > far) { const float c = near; near = far; far = c; }
        float near_y = (a1 - r.oy) * r.rdy, far_y = (a4 - r.oy) * r.rdy;
        if (near_y > far_y) { const float c = near_y; near_y = far_y; far_y = c; }
        if (near > far_y || near_y > far) { nears[n] = big; fars[n] = big; continue; }
        if (near_y > near) near = near_y;
        if (far_y < far) far = far_y;
        float near_z = (a2 - r.oz) * r.rdz, far_z = (a5 - r.oz) * r.rdz;
        if (near_z > far_z) { const float c = near_z; near_z = far_z; far_z = c; }
        if (near > far_z || near_z > far) { nears[n] = big; fars[n] = big; continue; }
        if (near_z > near) near = near_z;
        if (far_z < far) far = far_z;
        if (near < min_near) near = min_near;
        nears[n] = near;
        fars[n] = far;
    }
}

// raymarching.cu:313-325
__global__ void k_morton3d(const int32_t *__restrict__ coords, uint32_t N, int32_t *__restrict__ indices) {
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x)
        indices[n] = (int32_t)rm_morton3d((uint32_t)coords[n * 3], (uint32_t)coords[n * 3 + 1],
                                          (uint32_t)coords[n * 3 + 2]);
}

// raymarching.cu:336-353
__global__ void k_morton3d_invert(const int32_t *__restrict__ indices, uint32_t N, int32_t *__restrict__ coords) {
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        const int32_t ind = indices[n];
        coords[n * 3 + 0] = (int32_t)rm_morton3d_invert((uint32_t)(ind >> 0));
        coords[n * 3 + 1] = (int32_t)rm_morton3d_invert((uint32_t)(ind >> 1));
        coords[n * 3 + 2] = (int32_t)rm_morton3d_invert((uint32_t)(ind >> 2));
    }
}

// raymarching.cu:366-388.  One thread per output byte, 8 floats in as two 16-byte loads.
__global__ void k_packbits(const float *__restrict__ grid, uint32_t N, float thresh, uint8_t *__restrict__ bitfield) {
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        const float4 a = reinterpret_cast<const float4 *>(grid)[(size_t)n * 2];
        const float4 b = reinterpret_cast<const float4 *>(grid)[(size_t)n * 2 + 1];
        uint32_t bits = 0;
        bits |= (a.x > thresh) ? 1u : 0u;
        bits |= (a.y > thresh) ? 2u : 0u;
        bits |= (a.z > thresh) ? 4u : 0u;
        bits |= (a.w > thresh) ? 8u : 0u;
        bits |= (b.x > thresh) ? 16u : 0u;
        bits |= (b.y > thresh) ? 32u : 0u;
        bits |= (b.z > thresh) ? 64u : 0u;
        bits |= (b.w > thresh) ? 128u : 0u;
        bitfield[n] = (uint8_t)bits;
    }
}

// ---------------------------------------------------------------------------------------------
// device ray generation (nerf_lib.py:69-142, common.py:139-147)
// ---------------------------------------------------------------------------------------------
__global__ void k_generate_rays(const float *__restrict__ pose, uint32_t w, uint32_t h, float fx, float fy, float cx,
                                float cy, int camera_flip, const int32_t *__restrict__ pix, uint32_t N,
                                float *__restrict__ rays_o, float *__restrict__ rays_d) {
    ru_generate_rays<uint32_t>(RuOnePose{pose, pix}, RuPinhole{fx, fy, cx, cy}, camera_flip, w, blockDim.x, N, rays_o, rays_d);
}

// Backward of k_generate_rays with respect to the pose: grad_pose[:, 3] = sum_n grad_o[n]; with c_n the pixel's camera-frame
// direction (after the flip), v_n = R c_n, d_n = v_n / |v_n|:  grad_R = sum_n ((I - d_n d_n^T) grad_d[n] / |v_n|) c_n^T.
// Twelve sums over the rays: every ray's term and the sums are formed in fp64 (a few dozen operations per ray against two
// 12-byte loads; the per-entry error is then the final rounding to fp32), block tree + a fixed-order one-block final pass over
// the block partials, as k_recon_loss: no atomics, no counter, every partial the final pass reads was written by this call.
// The per-ray term (ru_pose_term) is ray_pose.h's, the block sum fixed_sum.h's: sum k on thread k.
#define RU_MAX_BLOCKS 2048u

__global__ void __launch_bounds__(RU_BLOCK)
k_generate_rays_bwd(const float *__restrict__ pose, uint32_t w, float fx, float fy, float cx, float cy, int camera_flip,
                    const int32_t *__restrict__ pix, uint32_t N, const float *__restrict__ g_o, const float *__restrict__ g_d,
                    double *__restrict__ partials) {
    __shared__ double red[12][RU_BLOCK / 64];
    double R[3][3];
    ru_load_rotation(pose, R);
    const RuFlip<double> flip = ru_flip<double>(camera_flip);
    const RuPinhole cam{fx, fy, cx, cy};
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.0;
    for (uint32_t n = blockIdx.x * RU_BLOCK + threadIdx.x; n < N; n += gridDim.x * RU_BLOCK)
        ru_pose_term(R, flip, pix ? (uint32_t)pix[n] : n, w, cam, g_o, g_d, n, acc);
    nsr_block_sum_stage(acc, red);
    if (threadIdx.x < 12) partials[(size_t)blockIdx.x * 12 + threadIdx.x] = nsr_block_sum_col<RU_BLOCK / 64>(red[threadIdx.x]);
}

__global__ void __launch_bounds__(RU_BLOCK)
k_generate_rays_bwd_final(const double *__restrict__ partials, uint32_t nblocks, float *__restrict__ grad_pose) {
    __shared__ double red[12][RU_BLOCK / 64];
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += RU_BLOCK) {
#pragma unroll
        for (int k = 0; k < 12; k++) acc[k] += partials[(size_t)b * 12 + k];
    }
    nsr_block_sum_stage(acc, red);
    if (threadIdx.x < 12) grad_pose[threadIdx.x] = (float)nsr_block_sum_col<RU_BLOCK / 64>(red[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

const char *nsr_status_string(int status) {
    switch (status) {
        case NSR_OK: return "ok";
        case NSR_ERR_INVALID_ARG: return "invalid argument (null pointer, bad size or enum)";
        case NSR_ERR_UNSUPPORTED: return "unsupported configuration for the gfx950 kernels";
        case NSR_ERR_LAUNCH: return "HIP kernel launch failed";
        default: return "unknown status";
    }
}
int nsr_abi_version(void) { return 6; }
const char *nsr_target_arch(void) { return "gfx950"; }

int nsr_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb, uint32_t N, float min_near,
                           float *nears, float *fars, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(rays_o); NSR_CHECK_PTR(rays_d); NSR_CHECK_PTR(aabb); NSR_CHECK_PTR(nears); NSR_CHECK_PTR(fars);
    hipLaunchKernelGGL(k_near_far_from_aabb, dim3(nsr_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d,
                       aabb, N, min_near, nears, fars);
    return nsr_launch_status();
}

int nsr_morton3d(const int32_t *coords, uint32_t N, int32_t *indices, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(coords); NSR_CHECK_PTR(indices);
    hipLaunchKernelGGL(k_morton3d, dim3(nsr_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, coords, N, indices);
    return nsr_launch_status();
}

int nsr_morton3d_invert(const int32_t *indices, uint32_t N, int32_t *coords, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(coords); NSR_CHECK_PTR(indices);
    hipLaunchKernelGGL(k_morton3d_invert, dim3(nsr_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, indices, N, coords);
    return nsr_launch_status();
}

int nsr_packbits(const float *grid, uint32_t N, float density_thresh, uint8_t *bitfield, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(grid); NSR_CHECK_PTR(bitfield);
    if (((uintptr_t)grid & 15u) != 0) return NSR_ERR_INVALID_ARG;   // 16-byte loads
    hipLaunchKernelGGL(k_packbits, dim3(nsr_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, grid, N, density_thresh,
                       bitfield);
    return nsr_launch_status();
}

int nsr_generate_rays(const float *pose, uint32_t w, uint32_t h, float fx, float fy, float cx, float cy, int camera_flip,
                      const int32_t *pix, uint32_t N, float *rays_o, float *rays_d, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(pose); NSR_CHECK_PTR(rays_o); NSR_CHECK_PTR(rays_d);
    if (w == 0 || h == 0) return NSR_ERR_INVALID_ARG;
    if (pix == nullptr && (uint64_t)N != (uint64_t)w * h) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_generate_rays, dim3(nsr_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, pose, w, h, fx, fy, cx, cy,
                       camera_flip, pix, N, rays_o, rays_d);
    return nsr_launch_status();
}

uint64_t nsr_generate_rays_backward_workspace_bytes(uint32_t N) {
    (void)N;
    return (uint64_t)RU_MAX_BLOCKS * 12 * sizeof(double);
}

int nsr_generate_rays_backward(const float *pose, uint32_t w, uint32_t h, float fx, float fy, float cx, float cy, int camera_flip,
                               const int32_t *pix, uint32_t N, const float *grad_rays_o, const float *grad_rays_d, void *workspace,
                               float *grad_pose, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(pose); NSR_CHECK_PTR(grad_rays_o); NSR_CHECK_PTR(grad_rays_d); NSR_CHECK_PTR(workspace); NSR_CHECK_PTR(grad_pose);
    if (w == 0 || h == 0 || ((uintptr_t)workspace & 7u) != 0) return NSR_ERR_INVALID_ARG;
    if (pix == nullptr && (uint64_t)N != (uint64_t)w * h) return NSR_ERR_INVALID_ARG;
    uint32_t nb = nsr_div_up(N, RU_BLOCK);
    if (nb > RU_MAX_BLOCKS) nb = RU_MAX_BLOCKS;
    hipLaunchKernelGGL(k_generate_rays_bwd, dim3(nb), dim3(RU_BLOCK), 0, (hipStream_t)stream, pose, w, fx, fy, cx, cy, camera_flip, pix,
                       N, grad_rays_o, grad_rays_d, (double *)workspace);
    hipLaunchKernelGGL(k_generate_rays_bwd_final, dim3(1), dim3(RU_BLOCK), 0, (hipStream_t)stream, (const double *)workspace, nb, grad_pose);
    return nsr_launch_status();
}

}   // extern "C"

