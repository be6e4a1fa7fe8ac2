// Per-ray arithmetic of device ray generation and of its backward towards the pose, shared by the single-pose kernels
// (ray_util.hip) and the mixed-frame ones (frame_batch.hip): one ray from a pose and a pixel id, one ray's twelve fp64 terms of
// the pose gradient, and the fixed-order block tree over twelve sums.
#pragma once
#include "nsr_common.h"

#define RU_BLOCK 256

struct RuPose { float r00, r01, r02, tx, r10, r11, r12, ty, r20, r21, r22, tz; };
__device__ __forceinline__ RuPose ru_load_pose(const float *__restrict__ pose) {
    return RuPose{pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], pose[6], pose[7], pose[8], pose[9], pose[10], pose[11]};
}

// ray n of pixel id p (nerf_lib.py:114-122, common.py:139-147); f0..f2 the camera flip's signs.  Idx: the caller's index type
// (k_generate_rays addresses its rows in 32 bits)
template <typename Idx>
__device__ __forceinline__ void ru_write_ray(const RuPose &P, float f0, float f1, float f2, uint32_t p, uint32_t w, float fx, float fy,
                                             float cx, float cy, Idx n, float *__restrict__ rays_o, float *__restrict__ rays_d) {
#pragma clang fp contract(off)
    const uint32_t py = p / w, px = p - py * w;
    // np.linspace(0, w, 2w+1)[1::2] == x + 0.5 exactly in fp32 for w < 2^22
    const float i = (float)px + 0.5f, j = (float)py + 0.5f;
    const float d0 = ((i - cx) / fx) * f0, d1 = ((j - cy) / fy) * f1, d2 = f2;
    const float wx = P.r00 * d0 + P.r01 * d1 + P.r02 * d2;
    const float wy = P.r10 * d0 + P.r11 * d1 + P.r12 * d2;
    const float wz = P.r20 * d0 + P.r21 * d1 + P.r22 * d2;
    const float nrm = sqrtf(wx * wx + wy * wy + wz * wz);
    rays_d[n * 3 + 0] = wx / nrm; rays_d[n * 3 + 1] = wy / nrm; rays_d[n * 3 + 2] = wz / nrm;
    rays_o[n * 3 + 0] = P.tx; rays_o[n * 3 + 1] = P.ty; rays_o[n * 3 + 2] = P.tz;
}

__device__ __forceinline__ void ru_load_rotation(const float *__restrict__ pose, double (&R)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[r][c] = (double)pose[r * 4 + c];
    }
}

// ray n's terms of the pose gradient, added to acc [3][4] row-major: with c the pixel's camera-frame direction (after the flip),
// v = R c, d = v / |v|:  acc[:, :3] += ((I - d d^T) g_d[n] / |v|) c^T,  acc[:, 3] += g_o[n]; all in fp64
__device__ __forceinline__ void ru_pose_term(const double (&R)[3][3], double f0, double f1, double f2, uint32_t p, uint32_t w, float fx,
                                             float fy, float cx, float cy, const float *__restrict__ g_o, const float *__restrict__ g_d,
                                             size_t n, double (&acc)[12]) {
    const uint32_t py = p / w, px = p - py * w;
    const double c[3] = {(((double)px + 0.5 - (double)cx) / (double)fx) * f0, (((double)py + 0.5 - (double)cy) / (double)fy) * f1, f2};
    double v[3], gd[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        v[r] = R[r][0] * c[0] + R[r][1] * c[1] + R[r][2] * c[2];
        gd[r] = (double)g_d[n * 3 + r];
    }
    const double inv = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double d[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
    const double dg = d[0] * gd[0] + d[1] * gd[1] + d[2] * gd[2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double h = (gd[r] - d[r] * dg) * inv;
#pragma unroll
        for (int k = 0; k < 3; k++) acc[r * 4 + k] += h * c[k];
        acc[r * 4 + 3] += (double)g_o[n * 3 + r];
    }
}

// fixed-order block tree over twelve values: threads 0..11 leave with the block's sum k in v[0]
__device__ __forceinline__ void ru_block_sum12(double (&v)[12]) {
    __shared__ double red[12][RU_BLOCK / 64];
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 12; k++) v[k] += __shfl_xor(v[k], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double s = 0.0;
        for (int w = 0; w < RU_BLOCK / 64; w++) s += red[threadIdx.x][w];
        v[0] = s;
    }
}
