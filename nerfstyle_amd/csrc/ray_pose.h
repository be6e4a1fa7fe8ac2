// Device ray generation and its backward towards the camera, shared by the single-pose kernels (ray_util.hip), the mixed-frame
// ones (frame_batch.hip) and the lens ones (lens.hip): one ray from a pose and a pixel id, the forward kernels' one body
// (ru_generate_rays), one ray's fp64 terms of the pose gradient (and of the lens gradient).  The sums over those terms are
// fixed_sum.h's and seg_sum.h's.
#pragma once
#include <type_traits>
#include "fixed_sum.h"

#define RU_BLOCK 256

// the signs of the camera flip (nerf_lib.py:121, bit order [2,1,0]), in the precision of the caller's arithmetic
template <typename T> struct RuFlip { T f0, f1, f2; };
template <typename T>
__host__ __device__ __forceinline__ RuFlip<T> ru_flip(int camera_flip) {
    return RuFlip<T>{(camera_flip >> 2) & 1 ? (T)-1 : (T)1, (camera_flip >> 1) & 1 ? (T)-1 : (T)1, (camera_flip >> 0) & 1 ? (T)-1 : (T)1};
}

struct RuPose { float r00, r01, r02, tx, r10, r11, r12, ty, r20, r21, r22, tz; };
__device__ __forceinline__ RuPose ru_load_pose(const float *__restrict__ pose) {
    return RuPose{pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], pose[6], pose[7], pose[8], pose[9], pose[10], pose[11]};
}

// row n from the camera-frame direction (d0, d1, d2): rotated by the pose and normalised (common.py:139-147)
template <typename Idx>
__device__ __forceinline__ void ru_write_dir(const RuPose &P, float d0, float d1, float d2, Idx n, float *__restrict__ rays_o,
                                             float *__restrict__ rays_d) {
#pragma clang fp contract(off)
    const float wx = P.r00 * d0 + P.r01 * d1 + P.r02 * d2;
    const float wy = P.r10 * d0 + P.r11 * d1 + P.r12 * d2;
    const float wz = P.r20 * d0 + P.r21 * d1 + P.r22 * d2;
    const float nrm = sqrtf(wx * wx + wy * wy + wz * wz);
    rays_d[n * 3 + 0] = wx / nrm; rays_d[n * 3 + 1] = wy / nrm; rays_d[n * 3 + 2] = wz / nrm;
    rays_o[n * 3 + 0] = P.tx; rays_o[n * 3 + 1] = P.ty; rays_o[n * 3 + 2] = P.tz;
}

// the two cameras of the forward kernels: pinhole values that came as kernel arguments, or the lens of include/nsr.h ("Lens
// refinement"), six f32 in device memory
struct RuPinhole { float fx, fy, cx, cy; };
struct RuLens { float fx, fy, cx, cy, k1, k2; };
__device__ __forceinline__ RuLens ru_load_lens(const float *__restrict__ lens) {
    return RuLens{lens[0], lens[1], lens[2], lens[3], lens[4], lens[5]};
}

// ray n of pixel id p (nerf_lib.py:114-122, common.py:139-147); f the camera flip's signs.  Idx: the caller's index type
// (k_generate_rays addresses its rows in 32 bits)
template <typename Idx>
__device__ __forceinline__ void ru_write_ray(const RuPose &P, const RuFlip<float> &f, uint32_t p, uint32_t w, const RuPinhole &C, Idx n,
                                             float *__restrict__ rays_o, float *__restrict__ rays_d) {
#pragma clang fp contract(off)
    const uint32_t py = p / w, px = p - py * w;
    // np.linspace(0, w, 2w+1)[1::2] == x + 0.5 exactly in fp32 for w < 2^22
    const float i = (float)px + 0.5f, j = (float)py + 0.5f;
    ru_write_dir(P, ((i - C.cx) / C.fx) * f.f0, ((j - C.cy) / C.fy) * f.f1, f.f2, n, rays_o, rays_d);
}

// ru_write_ray through the lens: the pinhole coordinates scaled by s = 1 + r2 (k1 + r2 k2).  With k1 = k2 = 0, s is exactly 1 and
// the row is ru_write_ray's bit for bit.
template <typename Idx>
__device__ __forceinline__ void ru_write_ray_lens(const RuPose &P, const RuFlip<float> &f, uint32_t p, uint32_t w, const RuLens &L, Idx n,
                                                  float *__restrict__ rays_o, float *__restrict__ rays_d) {
#pragma clang fp contract(off)
    const uint32_t py = p / w, px = p - py * w;
    const float i = (float)px + 0.5f, j = (float)py + 0.5f;
    const float x = (i - L.cx) / L.fx, y = (j - L.cy) / L.fy;
    const float r2 = x * x + y * y;
    const float s = 1.0f + r2 * (L.k1 + r2 * L.k2);
    ru_write_dir(P, (x * s) * f.f0, (y * s) * f.f1, f.f2, n, rays_o, rays_d);
}

// Where the rays of a forward launch take their pose and their pixel from: all from one pose (pix may be NULL: ray n is pixel
// n), or ray n from the pose of frame seg_frame[n / K] of F.
struct RuOnePose { const float *pose; const int32_t *pix; };
struct RuSegPoses { const float *poses; const int32_t *seg_frame, *pix; uint32_t F, K; };

// The body of the three forward kernels: a grid-stride loop over the N rays, each written by the writer of its camera
// (RuPinhole: ru_write_ray, RuLens: ru_write_ray_lens).  RuOnePose loads its pose once, before the loop; a ray of RuSegPoses
// whose segment names no frame in [0, F) becomes a NaN row, which the march treats as out of range.  block: the threads of
// the kernel's block (the kernel reads blockDim.x itself: inside a device function the compiler does not fold that read).
template <typename Idx, typename Frames, typename Cam>
__device__ __forceinline__ void ru_generate_rays(const Frames &fr, const Cam &cam, int camera_flip, uint32_t w, uint32_t block, uint32_t N,
                                                 float *__restrict__ rays_o, float *__restrict__ rays_d) {
    constexpr bool ONE = std::is_same_v<Frames, RuOnePose>;
    RuPose one{};
    if constexpr (ONE) one = ru_load_pose(fr.pose);
    const RuFlip<float> f = ru_flip<float>(camera_flip);
    const auto write = [&](const RuPose &P, uint32_t p, Idx n) {
        if constexpr (std::is_same_v<Cam, RuLens>) ru_write_ray_lens(P, f, p, w, cam, n, rays_o, rays_d);
        else ru_write_ray(P, f, p, w, cam, n, rays_o, rays_d);
    };
    for (uint32_t n = blockIdx.x * block + threadIdx.x; n < N; n += gridDim.x * block) {
        if constexpr (ONE) {
            write(one, fr.pix ? (uint32_t)fr.pix[n] : n, n);
        } else {
            const uint32_t frame = (uint32_t)fr.seg_frame[n / fr.K];
            if (frame >= fr.F) {
                const float nan = __int_as_float(0x7fc00000);
#pragma unroll
                for (int k = 0; k < 3; k++) { rays_o[(Idx)n * 3 + k] = nan; rays_d[(Idx)n * 3 + k] = nan; }
                continue;
            }
            write(ru_load_pose(fr.poses + (size_t)frame * 12), (uint32_t)fr.pix[n], n);
        }
    }
}

__device__ __forceinline__ void ru_load_rotation(const float *__restrict__ pose, double (&R)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[r][c] = (double)pose[r * 4 + c];
    }
}

// ray n's terms of the pose gradient for the camera-frame direction c (after the flip), added to acc[0..11] ([3][4] row-major):
// with v = R c, d = v / |v| and h = (I - d d^T) g_d[n] / |v|:  acc[:, :3] += h c^T,  acc[:, 3] += g_o[n]; all in fp64.  h is
// left for the caller (the gradient towards c is R^T h).
template <int NA>
__device__ __forceinline__ void ru_pose_term_dir(const double (&R)[3][3], const double (&c)[3], const float *__restrict__ g_o,
                                                 const float *__restrict__ g_d, size_t n, double (&acc)[NA], double (&h)[3]) {
    static_assert(NA >= 12, "twelve pose sums");
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
        h[r] = (gd[r] - d[r] * dg) * inv;
#pragma unroll
        for (int k = 0; k < 3; k++) acc[r * 4 + k] += h[r] * c[k];
        acc[r * 4 + 3] += (double)g_o[n * 3 + r];
    }
}

// ray n's terms of the pose gradient, added to acc [3][4] row-major: ru_pose_term_dir with the pinhole direction of pixel id p
__device__ __forceinline__ void ru_pose_term(const double (&R)[3][3], const RuFlip<double> &f, uint32_t p, uint32_t w, const RuPinhole &C,
                                             const float *__restrict__ g_o, const float *__restrict__ g_d, size_t n, double (&acc)[12]) {
    const uint32_t py = p / w, px = p - py * w;
    const double c[3] = {(((double)px + 0.5 - (double)C.cx) / (double)C.fx) * f.f0, (((double)py + 0.5 - (double)C.cy) / (double)C.fy) * f.f1,
                         f.f2};
    double h[3];
    ru_pose_term_dir(R, c, g_o, g_d, n, acc, h);
}

// ray n's eighteen terms through the lens L = (fx, fy, cx, cy, k1, k2): the twelve of ru_pose_term with the distorted direction
// in acc[0..11], and in acc[12..17] the gradient towards L in that order (include/nsr.h states the closed form); all in fp64
__device__ __forceinline__ void ru_lens_term(const double (&R)[3][3], const RuFlip<double> &f, uint32_t p, uint32_t w, const double (&L)[6],
                                             const float *__restrict__ g_o, const float *__restrict__ g_d, size_t n, double (&acc)[18]) {
    const uint32_t py = p / w, px = p - py * w;
    const double x = ((double)px + 0.5 - L[2]) / L[0], y = ((double)py + 0.5 - L[3]) / L[1];
    const double r2 = x * x + y * y;
    const double s = 1.0 + r2 * (L[4] + r2 * L[5]), ds = L[4] + 2.0 * L[5] * r2;
    const double c[3] = {(x * s) * f.f0, (y * s) * f.f1, f.f2};
    double h[3];
    ru_pose_term_dir(R, c, g_o, g_d, n, acc, h);
    const double gX = (R[0][0] * h[0] + R[1][0] * h[1] + R[2][0] * h[2]) * f.f0;
    const double gY = (R[0][1] * h[0] + R[1][1] * h[1] + R[2][1] * h[2]) * f.f1;
    const double m = gX * x + gY * y;
    const double gx = gX * s + 2.0 * m * ds * x, gy = gY * s + 2.0 * m * ds * y;
    acc[12] += -gx * x / L[0];
    acc[13] += -gy * y / L[1];
    acc[14] += -gx / L[0];
    acc[15] += -gy / L[1];
    acc[16] += m * r2;
    acc[17] += m * r2 * r2;
}

// the block of the mixed-frame and lens kernels (frame_batch.hip, lens.hip)
#define FB_BLOCK 256
