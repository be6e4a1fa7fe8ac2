// Mixed-frame ray batches: the rays of many cameras in one training step.  A batch is S segments of K rays, ray n belongs to
// segment n / K, segment s names one frame seg_frame[s] in [0, F) (frames may repeat).  S, K and F are host integers; seg_frame
// and the pixel ids live on the device, so a captured graph replays with fresh contents.
//     k_draw_frame_batch            (frame, pixel) pairs and their target rows from the counter-based RNG of the occupancy update
//     k_generate_rays_frames        k_generate_rays with the pose of the ray's segment
//     k_frames_bwd_*                its backward: one [3,4] sum per frame, deterministic
#include "philox.h"
#include "ray_pose.h"
#include "seg_sum.h"

static_assert(FB_BLOCK == SEG_BLOCK, "seg_blocks counts blocks of SEG_BLOCK threads");

// ---------------------------------------------------------------------------------------------
// the draw: uniform with replacement
// ---------------------------------------------------------------------------------------------
// Thread per ray.  The segment's frame is drawn again by each of its rays (ten rounds of integer multiplies) instead of being
// handed over through memory; the segment's first ray stores it.
__global__ void __launch_bounds__(FB_BLOCK)
k_draw_frame_batch(uint32_t F, uint32_t P, uint32_t K, uint32_t N, uint32_t seed_lo, uint32_t seed_hi, uint32_t sequence,
                   const uint32_t *__restrict__ sequence_dev, uint32_t stream_id, const int32_t *__restrict__ fixed_frames,
                   int32_t *__restrict__ seg_frame, int32_t *__restrict__ pix, int64_t *__restrict__ rows) {
    const uint32_t seq = sequence + (sequence_dev ? sequence_dev[0] : 0u);
    for (uint32_t n = blockIdx.x * FB_BLOCK + threadIdx.x; n < N; n += gridDim.x * FB_BLOCK) {
        const uint32_t s = n / K;
        const int32_t f = fixed_frames ? fixed_frames[s] : (int32_t)__umulhi(occ_philox(s, seq, 2u, stream_id, seed_lo, seed_hi).x, F);
        const uint32_t p = __umulhi(occ_philox(n, seq, 3u, stream_id, seed_lo, seed_hi).x, P);
        if (n - s * K == 0u) seg_frame[s] = f;
        pix[n] = (int32_t)p;
        // a fixed frame outside [0, F) stays in seg_frame (its rays become NaN); its rows stay inside the target table
        const uint32_t fr = (uint32_t)f < F ? (uint32_t)f : 0u;
        rows[n] = (int64_t)((uint64_t)fr * P + p);
    }
}

// after the draw, on the same stream: never the drawing kernel, which reads the word
__global__ void k_advance_sequence(uint32_t *__restrict__ sequence_dev) { sequence_dev[0] += 1u; }

// ---------------------------------------------------------------------------------------------
// forward: ru_write_ray (the arithmetic of k_generate_rays, contraction off) with the pose of the ray's segment
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FB_BLOCK)
k_generate_rays_frames(const float *__restrict__ poses, uint32_t F, uint32_t w, float fx, float fy, float cx, float cy, int camera_flip,
                       const int32_t *__restrict__ seg_frame, const int32_t *__restrict__ pix, uint32_t K, uint32_t N,
                       float *__restrict__ rays_o, float *__restrict__ rays_d) {
    const float f0 = (camera_flip >> 2) & 1 ? -1.0f : 1.0f;   // nerf_lib.py:121, bit order [2,1,0]
    const float f1 = (camera_flip >> 1) & 1 ? -1.0f : 1.0f;
    const float f2 = (camera_flip >> 0) & 1 ? -1.0f : 1.0f;
    for (uint32_t n = blockIdx.x * FB_BLOCK + threadIdx.x; n < N; n += gridDim.x * FB_BLOCK) {
        const uint32_t f = (uint32_t)seg_frame[n / K];
        if (f >= F) {      // no such frame: rays the march treats as out of range
            const float nan = __int_as_float(0x7fc00000);
#pragma unroll
            for (int k = 0; k < 3; k++) { rays_o[(size_t)n * 3 + k] = nan; rays_d[(size_t)n * 3 + k] = nan; }
            continue;
        }
        ru_write_ray(ru_load_pose(poses + (size_t)f * 12), f0, f1, f2, (uint32_t)pix[n], w, fx, fy, cx, cy, (size_t)n, rays_o, rays_d);
    }
}

// ---------------------------------------------------------------------------------------------
// backward: grad_poses[f] = sum over the rays of the segments naming f of the terms of k_generate_rays_bwd (ru_pose_term, fp64)
// ---------------------------------------------------------------------------------------------
// The three parts of seg_sum.h with twelve sums per segment: k_frames_bwd_thread, k_frames_bwd_block, and k_frames_bwd_final, a
// wave per frame over the segments naming it.
struct FbCam { uint32_t F, w; float fx, fy, cx, cy; int camera_flip; };

__global__ void __launch_bounds__(FB_BLOCK)
k_frames_bwd_thread(const float *__restrict__ poses, FbCam c, const int32_t *__restrict__ seg_frame, const int32_t *__restrict__ pix,
                    uint32_t S, uint32_t K, const float *__restrict__ g_o, const float *__restrict__ g_d, double *__restrict__ partials) {
    const uint32_t s = blockIdx.x * FB_BLOCK + threadIdx.x;
    if (s >= S) return;
    const uint32_t f = (uint32_t)seg_frame[s];
    if (f >= c.F) return;
    double R[3][3];
    ru_load_rotation(poses + (size_t)f * 12, R);
    const double f0 = (c.camera_flip >> 2) & 1 ? -1.0 : 1.0, f1 = (c.camera_flip >> 1) & 1 ? -1.0 : 1.0, f2 = (c.camera_flip >> 0) & 1 ? -1.0 : 1.0;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.0;
    for (uint32_t k = 0; k < K; k++) {
        const size_t n = (size_t)s * K + k;
        ru_pose_term(R, f0, f1, f2, (uint32_t)pix[n], c.w, c.fx, c.fy, c.cx, c.cy, g_o, g_d, n, acc);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) partials[(size_t)s * 12 + k] = acc[k];
}

__global__ void __launch_bounds__(FB_BLOCK)
k_frames_bwd_block(const float *__restrict__ poses, FbCam c, const int32_t *__restrict__ seg_frame, const int32_t *__restrict__ pix,
                   uint32_t K, uint32_t B, const float *__restrict__ g_o, const float *__restrict__ g_d, double *__restrict__ partials) {
    __shared__ double red[12][FB_BLOCK / 64];
    const uint32_t s = blockIdx.x / B, b = blockIdx.x - s * B;
    const uint32_t f = (uint32_t)seg_frame[s];
    if (f >= c.F) return;                                     // the whole block: nobody waits at the block sum's barrier
    double R[3][3];
    ru_load_rotation(poses + (size_t)f * 12, R);
    const double f0 = (c.camera_flip >> 2) & 1 ? -1.0 : 1.0, f1 = (c.camera_flip >> 1) & 1 ? -1.0 : 1.0, f2 = (c.camera_flip >> 0) & 1 ? -1.0 : 1.0;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.0;
    for (uint32_t k = b * FB_BLOCK + threadIdx.x; k < K; k += B * FB_BLOCK) {
        const size_t n = (size_t)s * K + k;
        ru_pose_term(R, f0, f1, f2, (uint32_t)pix[n], c.w, c.fx, c.fy, c.cx, c.cy, g_o, g_d, n, acc);
    }
    nsr_block_sum_stage(acc, red);
    if (threadIdx.x < 12) partials[(size_t)blockIdx.x * 12 + threadIdx.x] = nsr_block_sum_col<FB_BLOCK / 64>(red[threadIdx.x]);
}

__global__ void __launch_bounds__(64)
k_frames_bwd_final(const double *__restrict__ partials, const int32_t *__restrict__ seg_frame, uint32_t S, uint32_t B,
                   float *__restrict__ grad_poses) {
    const int32_t f = (int32_t)blockIdx.x;
    const double acc = seg_frame_sum(seg_frame, S, B, partials, 12u, 0u, 12u, [f](int32_t named) { return named == f; });
    if (threadIdx.x < 12u) grad_poses[(size_t)f * 12 + threadIdx.x] = (float)acc;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int nsr_draw_frame_batch(uint32_t F, uint32_t P, uint32_t S, uint32_t K, uint64_t seed, uint32_t sequence, uint32_t *sequence_dev,
                         uint32_t stream_id, const int32_t *fixed_frames, int advance, int32_t *seg_frame, int32_t *pix, int64_t *rows,
                         nsr_stream_t stream) {
    if (advance && sequence_dev == nullptr) return NSR_ERR_INVALID_ARG;
    const uint64_t N = (uint64_t)S * K;
    if (N > 0xffffffffull) return NSR_ERR_INVALID_ARG;
    if (N == 0 && !advance) return NSR_OK;
    if (N != 0) {
        NSR_CHECK_PTR(seg_frame); NSR_CHECK_PTR(pix); NSR_CHECK_PTR(rows);
        if (F == 0 || P == 0 || F > 0x7fffffffu || P > 0x7fffffffu) return NSR_ERR_INVALID_ARG;
        hipLaunchKernelGGL(k_draw_frame_batch, dim3(nsr_grid_1d(N, FB_BLOCK)), dim3(FB_BLOCK), 0, (hipStream_t)stream, F, P, K, (uint32_t)N,
                           (uint32_t)seed, (uint32_t)(seed >> 32), sequence, (const uint32_t *)sequence_dev, stream_id, fixed_frames,
                           seg_frame, pix, rows);
    }
    if (advance) hipLaunchKernelGGL(k_advance_sequence, dim3(1), dim3(1), 0, (hipStream_t)stream, sequence_dev);
    return nsr_launch_status();
}

int nsr_generate_rays_frames(const float *poses, uint32_t F, uint32_t w, uint32_t h, float fx, float fy, float cx, float cy,
                             int camera_flip, const int32_t *seg_frame, const int32_t *pix, uint32_t S, uint32_t K, float *rays_o,
                             float *rays_d, nsr_stream_t stream) {
    const uint64_t N = (uint64_t)S * K;
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(poses); NSR_CHECK_PTR(seg_frame); NSR_CHECK_PTR(pix); NSR_CHECK_PTR(rays_o); NSR_CHECK_PTR(rays_d);
    if (w == 0 || h == 0 || F == 0 || N > 0xffffffffull) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_generate_rays_frames, dim3(nsr_grid_1d(N, FB_BLOCK)), dim3(FB_BLOCK), 0, (hipStream_t)stream, poses, F, w, fx, fy,
                       cx, cy, camera_flip, seg_frame, pix, K, (uint32_t)N, rays_o, rays_d);
    return nsr_launch_status();
}

uint64_t nsr_generate_rays_frames_backward_workspace_bytes(uint32_t F, uint32_t S, uint32_t K) {
    (void)F;
    const uint64_t bytes = (uint64_t)S * seg_blocks(K) * 12 * sizeof(double);
    return bytes ? bytes : 12 * sizeof(double);
}

int nsr_generate_rays_frames_backward(const float *poses, uint32_t F, uint32_t w, uint32_t h, float fx, float fy, float cx, float cy,
                                      int camera_flip, const int32_t *seg_frame, const int32_t *pix, uint32_t S, uint32_t K,
                                      const float *grad_rays_o, const float *grad_rays_d, void *workspace, float *grad_poses,
                                      nsr_stream_t stream) {
    if (F == 0) return NSR_OK;
    NSR_CHECK_PTR(grad_poses);
    uint64_t N = (uint64_t)S * K;
    const uint32_t B = seg_blocks(K);
    if (N != 0) {
        NSR_CHECK_PTR(poses); NSR_CHECK_PTR(seg_frame); NSR_CHECK_PTR(pix); NSR_CHECK_PTR(grad_rays_o); NSR_CHECK_PTR(grad_rays_d);
        NSR_CHECK_PTR(workspace);
        if (w == 0 || h == 0 || ((uintptr_t)workspace & 7u) != 0 || N > 0xffffffffull || (uint64_t)S * B > 0x7fffffffull)
            return NSR_ERR_INVALID_ARG;
        const FbCam c{F, w, fx, fy, cx, cy, camera_flip};
        if (K < SEG_THREAD_K)
            hipLaunchKernelGGL(k_frames_bwd_thread, dim3(nsr_div_up(S, FB_BLOCK)), dim3(FB_BLOCK), 0, (hipStream_t)stream, poses, c, seg_frame,
                               pix, S, K, grad_rays_o, grad_rays_d, (double *)workspace);
        else
            hipLaunchKernelGGL(k_frames_bwd_block, dim3(S * B), dim3(FB_BLOCK), 0, (hipStream_t)stream, poses, c, seg_frame, pix, K, B,
                               grad_rays_o, grad_rays_d, (double *)workspace);
    }
    // no rays: every frame's gradient is still written (zeros)
    hipLaunchKernelGGL(k_frames_bwd_final, dim3(F), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, seg_frame,
                       N != 0 ? S : 0u, B, grad_poses);
    return nsr_launch_status();
}

}   // extern "C"
