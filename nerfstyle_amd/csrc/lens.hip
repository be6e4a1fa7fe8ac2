// Lens refinement: the rays of a mixed-frame batch through a lens that lives in device memory, lens = (fx, fy, cx, cy, k1, k2),
// and the backward towards the poses and the lens.  A captured graph therefore replays with the values the optimiser wrote.
//     k_generate_rays_lens          k_generate_rays_frames with ru_write_ray_lens
//     k_lens_bwd_thread / _block    k_frames_bwd_thread / _block with eighteen sums per segment (twelve pose, six lens)
//     k_lens_bwd_final              a wave per frame for the pose rows, one more wave for the lens row
// The single-pose case is F = S = 1, K = N.
#include "ray_pose.h"
#include "seg_sum.h"

static_assert(FB_BLOCK == SEG_BLOCK, "seg_blocks counts blocks of SEG_BLOCK threads");

__global__ void __launch_bounds__(FB_BLOCK)
k_generate_rays_lens(const float *__restrict__ poses, uint32_t F, uint32_t w, const float *__restrict__ lens, int camera_flip,
                     const int32_t *__restrict__ seg_frame, const int32_t *__restrict__ pix, uint32_t K, uint32_t N,
                     float *__restrict__ rays_o, float *__restrict__ rays_d) {
    const float f0 = (camera_flip >> 2) & 1 ? -1.0f : 1.0f;   // nerf_lib.py:121, bit order [2,1,0]
    const float f1 = (camera_flip >> 1) & 1 ? -1.0f : 1.0f;
    const float f2 = (camera_flip >> 0) & 1 ? -1.0f : 1.0f;
    const RuLens Ln = ru_load_lens(lens);
    for (uint32_t n = blockIdx.x * FB_BLOCK + threadIdx.x; n < N; n += gridDim.x * FB_BLOCK) {
        const uint32_t f = (uint32_t)seg_frame[n / K];
        if (f >= F) {      // no such frame: rays the march treats as out of range
            const float nan = __int_as_float(0x7fc00000);
#pragma unroll
            for (int k = 0; k < 3; k++) { rays_o[(size_t)n * 3 + k] = nan; rays_d[(size_t)n * 3 + k] = nan; }
            continue;
        }
        ru_write_ray_lens(ru_load_pose(poses + (size_t)f * 12), f0, f1, f2, (uint32_t)pix[n], w, Ln, (size_t)n, rays_o, rays_d);
    }
}

// ---------------------------------------------------------------------------------------------
// backward: the three parts of seg_sum.h with eighteen sums per segment, columns 0..11 the pose's and 12..17 the lens's
// ---------------------------------------------------------------------------------------------
struct LensCam { uint32_t F, w; int camera_flip; };

__device__ __forceinline__ void lens_load(const float *__restrict__ lens, double (&L)[6]) {
#pragma unroll
    for (int k = 0; k < 6; k++) L[k] = (double)lens[k];
}

__global__ void __launch_bounds__(FB_BLOCK)
k_lens_bwd_thread(const float *__restrict__ poses, LensCam c, const float *__restrict__ lens, const int32_t *__restrict__ seg_frame,
                  const int32_t *__restrict__ pix, uint32_t S, uint32_t K, const float *__restrict__ g_o, const float *__restrict__ g_d,
                  double *__restrict__ partials) {
    const uint32_t s = blockIdx.x * FB_BLOCK + threadIdx.x;
    if (s >= S) return;
    const uint32_t f = (uint32_t)seg_frame[s];
    if (f >= c.F) return;
    double R[3][3], L[6];
    ru_load_rotation(poses + (size_t)f * 12, R);
    lens_load(lens, L);
    const double f0 = (c.camera_flip >> 2) & 1 ? -1.0 : 1.0, f1 = (c.camera_flip >> 1) & 1 ? -1.0 : 1.0, f2 = (c.camera_flip >> 0) & 1 ? -1.0 : 1.0;
    double acc[18];
#pragma unroll
    for (int k = 0; k < 18; k++) acc[k] = 0.0;
    for (uint32_t k = 0; k < K; k++) {
        const size_t n = (size_t)s * K + k;
        ru_lens_term(R, f0, f1, f2, (uint32_t)pix[n], c.w, L, g_o, g_d, n, acc);
    }
#pragma unroll
    for (int k = 0; k < 18; k++) partials[(size_t)s * 18 + k] = acc[k];
}

__global__ void __launch_bounds__(FB_BLOCK)
k_lens_bwd_block(const float *__restrict__ poses, LensCam c, const float *__restrict__ lens, const int32_t *__restrict__ seg_frame,
                 const int32_t *__restrict__ pix, uint32_t K, uint32_t B, const float *__restrict__ g_o, const float *__restrict__ g_d,
                 double *__restrict__ partials) {
    __shared__ double red[18][FB_BLOCK / 64];
    const uint32_t s = blockIdx.x / B, b = blockIdx.x - s * B;
    const uint32_t f = (uint32_t)seg_frame[s];
    if (f >= c.F) return;                                     // the whole block: nobody waits at the block sum's barrier
    double R[3][3], L[6];
    ru_load_rotation(poses + (size_t)f * 12, R);
    lens_load(lens, L);
    const double f0 = (c.camera_flip >> 2) & 1 ? -1.0 : 1.0, f1 = (c.camera_flip >> 1) & 1 ? -1.0 : 1.0, f2 = (c.camera_flip >> 0) & 1 ? -1.0 : 1.0;
    double acc[18];
#pragma unroll
    for (int k = 0; k < 18; k++) acc[k] = 0.0;
    for (uint32_t k = b * FB_BLOCK + threadIdx.x; k < K; k += B * FB_BLOCK) {
        const size_t n = (size_t)s * K + k;
        ru_lens_term(R, f0, f1, f2, (uint32_t)pix[n], c.w, L, g_o, g_d, n, acc);
    }
    nsr_block_sum_stage(acc, red);
    if (threadIdx.x < 18) partials[(size_t)blockIdx.x * 18 + threadIdx.x] = nsr_block_sum_col<FB_BLOCK / 64>(red[threadIdx.x]);
}

// Blocks 0 .. pose_rows-1 (pose_rows = F, or 0 without grad_poses): a frame's pose row, columns 0..11 of the segments naming it.
// Block pose_rows: the lens row, columns 12..17 of every segment that names a frame in [0, F).
__global__ void __launch_bounds__(64)
k_lens_bwd_final(const double *__restrict__ partials, const int32_t *__restrict__ seg_frame, uint32_t S, uint32_t B, uint32_t F,
                 uint32_t pose_rows, float *__restrict__ grad_poses, float *__restrict__ grad_lens) {
    const uint32_t row = blockIdx.x, lane = threadIdx.x;
    if (row == pose_rows) {
        const double acc = seg_frame_sum(seg_frame, S, B, partials, 18u, 12u, 6u, [F](int32_t named) { return (uint32_t)named < F; });
        if (lane < 6u) grad_lens[lane] = (float)acc;
    } else {
        const double acc = seg_frame_sum(seg_frame, S, B, partials, 18u, 0u, 12u, [row](int32_t named) { return (uint32_t)named == row; });
        if (lane < 12u) grad_poses[(size_t)row * 12 + lane] = (float)acc;
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int nsr_generate_rays_lens(const float *poses, uint32_t F, uint32_t w, uint32_t h, const float *lens, int camera_flip,
                           const int32_t *seg_frame, const int32_t *pix, uint32_t S, uint32_t K, float *rays_o, float *rays_d,
                           nsr_stream_t stream) {
    const uint64_t N = (uint64_t)S * K;
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(poses); NSR_CHECK_PTR(lens); NSR_CHECK_PTR(seg_frame); NSR_CHECK_PTR(pix); NSR_CHECK_PTR(rays_o); NSR_CHECK_PTR(rays_d);
    if (w == 0 || h == 0 || F == 0 || N > 0xffffffffull) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_generate_rays_lens, dim3(nsr_grid_1d(N, FB_BLOCK)), dim3(FB_BLOCK), 0, (hipStream_t)stream, poses, F, w, lens,
                       camera_flip, seg_frame, pix, K, (uint32_t)N, rays_o, rays_d);
    return nsr_launch_status();
}

uint64_t nsr_generate_rays_lens_backward_workspace_bytes(uint32_t F, uint32_t S, uint32_t K) {
    (void)F;
    const uint64_t bytes = (uint64_t)S * seg_blocks(K) * 18 * sizeof(double);
    return bytes ? bytes : 18 * sizeof(double);
}

int nsr_generate_rays_lens_backward(const float *poses, uint32_t F, uint32_t w, uint32_t h, const float *lens, int camera_flip,
                                    const int32_t *seg_frame, const int32_t *pix, uint32_t S, uint32_t K, const float *grad_rays_o,
                                    const float *grad_rays_d, void *workspace, float *grad_poses, float *grad_lens,
                                    nsr_stream_t stream) {
    NSR_CHECK_PTR(grad_lens);
    if (F > 0x7ffffffeu) return NSR_ERR_INVALID_ARG;
    const uint64_t N = F != 0 ? (uint64_t)S * K : 0;          // without frames no segment names one
    const uint32_t B = seg_blocks(K);
    if (N != 0) {
        NSR_CHECK_PTR(poses); NSR_CHECK_PTR(lens); NSR_CHECK_PTR(seg_frame); NSR_CHECK_PTR(pix); NSR_CHECK_PTR(grad_rays_o);
        NSR_CHECK_PTR(grad_rays_d); NSR_CHECK_PTR(workspace);
        if (w == 0 || h == 0 || ((uintptr_t)workspace & 7u) != 0 || N > 0xffffffffull || (uint64_t)S * B > 0x7fffffffull)
            return NSR_ERR_INVALID_ARG;
        const LensCam c{F, w, camera_flip};
        if (K < SEG_THREAD_K)
            hipLaunchKernelGGL(k_lens_bwd_thread, dim3(nsr_div_up(S, FB_BLOCK)), dim3(FB_BLOCK), 0, (hipStream_t)stream, poses, c, lens,
                               seg_frame, pix, S, K, grad_rays_o, grad_rays_d, (double *)workspace);
        else
            hipLaunchKernelGGL(k_lens_bwd_block, dim3(S * B), dim3(FB_BLOCK), 0, (hipStream_t)stream, poses, c, lens, seg_frame, pix, K, B,
                               grad_rays_o, grad_rays_d, (double *)workspace);
    }
    // no rays: the lens row and every frame's row are still written (zeros)
    const uint32_t pose_rows = grad_poses != nullptr ? F : 0u;
    hipLaunchKernelGGL(k_lens_bwd_final, dim3(pose_rows + 1u), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, seg_frame,
                       N != 0 ? S : 0u, B, F, pose_rows, grad_poses, grad_lens);
    return nsr_launch_status();
}

}   // extern "C"
