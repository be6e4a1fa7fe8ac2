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
    ru_generate_rays<size_t>(RuSegPoses{poses, seg_frame, pix, F, K}, ru_load_lens(lens), camera_flip, w, FB_BLOCK, N, rays_o, rays_d);
}

// ---------------------------------------------------------------------------------------------
// backward: the three parts of seg_sum.h with eighteen sums per segment, columns 0..11 the pose's and 12..17 the lens's
// ---------------------------------------------------------------------------------------------
struct LensBwdArgs {
    const float *poses;
    uint32_t F, w;
    int camera_flip;
    const float *lens;
    const int32_t *seg_frame, *pix;
    uint32_t S, K, B;
    const float *g_o, *g_d;
    double *partials;                     // [S][B][18]
};

// make_term of seg_sum.h: ru_lens_term with the rotation of the segment's frame and the lens in fp64
__device__ __forceinline__ auto lens_terms(const LensBwdArgs &a) {
    return [=](uint32_t f, size_t n0) {
        double R[3][3], L[6];
        ru_load_rotation(a.poses + (size_t)f * 12, R);
#pragma unroll
        for (int k = 0; k < 6; k++) L[k] = (double)a.lens[k];
        const RuFlip<double> flip = ru_flip<double>(a.camera_flip);
        return [=](uint32_t k, double (&acc)[18]) {
            const size_t n = n0 + k;
            ru_lens_term(R, flip, (uint32_t)a.pix[n], a.w, L, a.g_o, a.g_d, n, acc);
        };
    };
}

__global__ void __launch_bounds__(SEG_BLOCK)
k_lens_bwd_thread(LensBwdArgs a) {
    seg_sum_thread<18>(a.seg_frame, a.F, a.S, a.K, a.partials, lens_terms(a));
}

__global__ void __launch_bounds__(SEG_BLOCK)
k_lens_bwd_block(LensBwdArgs a) {
    __shared__ double red[18][SEG_BLOCK / 64];
    seg_sum_block<18>(a.seg_frame, a.F, a.K, a.B, a.partials, red, lens_terms(a));
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
        if (w == 0 || h == 0 || !seg_sum_ok(N, S, K, workspace)) return NSR_ERR_INVALID_ARG;
        const LensBwdArgs a{poses, F, w, camera_flip, lens, seg_frame, pix, S, K, B, grad_rays_o, grad_rays_d, (double *)workspace};
        seg_sum_launch(k_lens_bwd_thread, k_lens_bwd_block, S, K, (hipStream_t)stream, a);
    }
    // no rays: the lens row and every frame's row are still written (zeros)
    const uint32_t pose_rows = grad_poses != nullptr ? F : 0u;
    hipLaunchKernelGGL(k_lens_bwd_final, dim3(pose_rows + 1u), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, seg_frame,
                       N != 0 ? S : 0u, B, F, pose_rows, grad_poses, grad_lens);
    return nsr_launch_status();
}

}   // extern "C"
