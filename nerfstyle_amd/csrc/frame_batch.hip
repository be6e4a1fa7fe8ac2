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
// forward: the body of k_generate_rays (ru_generate_rays, ray_pose.h) with the pose of the ray's segment
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FB_BLOCK)
k_generate_rays_frames(const float *__restrict__ poses, uint32_t F, uint32_t w, float fx, float fy, float cx, float cy, int camera_flip,
                       const int32_t *__restrict__ seg_frame, const int32_t *__restrict__ pix, uint32_t K, uint32_t N,
                       float *__restrict__ rays_o, float *__restrict__ rays_d) {
    ru_generate_rays<size_t>(RuSegPoses{poses, seg_frame, pix, F, K}, RuPinhole{fx, fy, cx, cy}, camera_flip, w, FB_BLOCK, N, rays_o,
                             rays_d);
}

// ---------------------------------------------------------------------------------------------
// backward: grad_poses[f] = sum over the rays of the segments naming f of the terms of k_generate_rays_bwd (ru_pose_term, fp64)
// ---------------------------------------------------------------------------------------------
// The three parts of seg_sum.h with twelve sums per segment: k_frames_bwd_thread and k_frames_bwd_block are seg_sum_thread and
// seg_sum_block over ru_pose_term, k_frames_bwd_final is a wave per frame over the segments naming it.
struct FbBwdArgs {
    const float *poses;
    uint32_t F, w;
    RuPinhole cam;
    int camera_flip;
    const int32_t *seg_frame, *pix;
    uint32_t S, K, B;
    const float *g_o, *g_d;
    double *partials;                     // [S][B][12]
};

// make_term of seg_sum.h: ru_pose_term with the rotation of the segment's frame
__device__ __forceinline__ auto fb_pose_terms(const FbBwdArgs &a) {
    return [=](uint32_t f, size_t n0) {
        double R[3][3];
        ru_load_rotation(a.poses + (size_t)f * 12, R);
        const RuFlip<double> flip = ru_flip<double>(a.camera_flip);
        return [=](uint32_t k, double (&acc)[12]) {
            const size_t n = n0 + k;
            ru_pose_term(R, flip, (uint32_t)a.pix[n], a.w, a.cam, a.g_o, a.g_d, n, acc);
        };
    };
}

__global__ void __launch_bounds__(SEG_BLOCK)
k_frames_bwd_thread(FbBwdArgs a) {
    seg_sum_thread<12>(a.seg_frame, a.F, a.S, a.K, a.partials, fb_pose_terms(a));
}

__global__ void __launch_bounds__(SEG_BLOCK)
k_frames_bwd_block(FbBwdArgs a) {
    __shared__ double red[12][SEG_BLOCK / 64];
    seg_sum_block<12>(a.seg_frame, a.F, a.K, a.B, a.partials, red, fb_pose_terms(a));
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
        if (w == 0 || h == 0 || !seg_sum_ok(N, S, K, workspace)) return NSR_ERR_INVALID_ARG;
        const FbBwdArgs a{poses, F, w, RuPinhole{fx, fy, cx, cy}, camera_flip, seg_frame, pix, S, K, B, grad_rays_o, grad_rays_d,
                          (double *)workspace};
        seg_sum_launch(k_frames_bwd_thread, k_frames_bwd_block, S, K, (hipStream_t)stream, a);
    }
    // no rays: every frame's gradient is still written (zeros)
    hipLaunchKernelGGL(k_frames_bwd_final, dim3(F), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, seg_frame,
                       N != 0 ? S : 0u, B, grad_poses);
    return nsr_launch_status();
}

}   // extern "C"
