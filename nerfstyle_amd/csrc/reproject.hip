// View reprojection (include/nsr.h, "View reprojection"): a rendered frame warped into a neighbouring camera through its
// depth, the pixels the other camera cannot see discarded, and the squared error of what is left.  The per-pixel body is
// reproject_core.h's; this file is the walk over (pair, pixel) and the fixed-order sum.
//
//   k_reproject        block pair * B + b, B = ceil(H*W / 256): thread t takes dst pixel b * 256 + t of the pair (consecutive
//                      lanes read consecutive rows of dist[a] and rgb[a]; the four taps of frame b are a gather), writes
//                      warped and mask when they are given and adds (squared error, 1) when the pixel is valid; the block sum
//                      of fixed_sum.h, thread k writes sum k to slot partials[blockIdx.x][k]
//   k_reproject_final  block pair: thread t adds slots t, t + 256, ... of the pair in that order, then the block sum -> stats
// No atomics and no counters: every slot read was written earlier in the same call, so stats is the same bits from call to call.
// A pair that names a frame outside [0, F) reads neither frame: its pixels are invalid and its slots hold zeros.
//
// Bytes per pair with N = H*W: read 4 N (dist[a]) + 12 N (rgb[a], valid pixels) + up to 16 N + 48 N (the taps, which
// neighbouring pixels share through the caches); written 12 N (warped) + N (mask) when asked for, and 16 B (the slots).
#include "fixed_sum.h"
#include "reproject_core.h"

#define RP_BLOCK 256
#define RP_MAX_PIXELS (1u << 30)

struct ReprojectArgs {
    const float *rgb, *dist, *poses;
    const int32_t *pairs;
    uint32_t F, HW, B;                   // B: blocks, and slots, per pair
    RpCamera cam;
    double depth_tol;
    float *warped;                       // [P, H*W, 3] or NULL
    uint8_t *mask;                       // [P, H*W] or NULL
    double *partials;                    // [P][B][2]
    double *stats;                       // [P, 2]
};

__global__ void __launch_bounds__(RP_BLOCK)
k_reproject(ReprojectArgs a) {
    __shared__ double red[2][RP_BLOCK / 64];
    const uint32_t pair = blockIdx.x / a.B, blk = blockIdx.x - pair * a.B;
    const uint32_t p = blk * RP_BLOCK + threadIdx.x;
    const uint32_t fa = (uint32_t)a.pairs[2 * pair], fb = (uint32_t)a.pairs[2 * pair + 1];
    double acc[2] = {0.0, 0.0};
    if (p < a.HW) {
        bool valid = false;
        double wc[3] = {0.0, 0.0, 0.0};
        if (fa < a.F && fb < a.F) {
            const size_t ra = (size_t)fa * a.HW, rb = (size_t)fb * a.HW;
            const RpFrame A = rp_frame(a.poses + (size_t)fa * 12, a.dist + ra, a.rgb + ra * 3);
            const RpFrame Bf = rp_frame(a.poses + (size_t)fb * 12, a.dist + rb, a.rgb + rb * 3);
            valid = rp_reproject_pixel(a.cam, A, Bf, p, a.depth_tol, wc);
            if (valid) {
                acc[0] = rp_sq_error(wc, A.rgb + (size_t)p * 3);
                acc[1] = 1.0;
            }
        }
        const size_t row = (size_t)pair * a.HW + p;
        if (a.warped) {
#pragma unroll
            for (int k = 0; k < 3; k++) a.warped[row * 3 + k] = valid ? (float)wc[k] : 0.0f;
        }
        if (a.mask) a.mask[row] = valid ? 1 : 0;
    }
    nsr_block_sum_stage(acc, red);
    if (threadIdx.x < 2) a.partials[(size_t)blockIdx.x * 2 + threadIdx.x] = nsr_block_sum_col<RP_BLOCK / 64>(red[threadIdx.x]);
}

__global__ void __launch_bounds__(RP_BLOCK)
k_reproject_final(ReprojectArgs a) {
    __shared__ double red[2][RP_BLOCK / 64];
    const double *slots = a.partials + (size_t)blockIdx.x * a.B * 2;
    double s[2] = {0.0, 0.0};
    for (uint32_t b = threadIdx.x; b < a.B; b += RP_BLOCK) {
        s[0] += slots[(size_t)b * 2];
        s[1] += slots[(size_t)b * 2 + 1];
    }
    nsr_block_sum_stage(s, red);
    if (threadIdx.x < 2) a.stats[(size_t)blockIdx.x * 2 + threadIdx.x] = nsr_block_sum_col<RP_BLOCK / 64>(red[threadIdx.x]);
}

static inline bool rp_shape_ok(uint32_t P, uint32_t H, uint32_t W) {
    return H >= 2 && W >= 2 && (uint64_t)H * W <= RP_MAX_PIXELS && (uint64_t)P * nsr_div_up((uint64_t)H * W, RP_BLOCK) <= 0x7fffffffull;
}

extern "C" {

uint64_t nsr_reproject_frames_workspace_bytes(uint32_t P, uint32_t H, uint32_t W) {
    if (!rp_shape_ok(P, H, W)) return 0;
    return (uint64_t)P * nsr_div_up((uint64_t)H * W, RP_BLOCK) * 2 * sizeof(double);
}

int nsr_reproject_frames(const float *rgb, const float *dist, const float *poses, uint32_t F, uint32_t H, uint32_t W, float fx, float fy,
                         float cx, float cy, int camera_flip, const int32_t *pairs, uint32_t P, double depth_tol, float *warped,
                         uint8_t *mask, double *stats, void *workspace, nsr_stream_t stream) {
    if (!rp_shape_ok(P, H, W) || F == 0 || camera_flip < 0 || camera_flip > 7) return NSR_ERR_INVALID_ARG;
    if (!(fx != 0.0f && fy != 0.0f) || !(depth_tol >= 0.0)) return NSR_ERR_INVALID_ARG;
    if (P == 0) return NSR_OK;
    NSR_CHECK_PTR(rgb); NSR_CHECK_PTR(dist); NSR_CHECK_PTR(poses); NSR_CHECK_PTR(pairs); NSR_CHECK_PTR(stats); NSR_CHECK_PTR(workspace);
    if (((uintptr_t)rgb & 3u) || ((uintptr_t)dist & 3u) || ((uintptr_t)poses & 3u) || ((uintptr_t)pairs & 3u) || ((uintptr_t)warped & 3u) ||
        ((uintptr_t)stats & 7u) || ((uintptr_t)workspace & 7u))
        return NSR_ERR_INVALID_ARG;

    ReprojectArgs a;
    a.rgb = rgb; a.dist = dist; a.poses = poses; a.pairs = pairs;
    a.F = F; a.HW = H * W; a.B = nsr_div_up(a.HW, RP_BLOCK);
    a.cam = rp_camera(fx, fy, cx, cy, W, H, camera_flip);
    a.depth_tol = depth_tol;
    a.warped = warped; a.mask = mask;
    a.partials = (double *)workspace; a.stats = stats;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_reproject, dim3(P * a.B), dim3(RP_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_reproject_final, dim3(P), dim3(RP_BLOCK), 0, s, a);
    return nsr_launch_status();
}

}   // extern "C"
