// Matting-Laplacian photorealism loss (Levin et al., "A Closed-Form Solution to Natural Image Matting"; the
// regulariser of Deep Photo Style Transfer), matrix-free: the value trace(V M V^T) and d/dV of the reference's
// MattingLaplacian (loss.py:217-278) without building the HW x HW sparse matrix.
//
// For every (2r+1)^2 window w that lies inside the image (k pixels) and every channel c of v:
//   mu = mean(I),  Sigma = (1/k) sum I I^T - mu mu^T + (eps/k) Id,  s0 = sum v,  s2 = sum v^2,  u = sum v (I - mu)
//   a = Sigma^-1 u / k,  beta = s0/k - mu^T a
//   L        = sum_w sum_c  s2 - s0^2/k - u^T a
//   dL/dv_pc = 2 sum_{w contains p} (v_pc - beta_wc - I_p^T a_wc) = 2 (n_p v_pc - sum beta - I_p^T sum a)
// All arithmetic in fp64.  The moments are taken of I minus the window's centre pixel: Sigma and u do not change with a shift
// of I, and the subtraction sum I I^T / k - mu mu^T then cancels numbers of the size of the window's spread, not of the
// image's level; on a step edge between two flat regions the raw moments lose the small eigenvalues' last digits (a
// gradient 3e-10 of its maximum off where two centred fp64 evaluations agree to 5e-11).  Sigma is factorised as L D L^T
// (backward stable): an adjugate over the determinant loses the small eigenvalues of a window that straddles a sharp edge
// (Sigma ~ rank 1 + eps/k), where the reference's LU does not.
//
// One workgroup per 32x8 pixel tile.  It stages target and v of the tile plus a 2r halo in LDS (as f32: the inputs are
// f32, converted to fp64 when read), solves every window whose centre lies within r of the tile (coefficients a, beta
// in LDS; windows outside the image store zeros) and gathers them per pixel.  The value of a window is added by the one
// tile that holds its centre; the block partials are summed in a fixed order by k_matting_final: no atomics, the result
// is the same bit for bit from run to run.
#include "fixed_sum.h"

#define MT_TX 32
#define MT_TY 8
#define MT_BLOCK (MT_TX * MT_TY)

struct MattingArgs {
    const float *target, *v;   // [3,H,W]
    uint32_t H, W;
    double eps;
    double *partials;          // [nblocks]
    double *loss;              // [1]
    float *grad;               // [3,H,W] or NULL
    uint32_t nblocks;
};

template <int R>
__global__ void __launch_bounds__(MT_BLOCK)
k_matting(MattingArgs a) {
    constexpr int D = 2 * R + 1, K = D * D;
    constexpr int PW = MT_TX + 4 * R, PH = MT_TY + 4 * R;     // staged pixels: tile + 2r halo
    constexpr int WW = MT_TX + 2 * R, WH = MT_TY + 2 * R;     // windows whose centre is within r of the tile
    constexpr int NP = PW * PH, NW = WW * WH;
    __shared__ float s_img[6][NP];                            // target rgb, then v rgb
    __shared__ double s_cf[12][NW];                           // a[c][0..2] at 4c+0..2, beta[c] at 4c+3
    __shared__ double s_red[MT_BLOCK / 64];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * MT_TX, y0 = blockIdx.y * MT_TY;
    const int H = (int)a.H, W = (int)a.W;
    const size_t plane = (size_t)a.H * a.W;

    for (int i = tid; i < NP; i += MT_BLOCK) {
        const int gx = x0 - 2 * R + i % PW, gy = y0 - 2 * R + i / PW;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const size_t o = in ? (size_t)gy * a.W + gx : 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            s_img[c][i] = in ? a.target[c * plane + o] : 0.0f;
            s_img[3 + c][i] = in ? a.v[c * plane + o] : 0.0f;
        }
    }
    __syncthreads();

    const double invk = 1.0 / (double)K;
    const double reg = a.eps / (double)K;
    double val = 0.0;
    for (int j = tid; j < NW; j += MT_BLOCK) {
        const int wx = j % WW, wy = j / WW;
        const int cx = x0 - R + wx, cy = y0 - R + wy;         // window centre in the image
        double cf[12];
#pragma unroll
        for (int q = 0; q < 12; q++) cf[q] = 0.0;
        if (cx >= R && cx < W - R && cy >= R && cy < H - R) {
            // moments over the window (the reference's win_mu / win_var, loss.py:252-254) of I - I(centre)
            const int pc = (wy + R) * PW + wx + R;
            const double c0 = s_img[0][pc], c1 = s_img[1][pc], c2 = s_img[2][pc];
            double sI[3] = {0.0, 0.0, 0.0}, sII[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            double s0[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0}, sVI[3][3] = {};
#pragma unroll 1
            for (int dy = 0; dy < D; dy++) {
#pragma unroll
                for (int dx = 0; dx < D; dx++) {
                    const int p = (wy + dy) * PW + wx + dx;
                    const double i0 = (double)s_img[0][p] - c0, i1 = (double)s_img[1][p] - c1, i2 = (double)s_img[2][p] - c2;
                    sI[0] += i0; sI[1] += i1; sI[2] += i2;
                    sII[0] += i0 * i0; sII[1] += i0 * i1; sII[2] += i0 * i2;
                    sII[3] += i1 * i1; sII[4] += i1 * i2; sII[5] += i2 * i2;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const double vc = s_img[3 + c][p];
                        s0[c] += vc; s2[c] += vc * vc;
                        sVI[c][0] += vc * i0; sVI[c][1] += vc * i1; sVI[c][2] += vc * i2;
                    }
                }
            }
            const double m0 = sI[0] * invk, m1 = sI[1] * invk, m2 = sI[2] * invk;
            const double S00 = sII[0] * invk - m0 * m0 + reg, S01 = sII[1] * invk - m0 * m1, S02 = sII[2] * invk - m0 * m2;
            const double S11 = sII[3] * invk - m1 * m1 + reg, S12 = sII[4] * invk - m1 * m2;
            const double S22 = sII[5] * invk - m2 * m2 + reg;
            // Sigma = L D L^T
            const double d0 = S00, r0 = 1.0 / d0;
            const double l10 = S01 * r0, l20 = S02 * r0;
            const double d1 = S11 - l10 * S01, r1 = 1.0 / d1;
            const double e21 = S12 - l20 * S01;
            const double l21 = e21 * r1;
            const double d2 = S22 - l20 * S02 - l21 * e21, r2 = 1.0 / d2;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                // u = sum v (I - mu) = sum v I - s0 mu, the same for the shifted I
                const double u0 = sVI[c][0] - s0[c] * m0, u1 = sVI[c][1] - s0[c] * m1, u2 = sVI[c][2] - s0[c] * m2;
                const double z0 = u0, z1 = u1 - l10 * z0, z2 = u2 - l20 * z0 - l21 * z1;
                const double x2 = z2 * r2, x1 = z1 * r1 - l21 * x2, x0 = z0 * r0 - l10 * x1 - l20 * x2;
                const double a0 = x0 * invk, a1 = x1 * invk, a2 = x2 * invk;
                cf[4 * c + 0] = a0; cf[4 * c + 1] = a1; cf[4 * c + 2] = a2;
                cf[4 * c + 3] = s0[c] * invk - ((m0 + c0) * a0 + (m1 + c1) * a1 + (m2 + c2) * a2);     // mu = m + I(centre)
                if (wx >= R && wx < R + MT_TX && wy >= R && wy < R + MT_TY)     // this tile holds the centre
                    val += s2[c] - s0[c] * s0[c] * invk - (u0 * a0 + u1 * a1 + u2 * a2);
            }
        }
        if (a.grad) {
#pragma unroll
            for (int q = 0; q < 12; q++) s_cf[q][j] = cf[q];
        }
    }

    nsr_block_sum_stage(val, s_red);                          // its barrier also publishes s_cf
    if (tid == 0) a.partials[blockIdx.y * gridDim.x + blockIdx.x] = nsr_block_sum_col<MT_BLOCK / 64>(s_red);
    if (!a.grad) return;

    const int tx = tid % MT_TX, ty = tid / MT_TX;
    const int px = x0 + tx, py = y0 + ty;
    if (px >= W || py >= H) return;
    double sa[12];
#pragma unroll
    for (int q = 0; q < 12; q++) sa[q] = 0.0;
#pragma unroll 1
    for (int dy = 0; dy < D; dy++) {
#pragma unroll
        for (int dx = 0; dx < D; dx++) {
            const int j = (ty + dy) * WW + tx + dx;           // windows centred at (px - r + dx, py - r + dy)
#pragma unroll
            for (int q = 0; q < 12; q++) sa[q] += s_cf[q][j];
        }
    }
    // number of windows inside the image that contain p
    const int nx = min(px + R, W - 1 - R) - max(px - R, R) + 1;
    const int ny = min(py + R, H - 1 - R) - max(py - R, R) + 1;
    const double n = (double)(nx * ny);
    const int p = (ty + 2 * R) * PW + tx + 2 * R;
    const double i0 = s_img[0][p], i1 = s_img[1][p], i2 = s_img[2][p];
    const size_t o = (size_t)py * a.W + px;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double g = n * (double)s_img[3 + c][p] - sa[4 * c + 3] - (i0 * sa[4 * c] + i1 * sa[4 * c + 1] + i2 * sa[4 * c + 2]);
        a.grad[c * plane + o] = (float)(2.0 * g);
    }
}

__global__ void __launch_bounds__(MT_BLOCK)
k_matting_final(MattingArgs a) {
    __shared__ double red[MT_BLOCK / 64];
    double s = 0.0;
    for (uint32_t b = threadIdx.x; b < a.nblocks; b += MT_BLOCK) s += a.partials[b];
    nsr_block_sum_stage(s, red);
    if (threadIdx.x == 0) a.loss[0] = nsr_block_sum_col<MT_BLOCK / 64>(red);
}

static dim3 mt_grid(uint32_t H, uint32_t W) { return dim3(nsr_div_up(W, MT_TX), nsr_div_up(H, MT_TY)); }

extern "C" {

uint64_t nsr_matting_laplacian_workspace_bytes(uint32_t H, uint32_t W, uint32_t win_rad) {
    (void)win_rad;
    const dim3 g = mt_grid(H, W);
    return (uint64_t)g.x * g.y * sizeof(double);
}

int nsr_matting_laplacian(const float *target, const float *v, uint32_t H, uint32_t W, uint32_t win_rad, double eps,
                          double *loss_out, float *grad_v, void *workspace, nsr_stream_t stream) {
    NSR_CHECK_PTR(target); NSR_CHECK_PTR(v); NSR_CHECK_PTR(loss_out); NSR_CHECK_PTR(workspace);
    if (win_rad != 1 && win_rad != 2) return NSR_ERR_UNSUPPORTED;
    if (H < 2 * win_rad + 1 || W < 2 * win_rad + 1 || H > 65535u * MT_TY) return NSR_ERR_INVALID_ARG;
    if ((uintptr_t)workspace & 7u) return NSR_ERR_INVALID_ARG;
    MattingArgs a;
    a.target = target; a.v = v; a.H = H; a.W = W; a.eps = eps;
    a.partials = (double *)workspace; a.loss = loss_out; a.grad = grad_v;
    const dim3 g = mt_grid(H, W);
    a.nblocks = g.x * g.y;
    const hipStream_t s = (hipStream_t)stream;
    if (win_rad == 1) hipLaunchKernelGGL(k_matting<1>, g, dim3(MT_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(k_matting<2>, g, dim3(MT_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_matting_final, dim3(1), dim3(MT_BLOCK), 0, s, a);
    return nsr_launch_status();
}

}   // extern "C"
