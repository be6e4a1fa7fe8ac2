// Marks the occupancy cells that no training camera sees as untrained (density_grid = -1): the producer of the state that
// nsr_occ_update and the occupied-cell list (occupancy.hip) already respect -- torch-ngp's mark_untrained_grid, instant-ngp's
// mark_untrained_density_grid -- which the reference dropped.  include/nsr.h ("Untrained cells") states the geometry; every
// operation of it is an IEEE fp64 + - x in the order written there (the square roots are taken on the host), and the whole file
// is compiled with contraction off, so tests/untrained_ref.py reaches the same bits with NumPy.
//
// One thread owns one bitfield byte = 8 consecutive cells of one cascade = the 2x2x2 Morton block at (ix0, iy0, iz0): the grid
// goes through registers as two 16-byte accesses (k_occ_packbits' shape), the byte is read, masked and written by the same
// thread, so no two threads touch the same word.  Every thread walks ALL F frames (no early exit: F is tens to hundreds and the
// kernel runs once per dataset); the poses sit in LDS as fp64, at most OU_CHUNK frames at a time, and every lane reads the same
// pose word (a broadcast, no bank conflict).
#include "nsr_common.h"
#include "rm_util.h"
#include "ray_pose.h"

#pragma clang fp contract(off)

#define OU_BLOCK 256
#define OU_CHUNK 128u          // frames staged per trip: 128 x 12 fp64 = 12 KiB of LDS

struct OuArgs {
    uint32_t *grid;            // density_grid as bit patterns: values that stay are never passed through a float operation
    uint8_t *bitfield;         // optional
    const float *poses;
    int32_t *counts;           // optional
    uint32_t *n_untrained;     // optional
    uint32_t C, H, N, bytes_per_cas, F, min_views;
    double bound, margin_cells, rH;
    double x_lo, x_hi, y_lo, y_hi;
    double kx_lo, kx_hi, ky_lo, ky_hi;       // sqrt(1 + x_lo^2), ...: the lengths of the half-spaces' normals
    double f0, f1, f2;
};

__global__ void __launch_bounds__(64)
k_ou_zero(uint32_t *__restrict__ n_untrained, uint32_t C) {
    if (threadIdx.x < C) n_untrained[threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(OU_BLOCK)
k_ou_mark(OuArgs a) {
    __shared__ double pose[OU_CHUNK * 12];
    __shared__ uint32_t marked[8];           // this block's untrained cells per cascade
    if (threadIdx.x < 8) marked[threadIdx.x] = 0u;
    // (the first __syncthreads of the frame loop orders this before any LDS atomic: F >= 1)
    for (uint32_t base = blockIdx.x * OU_BLOCK; base < a.N; base += gridDim.x * OU_BLOCK) {
        const uint32_t n = base + threadIdx.x;
        const bool live = n < a.N;
        // bytes_per_cas = H^3 / 8 is a multiple of 64 from H = 8 on: the 64 bytes of a wave lie in one cascade
        const uint32_t cas = (live ? n : base) / a.bytes_per_cas;
        const uint32_t m0 = ((live ? n : base) - cas * a.bytes_per_cas) * 8u;
        const uint32_t i0[3] = {rm_morton3d_invert(m0), rm_morton3d_invert(m0 >> 1), rm_morton3d_invert(m0 >> 2)};
        const double b = fmin((double)(1u << cas), a.bound);                 // min(2^cas, bound)
        const double half = b * a.rH;                                        // b / H; H is a power of two: exact either way
        const double rho = (a.margin_cells * half) * 1.7320508075688772;     // sqrt(3.0), correctly rounded
        const double lim_xhi = rho * a.kx_hi, lim_xlo = rho * a.kx_lo, lim_yhi = rho * a.ky_hi, lim_ylo = rho * a.ky_lo;
        // the two centres per axis of the 2x2x2 block: X = b (2 i + 1 - H) / H
        double X[3][2];
#pragma unroll
        for (int d = 0; d < 3; d++) {
#pragma unroll
            for (int k = 0; k < 2; k++)
                X[d][k] = (b * (double)(2 * (int32_t)(i0[d] + k) + 1 - (int32_t)a.H)) * a.rH;
        }
        uint32_t count[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (uint32_t f_lo = 0; f_lo < a.F; f_lo += OU_CHUNK) {
            const uint32_t nf = min(OU_CHUNK, a.F - f_lo);
            __syncthreads();                                                 // the last trip's readers are done
            for (uint32_t i = threadIdx.x; i < nf * 12u; i += OU_BLOCK) pose[i] = (double)a.poses[(size_t)f_lo * 12u + i];
            __syncthreads();
            if (!live) continue;                                             // (after both barriers: they are block-uniform)
            for (uint32_t f = 0; f < nf; f++) {
                const double *P = pose + f * 12u;
                double D[3][2];                                              // X - t
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    D[d][0] = X[d][0] - P[d * 4 + 3];
                    D[d][1] = X[d][1] - P[d * 4 + 3];
                }
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const double dx = D[0][j & 1], dy = D[1][(j >> 1) & 1], dz = D[2][(j >> 2) & 1];
                    // q = R^T (X - t), then the flip: the inverse of ru_write_ray's (x f0, y f1, f2) -> R c
                    const double xc = ((P[0] * dx + P[4] * dy) + P[8] * dz) * a.f0;
                    const double yc = ((P[1] * dx + P[5] * dy) + P[9] * dz) * a.f1;
                    const double zc = ((P[2] * dx + P[6] * dy) + P[10] * dz) * a.f2;
                    const bool seen = (zc + rho > 0.0) && (xc - a.x_hi * zc <= lim_xhi) && (a.x_lo * zc - xc <= lim_xlo) &&
                                      (yc - a.y_hi * zc <= lim_yhi) && (a.y_lo * zc - yc <= lim_ylo);
                    count[j] += seen ? 1u : 0u;
                }
            }
        }
        uint32_t clear = 0u;
        if (live) {
            uint4 *g4 = reinterpret_cast<uint4 *>(a.grid) + (size_t)n * 2;
            const uint4 lo = g4[0], hi = g4[1];
            uint32_t g[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (count[j] < a.min_views) {
                    g[j] = 0xBF800000u;                                      // -1.0f
                    clear |= 1u << j;
                } else if (__uint_as_float(g[j]) < 0.0f) {
                    g[j] = 0u;                                               // seen again: trainable, from zero
                }                                                            // else: the value's bits, NaN and -0.0f included
            }
            g4[0] = make_uint4(g[0], g[1], g[2], g[3]);
            g4[1] = make_uint4(g[4], g[5], g[6], g[7]);
            if (a.bitfield) a.bitfield[n] = (uint8_t)(a.bitfield[n] & ~clear);
            if (a.counts) {
                int4 *c4 = reinterpret_cast<int4 *>(a.counts) + (size_t)n * 2;
                c4[0] = make_int4((int)count[0], (int)count[1], (int)count[2], (int)count[3]);
                c4[1] = make_int4((int)count[4], (int)count[5], (int)count[6], (int)count[7]);
            }
        }
        if (a.n_untrained) {
            const uint32_t s = nsr_wave_sum((uint32_t)__popc(clear));
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&marked[cas], s);
        }
    }
    if (a.n_untrained) {
        __syncthreads();
        if (threadIdx.x < a.C && marked[threadIdx.x]) atomicAdd(a.n_untrained + threadIdx.x, marked[threadIdx.x]);
    }
}

// the shape rule of every nsr_occ_* call (occupancy.hip, occ_dims_ok)
static bool ou_dims_ok(uint32_t C, uint32_t H) {
    return C >= 1 && C <= 8 && H >= 8 && H <= 512 && (H & (H - 1u)) == 0u && (uint64_t)C * H * H * H < (1ull << 31);
}

extern "C" {

int nsr_occ_mark_untrained(float *density_grid, uint8_t *bitfield, uint32_t C, uint32_t H, float bound, const float *poses,
                           uint32_t F, double x_lo, double x_hi, double y_lo, double y_hi, int camera_flip, double margin_cells,
                           uint32_t min_views, int32_t *counts, uint32_t *n_untrained, nsr_stream_t stream) {
    NSR_CHECK_PTR(density_grid); NSR_CHECK_PTR(poses);
    if (!ou_dims_ok(C, H) || !(bound > 0.0f)) return NSR_ERR_INVALID_ARG;
    if (F == 0u || min_views == 0u || !(margin_cells >= 0.0)) return NSR_ERR_INVALID_ARG;
    if (!(x_lo < x_hi) || !(y_lo < y_hi) || !(x_hi - x_lo < INFINITY) || !(y_hi - y_lo < INFINITY)) return NSR_ERR_INVALID_ARG;
    if (((uintptr_t)density_grid | (uintptr_t)counts) & 15u) return NSR_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    OuArgs a;
    a.grid = reinterpret_cast<uint32_t *>(density_grid); a.bitfield = bitfield; a.poses = poses; a.counts = counts;
    a.n_untrained = n_untrained;
    a.C = C; a.H = H; a.bytes_per_cas = H * H * H / 8u; a.N = C * a.bytes_per_cas; a.F = F; a.min_views = min_views;
    a.bound = (double)bound; a.margin_cells = margin_cells; a.rH = 1.0 / (double)H;
    a.x_lo = x_lo; a.x_hi = x_hi; a.y_lo = y_lo; a.y_hi = y_hi;
    a.kx_lo = sqrt(1.0 + x_lo * x_lo); a.kx_hi = sqrt(1.0 + x_hi * x_hi);
    a.ky_lo = sqrt(1.0 + y_lo * y_lo); a.ky_hi = sqrt(1.0 + y_hi * y_hi);
    const RuFlip<double> flip = ru_flip<double>(camera_flip);          // as k_generate_rays
    a.f0 = flip.f0; a.f1 = flip.f1; a.f2 = flip.f2;
    if (n_untrained) hipLaunchKernelGGL(k_ou_zero, dim3(1), dim3(64), 0, s, n_untrained, C);
    hipLaunchKernelGGL(k_ou_mark, dim3(nsr_grid_1d(a.N, OU_BLOCK)), dim3(OU_BLOCK), 0, s, a);
    return nsr_launch_status();
}

}   // extern "C"
