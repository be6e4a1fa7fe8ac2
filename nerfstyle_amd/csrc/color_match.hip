// Colour transfer of pixel rows to a style image (ARF's colour matching; the reference's match_colors_for_image_set,
// utils/__init__.py:262-295), the two streaming passes over rows that already live in HBM:
//   nsr_color_moments   sum x and sum x x^T of every row's RGB in fp64, in an order fixed by (n, stride)
//   nsr_color_apply     x -> A x + b as an f32 fma chain, optional clamp to [0, 1], in place or to another buffer
// The 3x3 eigen-solve between them is host code (nerfstyle_amd/color_match.py).
//
// Rows are n x stride floats, stride 3 (RGB) or 4 (RGB + one float that is carried, never read as colour).  Both passes
// are bound by memory traffic and move 16 B per lane per access where the layout allows: a stride-4 row is one float4;
// four stride-3 rows are three float4 when their first byte is 16-byte aligned, scalar loads otherwise.  Which loads are
// used never changes the arithmetic or its order.
// The per-region form of both passes is color_regions.hip; what the two files share is color_common.h.
#include "color_common.h"

// ---- moments -------------------------------------------------------------------------------------------------------------------
// Units and the grid: color_common.h.  Thread t of the grid (T threads) adds units t, t + T, ... in that order and the rows of a
// group in ascending order: nine fp64 accumulators per thread.
template <int STRIDE>
__global__ void __launch_bounds__(CM_BLOCK)
k_color_moments(const float *__restrict__ rows, uint64_t n, double *__restrict__ partials) {
    __shared__ double red[9][CM_WAVES];
    CmAcc a;
#pragma unroll
    for (int k = 0; k < 9; k++) a.s[k] = 0.0;
    const uint64_t T = (uint64_t)gridDim.x * CM_BLOCK;
    const uint64_t tid = (uint64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    if (STRIDE == 4) {
        // four rows a trip, T apart (every access of a wave is 1 KiB contiguous), loaded before they are added in order
        const float4 *q = reinterpret_cast<const float4 *>(rows);
        for (uint64_t i = tid; i < n; i += 4 * T) {
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (i + k * T < n) v[k] = q[i + k * T];
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (i + k * T < n) cm_add(a, v[k].x, v[k].y, v[k].z);
        }
    } else {
        const uint64_t groups = (n + 3) / 4, full = n / 4;
        const bool vec = ((uintptr_t)rows & 15u) == 0;                  // a full group is 48 B
        for (uint64_t g = tid; g < groups; g += T) {
            const float *p = rows + g * 12;
            if (g < full && vec) {
                const float4 *q = reinterpret_cast<const float4 *>(p);
                const float4 v0 = q[0], v1 = q[1], v2 = q[2];
                cm_add(a, v0.x, v0.y, v0.z); cm_add(a, v0.w, v1.x, v1.y);
                cm_add(a, v1.z, v1.w, v2.x); cm_add(a, v2.y, v2.z, v2.w);
            } else {
                const uint32_t m = g < full ? 4u : (uint32_t)(n - g * 4);
                for (uint32_t j = 0; j < m; j++) cm_add(a, p[j * 3], p[j * 3 + 1], p[j * 3 + 2]);
            }
        }
    }
    nsr_block_sum_stage(a.s, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) partials[(uint64_t)blockIdx.x * 9 + k] = nsr_block_sum_col<CM_WAVES>(red[k]);
    }
}

// one block: thread t adds the partials of blocks t, t + 256, ... in that order, then the block sum
__global__ void __launch_bounds__(CM_BLOCK)
k_color_moments_final(const double *__restrict__ partials, uint32_t nblocks, double *__restrict__ moments) {
    __shared__ double red[9][CM_WAVES];
    CmAcc a;
#pragma unroll
    for (int k = 0; k < 9; k++) a.s[k] = 0.0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += CM_BLOCK) {
#pragma unroll
        for (int k = 0; k < 9; k++) a.s[k] += partials[(uint64_t)b * 9 + k];
    }
    nsr_block_sum_stage(a.s, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) moments[k] = nsr_block_sum_col<CM_WAVES>(red[k]);
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------
// stride 4: one float4 per row, four rows a thread per trip (T apart, so every access of a wave is 1 KiB contiguous).
// A row is read and written by the same thread, so dst == src is safe.
__global__ void __launch_bounds__(CM_BLOCK)
k_color_apply4(const float *src, float *dst, uint64_t n, const float *__restrict__ tf, int clamp) {
    const CmTf t = cm_load_tf(tf);
    const float4 *s = reinterpret_cast<const float4 *>(src);
    float4 *d = reinterpret_cast<float4 *>(dst);
    const uint64_t T = (uint64_t)gridDim.x * CM_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * CM_BLOCK + threadIdx.x; i < n; i += 4 * T) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k * T < n) v[k] = s[i + k * T];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k * T < n) {
                cm_map(t, clamp, v[k].x, v[k].y, v[k].z);        // .w is carried as loaded
                d[i + k * T] = v[k];
            }
    }
}

// stride 3: rows [head, head + 4 * ngroups) as groups of four rows = three float4 (the host makes their first byte 16-byte
// aligned in src and dst alike), the other n - 4 * ngroups rows (head, tail, or all of them) one float at a time
__global__ void __launch_bounds__(CM_BLOCK)
k_color_apply3(const float *src, float *dst, uint64_t n, uint32_t head, uint64_t ngroups, const float *__restrict__ tf, int clamp) {
    const CmTf t = cm_load_tf(tf);
    const uint64_t T = (uint64_t)gridDim.x * CM_BLOCK;
    const uint64_t tid = (uint64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
    const float4 *s = reinterpret_cast<const float4 *>(src + (uint64_t)head * 3);
    float4 *d = reinterpret_cast<float4 *>(dst + (uint64_t)head * 3);
    for (uint64_t g = tid; g < ngroups; g += T) {
        float4 v0 = s[g * 3], v1 = s[g * 3 + 1], v2 = s[g * 3 + 2];
        cm_map(t, clamp, v0.x, v0.y, v0.z);
        cm_map(t, clamp, v0.w, v1.x, v1.y);
        cm_map(t, clamp, v1.z, v1.w, v2.x);
        cm_map(t, clamp, v2.y, v2.z, v2.w);
        d[g * 3] = v0; d[g * 3 + 1] = v1; d[g * 3 + 2] = v2;
    }
    const uint64_t nscalar = n - 4 * ngroups;
    for (uint64_t j = tid; j < nscalar; j += T) {
        const uint64_t row = j < head ? j : j + 4 * ngroups;
        float r = src[row * 3], g = src[row * 3 + 1], b = src[row * 3 + 2];
        cm_map(t, clamp, r, g, b);
        dst[row * 3] = r; dst[row * 3 + 1] = g; dst[row * 3 + 2] = b;
    }
}

extern "C" {

// enough for either stride: the stride-4 grid (one unit a row) is never the smaller one
uint64_t nsr_color_moments_workspace_bytes(uint64_t n) { return (uint64_t)cm_moment_blocks(n) * 9 * sizeof(double); }

int nsr_color_moments(const float *rows, uint64_t n, uint32_t stride, double *moments, void *workspace, nsr_stream_t stream) {
    NSR_CHECK_PTR(rows); NSR_CHECK_PTR(moments); NSR_CHECK_PTR(workspace);
    if (n == 0 || (stride != 3 && stride != 4)) return NSR_ERR_INVALID_ARG;
    if (((uintptr_t)rows & 3u) || ((uintptr_t)moments & 7u) || ((uintptr_t)workspace & 7u)) return NSR_ERR_INVALID_ARG;
    if (stride == 4 && ((uintptr_t)rows & 15u)) return NSR_ERR_INVALID_ARG;
    const uint32_t nblocks = cm_moment_blocks(cm_moment_units(n, stride));
    const hipStream_t s = (hipStream_t)stream;
    double *partials = (double *)workspace;
    if (stride == 4) hipLaunchKernelGGL(k_color_moments<4>, dim3(nblocks), dim3(CM_BLOCK), 0, s, rows, n, partials);
    else hipLaunchKernelGGL(k_color_moments<3>, dim3(nblocks), dim3(CM_BLOCK), 0, s, rows, n, partials);
    hipLaunchKernelGGL(k_color_moments_final, dim3(1), dim3(CM_BLOCK), 0, s, (const double *)partials, nblocks, moments);
    return nsr_launch_status();
}

int nsr_color_apply(const float *src, float *dst, uint64_t n, uint32_t stride, const float *tf, int clamp, nsr_stream_t stream) {
    NSR_CHECK_PTR(src); NSR_CHECK_PTR(dst); NSR_CHECK_PTR(tf);
    if (n == 0 || (stride != 3 && stride != 4)) return NSR_ERR_INVALID_ARG;
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if ((a & 3u) || (b & 3u) || ((uintptr_t)tf & 3u)) return NSR_ERR_INVALID_ARG;
    if (n > (UINT64_MAX >> 8) / stride) return NSR_ERR_INVALID_ARG;
    const uint64_t bytes = n * stride * sizeof(float);
    if (a != b && a < b + bytes && b < a + bytes) return NSR_ERR_INVALID_ARG;       // in place or disjoint, nothing between
    const hipStream_t s = (hipStream_t)stream;
    if (stride == 4) {
        if ((a & 15u) || (b & 15u)) return NSR_ERR_INVALID_ARG;
        hipLaunchKernelGGL(k_color_apply4, dim3(nsr_grid_1d((n + 3) / 4, CM_BLOCK)), dim3(CM_BLOCK), 0, s, src, dst, n, tf, clamp);
    } else {
        // rows are 12 B: `head` rows bring a base at 4 * head bytes past a 16-byte boundary onto the next one.  src and dst
        // must sit at the same offset for the float4 path; otherwise every row goes the scalar way.
        uint32_t head = 0;
        uint64_t ngroups = 0;
        if ((a & 15u) == (b & 15u)) {
            head = (uint32_t)((a >> 2) & 3u);
            if (head > n) head = (uint32_t)n;
            ngroups = (n - head) / 4;
        }
        const uint64_t nscalar = n - 4 * ngroups;
        hipLaunchKernelGGL(k_color_apply3, dim3(nsr_grid_1d(ngroups > nscalar ? ngroups : nscalar, CM_BLOCK)), dim3(CM_BLOCK), 0, s,
                           src, dst, n, head, ngroups, tf, clamp);
    }
    return nsr_launch_status();
}

}   // extern "C"
