// Fused Adam (+ GradScaler unscale, + EMA shadow, + grad zero-fill, + half copy) over one flat
// fp32 arena, gfx950.  Replaces torch.optim.Adam(eps=1e-15) + zero_grad + torch_ema on the hot
// path (trainers/base.py:216-229,420-426, utils/__init__.py:116-142): one streaming pass of
// 16-byte accesses instead of ~10 elementwise launches over 25 M parameters.
#include "nsr_common.h"

// the scalars of one step, shared by the flat (k_adam) and the lane-packed (k_lanes_adam) kernel
struct AdamScalars {
    float beta1, beta2, eps, step_size, inv_sqrt_bc2, grad_scale_inv, ema_decay;
    const uint32_t *dyn;             // device-side scaler state (nsr_scaler_update) or NULL: host-side scalars above
};

struct AdamArgs {
    float *p, *g, *m, *v, *ema;
    _Float16 *half_copy;
    uint64_t n, half_n;              // half_copy covers the first half_n elements (the tables of a whole-arena launch)
    uint32_t mask4;
    AdamScalars s;
};

// Device-side GradScaler + step bookkeeping (torch.cuda.amp.GradScaler's policy, trainers/base.py:228,420-425), 16 words:
//   [0] f32 scale   [1] i32 growth tracker   [2] u32 found_inf (set by k_grad_check, consumed by k_scaler_update)
//   [3] u32 optimiser steps taken (skipped steps do not count: bias corrections and the LambdaLR schedule follow it)
//   [4] u32 steps skipped so far   [5] u32 EMA updates made (torch_ema's num_updates)   [6..7] reserved
//   [8] u32 skip this step   [9] f32 step_size = lr / (1 - beta1^t)   [10] f32 1 / sqrt(1 - beta2^t)
//   [11] f32 1 / scale (the scale the gradients carry)   [12] f32 lr   [13] f32 EMA decay of this step   [14..15] reserved
enum { SC_SCALE = 0, SC_TRACKER = 1, SC_FOUND = 2, SC_STEP = 3, SC_SKIPPED = 4, SC_EMA_N = 5, SC_SKIP = 8, SC_STEP_SIZE = 9,
       SC_INV_BC2 = 10, SC_INV_SCALE = 11, SC_LR = 12, SC_EMA_DECAY = 13 };

// No FMA contraction in adam_one / ema_move: left to the compiler, k_adam and k_lanes_adam fused different products of
// b1 * m + (1 - b1) * g, and the two kernels differed in the last bits where the addends cancel.
__device__ __forceinline__ float adam_one(float &p, float g, float &m, float &v, const AdamScalars &a) {
#pragma clang fp contract(off)
    g *= a.grad_scale_inv;
    m = a.beta1 * m + (1.0f - a.beta1) * g;          // torch: exp_avg.lerp_(grad, 1 - beta1)
    v = a.beta2 * v + (1.0f - a.beta2) * g * g;      // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
    p -= a.step_size * (m / denom);
    return p;
}

// this step's scalars from the device-side scaler state (no-op on the host-scalar path); true: the step is skipped
__device__ __forceinline__ bool adam_scalars(AdamScalars &a) {
    if (!a.dyn) return false;
    a.step_size = __uint_as_float(a.dyn[SC_STEP_SIZE]);
    a.inv_sqrt_bc2 = __uint_as_float(a.dyn[SC_INV_BC2]);
    a.grad_scale_inv = __uint_as_float(a.dyn[SC_INV_SCALE]);
    a.ema_decay = __uint_as_float(a.dyn[SC_EMA_DECAY]);          // (read only where there is an EMA shadow)
    return a.dyn[SC_SKIP] != 0u;
}

// torch_ema: shadow.sub_((1 - decay) * (shadow - param)), k = 1 - decay
__device__ __forceinline__ void ema_move(float &e, float p, float k) {
#pragma clang fp contract(off)
    e -= k * (e - p);
}

__device__ __forceinline__ void ema_move(float *ema, uint64_t i, const float4 &p, float decay) {
    float4 e = reinterpret_cast<float4 *>(ema)[i];
    const float k = 1.0f - decay;
    ema_move(e.x, p.x, k); ema_move(e.y, p.y, k); ema_move(e.z, p.z, k); ema_move(e.w, p.w, k);
    reinterpret_cast<float4 *>(ema)[i] = e;
}

// four parameters -> the f16 gather copy (one table row of the interleaved layout)
__device__ __forceinline__ void store_half_row(_Float16 *half_copy, uint64_t r, const float4 &p) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 h;
    h[0] = (_Float16)p.x; h[1] = (_Float16)p.y; h[2] = (_Float16)p.z; h[3] = (_Float16)p.w;
    reinterpret_cast<h4 *>(half_copy)[r] = h;
}

// any non-finite value among the trained elements -> found_inf (GradScaler.unscale_'s check, one streaming pass)
__global__ void __launch_bounds__(256)
k_grad_check(const float *__restrict__ g, uint64_t n, uint32_t mask4, uint32_t *__restrict__ found) {
    const uint64_t n4 = n / 4;
    uint32_t bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    // exponent all ones <=> inf or nan
    auto chk = [&](const float4 &v) {
        const uint32_t e0 = __float_as_uint(v.x) & 0x7F800000u, e1 = __float_as_uint(v.y) & 0x7F800000u;
        const uint32_t e2 = __float_as_uint(v.z) & 0x7F800000u, e3 = __float_as_uint(v.w) & 0x7F800000u;
        bad |= ((mask4 & 1u) && e0 == 0x7F800000u) | ((mask4 & 2u) && e1 == 0x7F800000u) |
               ((mask4 & 4u) && e2 == 0x7F800000u) | ((mask4 & 8u) && e3 == 0x7F800000u);
    };
    for (; i + 3 * stride < n4; i += 4 * stride) {          // four 16-byte loads in flight per lane
        const float4 a0 = reinterpret_cast<const float4 *>(g)[i], a1 = reinterpret_cast<const float4 *>(g)[i + stride];
        const float4 a2 = reinterpret_cast<const float4 *>(g)[i + 2 * stride], a3 = reinterpret_cast<const float4 *>(g)[i + 3 * stride];
        chk(a0); chk(a1); chk(a2); chk(a3);
    }
    for (; i < n4; i += stride) chk(reinterpret_cast<const float4 *>(g)[i]);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) {
        const uint64_t j = n4 * 4 + threadIdx.x;
        if ((mask4 & (1u << (j & 3u))) && (__float_as_uint(g[j]) & 0x7F800000u) == 0x7F800000u) bad = 1;
    }
    if (__ballot(bad != 0) != 0ull && (threadIdx.x & 63u) == 0) atomicOr(found, 1u);
}

// one thread: GradScaler.step's decision + GradScaler.update + the step counter, the LambdaLR value and Adam's bias
// corrections (double precision, as torch computes them on the host)
__global__ void k_scaler_update(uint32_t *st, float lr_base, float lr_decay_steps, float beta1, float beta2, float growth,
                                float backoff, uint32_t growth_interval, int enabled, float ema_decay_max) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (ema_decay_max >= 0.0f) {
        // torch_ema (utils/__init__.py:116-142): num_updates += 1; decay = min(decay, (1 + n) / (10 + n)) -- on every call,
        // skipped optimiser steps included (ema.update() is unconditional, trainers/base.py:426)
        const uint32_t n = st[SC_EMA_N] + 1u;
        st[SC_EMA_N] = n;
        st[SC_EMA_DECAY] = __float_as_uint(fminf(ema_decay_max, (1.0f + (float)n) / (10.0f + (float)n)));
    }
    float scale = __uint_as_float(st[SC_SCALE]);
    const bool inf = enabled && st[SC_FOUND] != 0u;
    st[SC_FOUND] = 0u;
    st[SC_INV_SCALE] = __float_as_uint(enabled ? 1.0f / scale : 1.0f);         // the scale THESE gradients carry
    st[SC_SKIP] = inf ? 1u : 0u;
    if (inf) {
        st[SC_SKIPPED] += 1u;
        st[SC_SCALE] = __float_as_uint(scale * backoff);
        st[SC_TRACKER] = 0u;
        return;
    }
    const uint32_t t = st[SC_STEP] + 1u;
    st[SC_STEP] = t;
    // LambdaLR: k scheduler steps have been taken before optimiser step k + 1 (trainers/base.py:223-226,424-425)
    const double lr = lr_decay_steps > 0.0f ? (double)lr_base * pow(0.1, (double)(t - 1u) / (double)lr_decay_steps) : (double)lr_base;
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    st[SC_LR] = __float_as_uint((float)lr);
    st[SC_STEP_SIZE] = __float_as_uint((float)(lr / bc1));
    st[SC_INV_BC2] = __float_as_uint((float)(1.0 / sqrt(bc2)));
    if (enabled) {
        const uint32_t tr = st[SC_TRACKER] + 1u;
        if (tr >= growth_interval) {
            st[SC_SCALE] = __float_as_uint(scale * growth);
            st[SC_TRACKER] = 0u;
        } else {
            st[SC_TRACKER] = tr;
        }
    }
}

__global__ void __launch_bounds__(256)
k_adam(AdamArgs a) {
    const uint64_t n4 = a.n / 4;
    const bool skip = adam_scalars(a.s);
    if (skip) {
        // GradScaler skipped optimizer.step(): parameters and moments stay; the gradient is cleared (the reference's
        // zero_grad at the top of the next iteration) and the EMA still moves (ema.update() is unconditional, base.py:426)
        for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * blockDim.x) {
            reinterpret_cast<float4 *>(a.g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.ema) ema_move(a.ema, i, reinterpret_cast<float4 *>(a.p)[i], a.s.ema_decay);
        }
        if (blockIdx.x == 0 && threadIdx.x < (a.n & 3u)) {
            const uint64_t i = n4 * 4 + threadIdx.x;
            a.g[i] = 0.0f;
            if (a.ema) ema_move(a.ema[i], a.p[i], 1.0f - a.s.ema_decay);
        }
        return;
    }
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * blockDim.x) {
        float4 p = reinterpret_cast<float4 *>(a.p)[i];
        const float4 g = reinterpret_cast<float4 *>(a.g)[i];
        float4 m = reinterpret_cast<float4 *>(a.m)[i];
        float4 v = reinterpret_cast<float4 *>(a.v)[i];
        if (a.mask4 & 1u) adam_one(p.x, g.x, m.x, v.x, a.s);
        if (a.mask4 & 2u) adam_one(p.y, g.y, m.y, v.y, a.s);
        if (a.mask4 & 4u) adam_one(p.z, g.z, m.z, v.z, a.s);
        if (a.mask4 & 8u) adam_one(p.w, g.w, m.w, v.w, a.s);
        reinterpret_cast<float4 *>(a.p)[i] = p;
        reinterpret_cast<float4 *>(a.m)[i] = m;
        reinterpret_cast<float4 *>(a.v)[i] = v;
        reinterpret_cast<float4 *>(a.g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.ema) ema_move(a.ema, i, p, a.s.ema_decay);
        if (a.half_copy && i * 4 < a.half_n) store_half_row(a.half_copy, i, p);
    }
    if (blockIdx.x == 0 && threadIdx.x < (a.n & 3u)) {
        const uint64_t i = n4 * 4 + threadIdx.x;
        float p = a.p[i], m = a.m[i], v = a.v[i];
        if (a.mask4 & (1u << (i & 3u))) adam_one(p, a.g[i], m, v, a.s);
        a.p[i] = p; a.m[i] = m; a.v[i] = v; a.g[i] = 0.0f;
        if (a.ema) ema_move(a.ema[i], p, 1.0f - a.s.ema_decay);
        if (a.half_copy && i < a.half_n) a.half_copy[i] = (_Float16)p;
    }
}

// host-scalar path: Adam's bias corrections for step `step`, in double precision as torch computes them
static AdamScalars host_scalars(float lr, float beta1, float beta2, float eps, float grad_scale_inv, float ema_decay, uint32_t step) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    return AdamScalars{beta1, beta2, eps, (float)((double)lr / bc1), (float)(1.0 / sqrt(bc2)), grad_scale_inv, ema_decay, nullptr};
}

// device-state path: step size, bias correction, 1 / scale and the EMA decay are read from the state in the kernel
static AdamScalars device_scalars(float beta1, float beta2, float eps, const void *scaler_state) {
    return AdamScalars{beta1, beta2, eps, 0.0f, 1.0f, 1.0f, 0.0f, (const uint32_t *)scaler_state};
}

static int adam_launch(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *ema, void *half_copy, uint64_t n,
                       uint64_t half_n, uint32_t elem_mask4, const AdamScalars &sc, nsr_stream_t stream) {
    NSR_CHECK_PTR(params); NSR_CHECK_PTR(grads); NSR_CHECK_PTR(exp_avg); NSR_CHECK_PTR(exp_avg_sq);
    const uintptr_t al = (uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq |
                         (uintptr_t)ema | (uintptr_t)half_copy;
    if (al & 15u) return NSR_ERR_INVALID_ARG;
    const AdamArgs a{params, grads, exp_avg, exp_avg_sq, ema, (_Float16 *)half_copy, n, half_n, elem_mask4 & 0xFu, sc};
    hipLaunchKernelGGL(k_adam, dim3(nsr_grid_1d(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return nsr_launch_status();
}

extern "C" int nsr_adam_step(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *ema, void *half_copy,
                             uint64_t n, float lr, float beta1, float beta2, float eps, float grad_scale_inv, float ema_decay,
                             uint32_t step, uint32_t elem_mask4, nsr_stream_t stream) {
    if (n == 0) return NSR_OK;
    if (step == 0) return NSR_ERR_INVALID_ARG;
    return adam_launch(params, grads, exp_avg, exp_avg_sq, ema, half_copy, n, n, elem_mask4,
                       host_scalars(lr, beta1, beta2, eps, grad_scale_inv, ema_decay, step), stream);
}

extern "C" int nsr_grad_check(const float *grads, uint64_t n, uint32_t elem_mask4, void *scaler_state, nsr_stream_t stream) {
    if (n == 0) return NSR_OK;
    NSR_CHECK_PTR(grads); NSR_CHECK_PTR(scaler_state);
    if (((uintptr_t)grads & 15u) || ((uintptr_t)scaler_state & 3u)) return NSR_ERR_INVALID_ARG;
    uint64_t blocks = (n / 4 + 256 * 4 - 1) / (256 * 4);
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_grad_check, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, grads, n, elem_mask4 & 0xFu,
                       (uint32_t *)scaler_state + SC_FOUND);
    return nsr_launch_status();
}

extern "C" int nsr_scaler_update(void *scaler_state, float lr_base, float lr_decay_steps, float beta1, float beta2, float growth_factor,
                                 float backoff_factor, uint32_t growth_interval, int enabled, float ema_decay_max,
                                 nsr_stream_t stream) {
    NSR_CHECK_PTR(scaler_state);
    if (((uintptr_t)scaler_state & 3u) || growth_interval == 0) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_scaler_update, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t *)scaler_state, lr_base, lr_decay_steps, beta1,
                       beta2, growth_factor, backoff_factor, growth_interval, enabled, ema_decay_max);
    return nsr_launch_status();
}

extern "C" int nsr_adam_step_scaled(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *ema, void *half_copy,
                                    uint64_t n, uint64_t half_n, float beta1, float beta2, float eps, uint32_t elem_mask4,
                                    const void *scaler_state, nsr_stream_t stream) {
    if (n == 0) return NSR_OK;
    NSR_CHECK_PTR(scaler_state);
    if (((uintptr_t)scaler_state & 3u) || half_n > n || (half_n & 3u)) return NSR_ERR_INVALID_ARG;
    return adam_launch(params, grads, exp_avg, exp_avg_sq, ema, half_copy, n, half_n, elem_mask4,
                       device_scalars(beta1, beta2, eps, scaler_state), stream);
}

// ---- lane-packed tables: one hash table of the interleaved rows (tables[row][enc][feat], 16 B per row), trained alone ----
// (the stylisation stage, trainers/style.py:25) and sharded across data-parallel ranks.  The trained float2 of row r is
// packed[2r .. 2r+1]; lane0 = 0 (density table, mask 0x3) or 2 (colour table, mask 0xC).

__device__ __forceinline__ float2 lanes_of(const float4 &p, uint32_t lane0) {
    return lane0 ? make_float2(p.z, p.w) : make_float2(p.x, p.y);
}

// trained lanes of every row -> packed; all four lanes of the row's gradient zeroed (untrained gradients are still zeroed)
__global__ void __launch_bounds__(256)
k_lanes_pack(float *__restrict__ g, uint64_t rows, uint32_t lane0, float *__restrict__ packed) {
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4 *>(g)[r];
        reinterpret_cast<float2 *>(packed)[r] = lanes_of(v, lane0);
        reinterpret_cast<float4 *>(g)[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

struct LanesArgs {
    float *arena;                    // interleaved table rows, updated in place (trained lanes only)
    _Float16 *half_copy;             // f16 gather copy of the rows or NULL
    const float *g;                  // packed gradient of rows [row_lo, row_hi): g[2 (r - row_lo) + l]
    float *m, *v;                    // packed moments, same indexing
    float *ema;                      // EMA shadow of all four lanes of rows [row_lo, row_hi): ema[r - row_lo] (float4) or NULL
    float *out;                      // packed updated parameters, same indexing as g (may alias g)
    uint64_t row_lo, row_hi;
    uint32_t lane0;
    AdamScalars s;
};

// k_adam on the trained lanes of rows [row_lo, row_hi): the same adam_one and the same EMA expression over the whole row
// (k_adam's EMA moves all four elements of a region's float4), so a world of one equals nsr_adam_step* with elem_mask4 bit for bit
__global__ void __launch_bounds__(256)
k_lanes_adam(LanesArgs a) {
    const bool skip = adam_scalars(a.s);
    const uint64_t n = a.row_hi - a.row_lo;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = a.row_lo + i;
        float4 p = reinterpret_cast<const float4 *>(a.arena)[r];
        if (!skip) {
            const float2 g = reinterpret_cast<const float2 *>(a.g)[i];
            float2 m = reinterpret_cast<const float2 *>(a.m)[i];
            float2 v = reinterpret_cast<const float2 *>(a.v)[i];
            if (a.lane0) {
                adam_one(p.z, g.x, m.x, v.x, a.s);
                adam_one(p.w, g.y, m.y, v.y, a.s);
            } else {
                adam_one(p.x, g.x, m.x, v.x, a.s);
                adam_one(p.y, g.y, m.y, v.y, a.s);
            }
            reinterpret_cast<float4 *>(a.arena)[r] = p;
            reinterpret_cast<float2 *>(a.m)[i] = m;
            reinterpret_cast<float2 *>(a.v)[i] = v;
            if (a.half_copy) store_half_row(a.half_copy, r, p);
        }
        reinterpret_cast<float2 *>(a.out)[i] = lanes_of(p, a.lane0);
        if (a.ema) ema_move(a.ema, i, p, a.s.ema_decay);
    }
}

// gathered packed parameters of rows [row_lo, row_hi) -> their arena lanes and all four lanes of the f16 copy
__global__ void __launch_bounds__(256)
k_lanes_unpack(const float *__restrict__ packed, uint64_t row_lo, uint64_t row_hi, uint32_t lane0, float *__restrict__ arena,
               _Float16 *__restrict__ half_copy) {
    for (uint64_t r = row_lo + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < row_hi; r += (uint64_t)gridDim.x * blockDim.x) {
        const float2 q = reinterpret_cast<const float2 *>(packed)[r];
        float4 p = reinterpret_cast<const float4 *>(arena)[r];
        if (lane0) { p.z = q.x; p.w = q.y; } else { p.x = q.x; p.y = q.y; }
        reinterpret_cast<float4 *>(arena)[r] = p;
        if (half_copy) store_half_row(half_copy, r, p);
    }
}

static int lane0_of(uint32_t lane_mask) { return lane_mask == 0x3u ? 0 : lane_mask == 0xCu ? 2 : -1; }

extern "C" int nsr_lanes_pack(float *grad_arena, uint64_t rows, uint32_t lane_mask, float *packed, nsr_stream_t stream) {
    if (rows == 0) return NSR_OK;
    NSR_CHECK_PTR(grad_arena); NSR_CHECK_PTR(packed);
    const int lane0 = lane0_of(lane_mask);
    if (lane0 < 0 || ((uintptr_t)grad_arena & 15u) || ((uintptr_t)packed & 7u)) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_lanes_pack, dim3(nsr_grid_1d(rows, 256)), dim3(256), 0, (hipStream_t)stream, grad_arena, rows,
                       (uint32_t)lane0, packed);
    return nsr_launch_status();
}

static int lanes_adam_launch(float *arena, void *half_copy, const float *grad, float *exp_avg, float *exp_avg_sq, float *ema,
                             float *packed_out, uint64_t row_lo, uint64_t row_hi, uint32_t lane_mask, const AdamScalars &sc,
                             nsr_stream_t stream) {
    if (row_hi < row_lo) return NSR_ERR_INVALID_ARG;
    if (row_hi == row_lo) return NSR_OK;
    if (!arena || !grad || !exp_avg || !exp_avg_sq || !packed_out) return NSR_ERR_INVALID_ARG;
    const int lane0 = lane0_of(lane_mask);
    const uintptr_t al8 = (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)packed_out | (uintptr_t)half_copy;
    if (lane0 < 0 || (al8 & 7u) || (((uintptr_t)arena | (uintptr_t)ema) & 15u)) return NSR_ERR_INVALID_ARG;
    const LanesArgs a{arena, (_Float16 *)half_copy, grad, exp_avg, exp_avg_sq, ema, packed_out, row_lo, row_hi, (uint32_t)lane0, sc};
    hipLaunchKernelGGL(k_lanes_adam, dim3(nsr_grid_1d(row_hi - row_lo, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return nsr_launch_status();
}

extern "C" int nsr_lanes_adam(float *arena, void *half_copy, const float *grad, float *exp_avg, float *exp_avg_sq, float *ema,
                              float *packed_out, uint64_t row_lo, uint64_t row_hi, uint32_t lane_mask, float lr, float beta1,
                              float beta2, float eps, float grad_scale_inv, float ema_decay, uint32_t step, nsr_stream_t stream) {
    if (step == 0) return NSR_ERR_INVALID_ARG;
    return lanes_adam_launch(arena, half_copy, grad, exp_avg, exp_avg_sq, ema, packed_out, row_lo, row_hi, lane_mask,
                             host_scalars(lr, beta1, beta2, eps, grad_scale_inv, ema_decay, step), stream);
}

extern "C" int nsr_lanes_adam_scaled(float *arena, void *half_copy, const float *grad, float *exp_avg, float *exp_avg_sq,
                                     float *ema, float *packed_out, uint64_t row_lo, uint64_t row_hi, uint32_t lane_mask,
                                     float beta1, float beta2, float eps, const void *scaler_state, nsr_stream_t stream) {
    if (row_hi == row_lo) return NSR_OK;             // an empty shard is a no-op, as in nsr_lanes_adam and nsr_adam_step_scaled
    NSR_CHECK_PTR(scaler_state);
    if ((uintptr_t)scaler_state & 3u) return NSR_ERR_INVALID_ARG;
    return lanes_adam_launch(arena, half_copy, grad, exp_avg, exp_avg_sq, ema, packed_out, row_lo, row_hi, lane_mask,
                             device_scalars(beta1, beta2, eps, scaler_state), stream);
}

extern "C" int nsr_lanes_unpack(const float *packed, uint64_t row_lo, uint64_t row_hi, uint32_t lane_mask, float *arena,
                                void *half_copy, nsr_stream_t stream) {
    if (row_hi < row_lo) return NSR_ERR_INVALID_ARG;
    if (row_hi == row_lo) return NSR_OK;
    NSR_CHECK_PTR(packed); NSR_CHECK_PTR(arena);
    const int lane0 = lane0_of(lane_mask);
    if (lane0 < 0 || (((uintptr_t)packed | (uintptr_t)half_copy) & 7u) || ((uintptr_t)arena & 15u)) return NSR_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_lanes_unpack, dim3(nsr_grid_1d(row_hi - row_lo, 256)), dim3(256), 0, (hipStream_t)stream, packed, row_lo,
                       row_hi, (uint32_t)lane0, arena, (_Float16 *)half_copy);
    return nsr_launch_status();
}
