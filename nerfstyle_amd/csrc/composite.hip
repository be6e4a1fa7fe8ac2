// Training composite (raymarching.cu:806-997) with the render_train epilogue (renderer.py:225-233), the per-ray geometry terms
// (differentiable depth, mip-NeRF 360 distortion) and the reconstruction loss (trainers/base.py:251-304) for gfx950.
//
// In the ray kernels (k_comp_fwd, k_comp_bwd, k_geom_fwd, k_geom_bwd, and k_rays_pos_bwd, which sums the samples' position
// gradients back to their ray on the same walk) a WAVE owns a ray and a LANE owns a sample:
//   * 64 consecutive samples of the ray per trip: sigma / delta / colour rows are whole contiguous pieces of the sample
//     buffers (16-byte loads for C = 4 or 8);
//   * the recurrences are wave scans on the DPP network (row_shr 1/2/4/8, row_bcast 15/31): transmittance = exclusive
//     product scan of (1 - alpha), t = inclusive sum scan of the step lengths, the backward's running colour = inclusive
//     sum scans of weight * colour; sums over the ray are lane 63 of a scan; a carry (T, t, sums) links the trips of a
//     ray longer than 64 samples; the early stop (T < T_thresh, :862 / :961) is a ballot;
//   * persistent waves (grid-stride over rays), the next ray's header in flight while this one is evaluated;
//   * the composite forward also writes what Renderer.render_train returns (image[:, :3] + (1 - weights_sum), the class
//     channels, (depth - near) clamped / (far - near)), its backward takes the gradients of exactly those outputs.
// Written once: the ray walk (CpWalk, all four), the trip carry and early stop (cp_carry, cp_stopped, all four) and the zeros behind
// a stop and on a dropped ray (cp_zero_tail, the two backwards).  The trip front is spelled out per kernel (why).
// The scans reassociate the reference's serial fp32 products and sums: results differ from the oracle in the last bits
// (tests: <= 2e-5 absolute), and are bit-identical from run to run.
//
// The loss kernel is one thread per ray (value + gradient in one pass, targets gathered through the pixel indices), a
// block sum for the value and a second one-block kernel that adds the block partials in a fixed order (fixed_sum.h in both).
#include <type_traits>
#include "seg_sum.h"

#define CP_MAXC 16
#define CP_BLOCK 256
static_assert(CP_BLOCK == SEG_BLOCK, "seg_blocks counts blocks of SEG_BLOCK threads");

#define CP_DPP(old, v, ctrl, rm, bm)                                                                                  \
    __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, (float)(old)), __builtin_bit_cast(int, (float)(v)), \
                                                          (ctrl), (rm), (bm), false))

// inclusive wave64 scans: lanes without a source keep the identity (`old` operand, bound_ctrl off)
__device__ __forceinline__ float cp_scan_add(float v) {
    v += CP_DPP(0.0f, v, 0x111, 0xF, 0xF);      // row_shr:1
    v += CP_DPP(0.0f, v, 0x112, 0xF, 0xF);      // row_shr:2
    v += CP_DPP(0.0f, v, 0x114, 0xF, 0xF);      // row_shr:4
    v += CP_DPP(0.0f, v, 0x118, 0xF, 0xF);      // row_shr:8
    v += CP_DPP(0.0f, v, 0x142, 0xA, 0xF);      // row_bcast:15 -> rows 1, 3
    v += CP_DPP(0.0f, v, 0x143, 0xC, 0xF);      // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ float cp_scan_mul(float v) {
    v *= CP_DPP(1.0f, v, 0x111, 0xF, 0xF);
    v *= CP_DPP(1.0f, v, 0x112, 0xF, 0xF);
    v *= CP_DPP(1.0f, v, 0x114, 0xF, 0xF);
    v *= CP_DPP(1.0f, v, 0x118, 0xF, 0xF);
    v *= CP_DPP(1.0f, v, 0x142, 0xA, 0xF);
    v *= CP_DPP(1.0f, v, 0x143, 0xC, 0xF);
    return v;
}
// lane i <- lane i - 1 (lane 0 <- `first`)
__device__ __forceinline__ float cp_shift_up(float v, float first) { return CP_DPP(first, v, 0x138, 0xF, 0xF); }   // wave_shr:1
__device__ __forceinline__ float cp_lane(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ float cp_sum(float v) { return cp_lane(cp_scan_add(v), 63); }

struct CompArgs {
    const float *sigmas, *rgbs, *deltas;
    const int32_t *rays;
    uint32_t M, N, C;
    float T_thresh;
    int is_ndc;
    // forward outputs
    float *weights_sum, *depth, *image;
    const float *nears, *fars;             // epilogue (both or neither)
    float *rgb_map, *depth_norm, *classes; // epilogue outputs: [N,3], [N], [N, C-3] (classes may be NULL)
    // backward inputs / outputs
    const float *g_ws, *g_image;           // legacy form: d/d weights_sum [N], d/d image [N,C]
    const float *g_rgb_map, *g_classes;    // epilogue form: d/d rgb_map [N,3], d/d classes [N,C-3] (each may be NULL)
    const float *ws_in, *image_in;
    float *g_sigmas, *g_rgbs;
    int epilogue, zero_fill;
};

// one sample's colour row into registers; CT > 0: compile-time C with 16-byte loads, CT == 0: runtime C, scalar loads
template <int CT>
__device__ __forceinline__ void cp_load_row(const float *__restrict__ rgbs, size_t p, uint32_t C, float (&c)[CT ? CT : CP_MAXC]) {
    if (CT > 0) {
#pragma unroll
        for (int q = 0; q < CT / 4; q++) {
            const float4 v = reinterpret_cast<const float4 *>(rgbs + p * CT)[q];
            c[4 * q] = v.x; c[4 * q + 1] = v.y; c[4 * q + 2] = v.z; c[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CP_MAXC; k++) c[k] = (uint32_t)k < C ? rgbs[p * C + k] : 0.0f;
    }
}

// persistent ray walk: wave gw takes rays gw, gw + nwaves, ...; header() hands out the wave-uniform header of ray n, then issues the
// load of the next one.  The caller's loop advances n (r.n += r.nwaves): doing it inside header() cost k_comp_fwd<8> 26 VGPRs.
struct CpWalk {
    const int32_t *rays;
    uint32_t N, nwaves, n;
    int32_t h0 = 0, h1 = 0, h2 = 0;        // header of ray n (after header(): of ray n + nwaves), one copy per lane
    uint32_t index, offset, steps;         // the current ray's, wave-uniform
    __device__ __forceinline__ CpWalk(const int32_t *rays_, uint32_t N_)
        : rays(rays_), N(N_), nwaves(gridDim.x * (CP_BLOCK / 64)), n(blockIdx.x * (CP_BLOCK / 64) + (threadIdx.x >> 6)) { load(n); }
    __device__ __forceinline__ void load(uint32_t m) { if (m < N) { h0 = rays[m * 3]; h1 = rays[m * 3 + 1]; h2 = rays[m * 3 + 2]; } }
    __device__ __forceinline__ void header() {
        index = (uint32_t)__builtin_amdgcn_readfirstlane(h0), offset = (uint32_t)__builtin_amdgcn_readfirstlane(h1), steps = (uint32_t)__builtin_amdgcn_readfirstlane(h2);
        load(n + nwaves);                  // next header in flight
    }
};

// carry into the next trip; whether the ray ends in this one (a sample of it is not live)
__device__ __forceinline__ void cp_carry(float &T, float incl) { T *= cp_lane(incl, 63); }
__device__ __forceinline__ void cp_carry(float &T, float &t, float incl, float tc) { cp_carry(T, incl); t = cp_lane(tc, 63); }
__device__ __forceinline__ bool cp_stopped(bool in, bool live) { return __ballot(in && !live) != 0ull; }
// zeros from `base` to the ray's end inside the buffer: behind an early stop, a dropped ray (:929), one without a range.  C == 0: sigmas only
__device__ __forceinline__ void cp_zero_tail(uint32_t offset, uint32_t steps, uint32_t base, uint32_t lane, uint32_t M, float *g_sigmas, float *g_rgbs, uint32_t C) {
    for (; base < steps; base += 64) {
        const uint32_t i = base + lane;
        const size_t p = (size_t)offset + i;
        if (i < steps && p < M) {
            g_sigmas[p] = 0.0f;
            for (uint32_t k = 0; k < C; k++) g_rgbs[p * C + k] = 0.0f;
        }
    }
}

template <int CT>
__global__ void __launch_bounds__(CP_BLOCK)
k_comp_fwd(CompArgs a) {
    // no contraction: which products the compiler fuses into an fma differs between the instantiations, and the runtime-C
    // kernel must give the bits of the compile-time-C one (a colour pointer's alignment must not change a result)
#pragma clang fp contract(off)
    constexpr int NC = CT ? CT : CP_MAXC;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t C = CT ? (uint32_t)CT : a.C;
    for (CpWalk r(a.rays, a.N); r.n < a.N; r.n += r.nwaves) {
        r.header();
        const uint32_t index = r.index, offset = r.offset, steps = r.steps;
        float T = 1.0f, t = 0.0f, ws = 0.0f, d = 0.0f;
        float acc[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) acc[k] = 0.0f;
        if (steps != 0 && offset + steps < a.M) {                                                   // :830
            for (uint32_t base = 0; base < steps; base += 64) {
                const uint32_t i = base + lane;
                const bool in = i < steps;
                const size_t p = (size_t)offset + min(i, steps - 1u);
                const float sg = a.sigmas[p];
                const float2 dd = *reinterpret_cast<const float2 *>(a.deltas + p * 4 + (a.is_ndc ? 2 : 0));
                float c[NC];
                cp_load_row<CT>(a.rgbs, p, C, c);
                const float alpha = in ? 1.0f - __expf(-sg * dd.x) : 0.0f;
                const float incl = cp_scan_mul(1.0f - alpha);
                const float Tb = T * cp_shift_up(incl, 1.0f);              // transmittance in front of the sample
                const float tc = t + cp_scan_add(in ? dd.y : 0.0f);        // t += deltas[1] (:857)
                // the serial loop reaches sample i iff every T after the samples before it stayed >= T_thresh (:862)
                const bool live = in && (i == 0u || Tb >= a.T_thresh);
                const float w = live ? alpha * Tb : 0.0f;
                ws += cp_sum(w);
                d += cp_sum(w * tc);
#pragma unroll
                for (int k = 0; k < NC; k++)
                    if (CT || (uint32_t)k < C) acc[k] += cp_sum(w * c[k]);
                cp_carry(T, t, incl, tc);
                if (cp_stopped(in, live) || T < a.T_thresh) break;
            }
        }
        // lane k holds channel k
        float mine = acc[0];
#pragma unroll
        for (int k = 1; k < NC; k++) mine = lane == (uint32_t)k ? acc[k] : mine;
        if (lane < C) a.image[(size_t)index * C + lane] = mine;
        if (lane == 0) { a.weights_sum[index] = ws; a.depth[index] = d; }
        if (a.epilogue) {
            // renderer.py:229-233: white background, depth normalised to [near, far]
            if (lane < 3u) a.rgb_map[(size_t)index * 3 + lane] = mine + (1.0f - ws);
            else if (lane < C && a.classes) a.classes[(size_t)index * (C - 3u) + (lane - 3u)] = mine;
            if (lane == 0) {
                const float nr = a.nears[index], fr = a.fars[index];
                a.depth_norm[index] = fmaxf(d - nr, 0.0f) / (fr - nr);
            }
        }
    }
}

template <int CT>
__global__ void __launch_bounds__(CP_BLOCK)
k_comp_bwd(CompArgs a) {
#pragma clang fp contract(off)                  // see k_comp_fwd
    constexpr int NC = CT ? CT : CP_MAXC;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t C = CT ? (uint32_t)CT : a.C;
    for (CpWalk r(a.rays, a.N); r.n < a.N; r.n += r.nwaves) {
        r.header();
        const uint32_t index = r.index, offset = r.offset, steps = r.steps;
        if (steps == 0) continue;
        uint32_t base = 0;
        if (offset + steps < a.M) {
            // per-ray gradients of the outputs, in lane k for channel k, then wave-uniform
            float gl = 0.0f, il = 0.0f;
            if (lane < C) {
                il = a.image_in[(size_t)index * C + lane];
                if (a.epilogue) {
                    if (lane < 3u) gl = a.g_rgb_map ? a.g_rgb_map[(size_t)index * 3 + lane] : 0.0f;
                    else gl = a.g_classes ? a.g_classes[(size_t)index * (C - 3u) + (lane - 3u)] : 0.0f;
                } else {
                    gl = a.g_image[(size_t)index * C + lane];
                }
            }
            float gim[NC], im[NC];
#pragma unroll
            for (int k = 0; k < NC; k++) { gim[k] = cp_lane(gl, k); im[k] = cp_lane(il, k); }
            float gws = a.g_ws ? a.g_ws[index] : 0.0f;
            // rgb_map = image[:3] + (1 - ws): d/d ws collects minus the three colour gradients
            if (a.epilogue) gws -= gim[0] + gim[1] + gim[2];
            const float ws_final = a.ws_in[index];
            const float tail = gws * (1.0f - ws_final);
            float T = 1.0f;
            float buf[NC];
#pragma unroll
            for (int k = 0; k < NC; k++) buf[k] = 0.0f;
            for (; base < steps; base += 64) {
                const uint32_t i = base + lane;
                const bool in = i < steps;
                const size_t p = (size_t)offset + min(i, steps - 1u);
                const float sg = a.sigmas[p];
                const float dt = a.deltas[p * 4 + (a.is_ndc ? 2 : 0)];
                float c[NC];
                cp_load_row<CT>(a.rgbs, p, C, c);
                const float alpha = in ? 1.0f - __expf(-sg * dt) : 0.0f;
                const float incl = cp_scan_mul(1.0f - alpha);
                const float Tb = T * cp_shift_up(incl, 1.0f);
                const float Ta = T * incl;                                  // T after the sample's update (:959)
                const float w = alpha * Tb;
                const bool live = in && Ta >= a.T_thresh;                   // :961 -- the stopping sample gets no gradient
                float gsum = 0.0f;
                float gc[NC];
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    if (CT || (uint32_t)k < C) {
                        const float run = buf[k] + cp_scan_add(w * c[k]);   // rgbs_buf after this sample (:957)
                        gsum += gim[k] * (Ta * c[k] - (im[k] - run));
                        gc[k] = live ? gim[k] * w : 0.0f;
                        buf[k] = cp_lane(run, 63);
                    } else {
                        gc[k] = 0.0f;
                    }
                }
                if (in && (live || a.zero_fill)) {
                    a.g_sigmas[p] = live ? dt * (gsum + tail) : 0.0f;
                    if (CT > 0) {
#pragma unroll
                        for (int q = 0; q < CT / 4; q++)
                            reinterpret_cast<float4 *>(a.g_rgbs + p * CT)[q] = make_float4(gc[4 * q], gc[4 * q + 1], gc[4 * q + 2], gc[4 * q + 3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < NC; k++)
                            if ((uint32_t)k < C) a.g_rgbs[p * C + k] = gc[k];
                    }
                }
                cp_carry(T, incl);
                if (cp_stopped(in, live)) { base += 64; break; }
            }
        }
        if (a.zero_fill) cp_zero_tail(offset, steps, base, lane, a.M, a.g_sigmas, a.g_rgbs, C);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// per-ray geometry terms on the training composite's weights: differentiable depth and the mip-NeRF 360 distortion
// ---------------------------------------------------------------------------------------------------------------------
// Samples, columns, live rule and trip structure are k_comp_fwd's (same alpha, same scans, so d has the bits of its depth).
// With w_i the composite weights, t_i the running depth parameter and R = far - near:
//   depth      = max(sum_i w_i t_i - near, 0) / R
//   distortion = (sum_ij w_i w_j |t_i - t_j| + 1/3 sum_i w_i^2 delta_i) / R
// t never decreases along a ray, so the pair term is 2 sum_i w_i (t_i W_<i - S_<i) with the exclusive prefixes W = sum w,
// S = sum w t: two more wave scans, no O(n^2) work.  The forward leaves (W, S, pair, self) of the whole ray in totals[index];
// the backward walks the ray front to back once more (the live set needs T, which only exists in that direction) and takes
// every "sum over the samples behind this one" as total minus inclusive prefix.  The prefixes of W and S are accumulated by the
// same instructions as the totals, so on the last live sample that difference is exactly 0.
// Unlike :961 the derivative is exact on every live sample, the stopping one included (the live set is held constant):
//   f_k = G_depth [d > near] t_k / R + G_dist (2 sum_j w_j |t_k - t_j| + 2/3 w_k delta_k) / R        (d loss / d w_k)
//   grad_sigma_i = delta_i (f_i T_{i+1} - sum_{k>i} f_k w_k),   T_{i+1} = T_i exp(-sigma_i delta_i)
// (T_{i+1} from the exponential, not as T_i - w_i: behind an opaque sample that difference is 0 in fp32).
// A ray whose R is not a positive finite number (a miss has near == far == FLT_MAX), a dropped ray and an empty one give 0 and
// zero gradients.
struct GeomArgs {
    const float *sigmas, *deltas;
    const int32_t *rays;
    const float *nears, *fars;
    uint32_t M, N;
    float T_thresh;
    int is_ndc;
    float *depth, *distortion;             // forward outputs [N]
    float *totals;                         // [N,4]: written by the forward, read by the backward
    const float *g_depth, *g_dist;         // [N] each, either may be NULL (zero)
    float *g_sigmas;                       // [M]
};

__device__ __forceinline__ bool cp_range_ok(float R) { return R > 0.0f && R <= 3.402823466e+38f; }

__global__ void __launch_bounds__(CP_BLOCK)
k_geom_fwd(GeomArgs a) {
#pragma clang fp contract(off)                  // see k_comp_fwd
    const uint32_t lane = threadIdx.x & 63u;
    for (CpWalk r(a.rays, a.N); r.n < a.N; r.n += r.nwaves) {
        r.header();
        const uint32_t index = r.index, offset = r.offset, steps = r.steps;
        const float nr = a.nears[index], R = a.fars[index] - nr;
        float T = 1.0f, t = 0.0f, W = 0.0f, S = 0.0f, P = 0.0f, Q = 0.0f;
        const bool ok = steps != 0 && offset + steps < a.M && cp_range_ok(R);
        if (ok) {
            for (uint32_t base = 0; base < steps; base += 64) {
                const uint32_t i = base + lane;
                const bool in = i < steps;
                const size_t p = (size_t)offset + min(i, steps - 1u);
                const float sg = a.sigmas[p];
                const float2 dd = *reinterpret_cast<const float2 *>(a.deltas + p * 4 + (a.is_ndc ? 2 : 0));
                const float alpha = in ? 1.0f - __expf(-sg * dd.x) : 0.0f;
                const float incl = cp_scan_mul(1.0f - alpha);
                const float Tb = T * cp_shift_up(incl, 1.0f);
                const float tc = t + cp_scan_add(in ? dd.y : 0.0f);
                const bool live = in && (i == 0u || Tb >= a.T_thresh);
                const float w = live ? alpha * Tb : 0.0f;
                const float wi = cp_scan_add(w), si = cp_scan_add(w * tc);
                const float Wex = W + cp_shift_up(wi, 0.0f), Sex = S + cp_shift_up(si, 0.0f);   // over the samples in front
                P += cp_sum(w * (tc * Wex - Sex));
                Q += cp_sum(w * w * dd.x);
                W += cp_lane(wi, 63);
                S += cp_lane(si, 63);
                cp_carry(T, t, incl, tc);
                if (cp_stopped(in, live) || T < a.T_thresh) break;
            }
        }
        // lane k holds total k
        const float mine = lane == 0u ? W : lane == 1u ? S : lane == 2u ? P : Q;
        if (lane < 4u) a.totals[(size_t)index * 4 + lane] = mine;
        if (lane == 0) {
            a.depth[index] = ok ? fmaxf(S - nr, 0.0f) / R : 0.0f;
            a.distortion[index] = ok ? (2.0f * P + Q / 3.0f) / R : 0.0f;
        }
    }
}

__global__ void __launch_bounds__(CP_BLOCK)
k_geom_bwd(GeomArgs a) {
#pragma clang fp contract(off)                  // see k_comp_fwd
    const uint32_t lane = threadIdx.x & 63u;
    for (CpWalk r(a.rays, a.N); r.n < a.N; r.n += r.nwaves) {
        r.header();
        const uint32_t index = r.index, offset = r.offset, steps = r.steps;
        if (steps == 0) continue;
        uint32_t base = 0;
        const float nr = a.nears[index], R = a.fars[index] - nr;
        if (offset + steps < a.M && cp_range_ok(R)) {
            const float tl = lane < 4u ? a.totals[(size_t)index * 4 + lane] : 0.0f;
            const float Wt = cp_lane(tl, 0), St = cp_lane(tl, 1), Pt = cp_lane(tl, 2), Qt = cp_lane(tl, 3);
            const float gd = a.g_depth ? a.g_depth[index] : 0.0f, gx = a.g_dist ? a.g_dist[index] : 0.0f;
            const float cD = St > nr ? gd / R : 0.0f;                       // the clamp of the depth passes a gradient iff d > near
            const float cX = gx / R;
            // sum_k f_k w_k over the ray: the depth part is cD * d, the distortion numerator is homogeneous of degree 2 in w
            const float Ft = cD * St + cX * (2.0f * (2.0f * Pt + Qt / 3.0f));
            float T = 1.0f, t = 0.0f, W = 0.0f, S = 0.0f, F = 0.0f;
            for (; base < steps; base += 64) {
                const uint32_t i = base + lane;
                const bool in = i < steps;
                const size_t p = (size_t)offset + min(i, steps - 1u);
                const float sg = a.sigmas[p];
                const float2 dd = *reinterpret_cast<const float2 *>(a.deltas + p * 4 + (a.is_ndc ? 2 : 0));
                const float om = in ? __expf(-sg * dd.x) : 1.0f;
                const float alpha = 1.0f - om;
                const float incl = cp_scan_mul(1.0f - alpha);               // (1 - alpha, not om: the forward's bits, the same live set)
                const float Tb = T * cp_shift_up(incl, 1.0f);
                const float tc = t + cp_scan_add(in ? dd.y : 0.0f);
                const bool live = in && (i == 0u || Tb >= a.T_thresh);
                const float w = live ? alpha * Tb : 0.0f;
                const float wi = cp_scan_add(w), si = cp_scan_add(w * tc);
                const float Wex = W + cp_shift_up(wi, 0.0f), Sex = S + cp_shift_up(si, 0.0f);
                const float Win = W + wi, Sin = S + si;
                // sum_j w_j |t_k - t_j|: the samples in front, then the samples behind (total - inclusive prefix)
                const float A = (tc * Wex - Sex) + ((St - Sin) - tc * (Wt - Win));
                const float f = cD * tc + cX * (2.0f * A + (2.0f / 3.0f) * (w * dd.x));
                const float fi = F + cp_scan_add(f * w);
                if (in) a.g_sigmas[p] = live ? dd.x * (f * (Tb * om) - (Ft - fi)) : 0.0f;
                W += cp_lane(wi, 63);
                S += cp_lane(si, 63);
                F = cp_lane(fi, 63);
                cp_carry(T, t, incl, tc);
                if (cp_stopped(in, live) || T < a.T_thresh) { base += 64; break; }
            }
        }
        cp_zero_tail(offset, steps, base, lane, a.M, a.g_sigmas, nullptr, 0u);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// position gradients of the samples back to their ray: xyz_i = o + t_i d  ->  d/d o = sum_i g_i, d/d d = sum_i t_i g_i
// ---------------------------------------------------------------------------------------------------------------------
// The ray walk, the "offset + steps < M" drop test and the running parameter (sum scan of deltas[:, 1], carried across trips)
// are k_comp_fwd's.  The march emits deltas[:, 1] = t_next - last_t with last_t starting at the ray's first parameter, so that
// running sum is the parameter BEHIND sample i measured from the start: with nears given, the sample's own parameter
// t_i = near + sum_{j <= i} deltas[j, 1] - deltas[i, 0] is used (where the march put xyz_i); without, the running sum itself.
// t_i, the samples of a ray and their count are constants of differentiation.  Dropped and empty rays get zeros.
struct PosArgs {
    const float *g_xyzs, *deltas, *nears;
    const int32_t *rays;
    uint32_t M, N;
    float *g_o, *g_d;                      // [N,3] each
};

__global__ void __launch_bounds__(CP_BLOCK)
k_rays_pos_bwd(PosArgs a) {
#pragma clang fp contract(off)                  // see k_comp_fwd
    const uint32_t lane = threadIdx.x & 63u;
    for (CpWalk r(a.rays, a.N); r.n < a.N; r.n += r.nwaves) {
        r.header();
        const uint32_t index = r.index, offset = r.offset, steps = r.steps;
        float t = 0.0f, so[3] = {0.0f, 0.0f, 0.0f}, sd[3] = {0.0f, 0.0f, 0.0f};
        if (steps != 0 && offset + steps < a.M) {
            const float t0 = a.nears ? a.nears[index] : 0.0f;
            for (uint32_t base = 0; base < steps; base += 64) {
                const uint32_t i = base + lane;
                const bool in = i < steps;
                const size_t p = (size_t)offset + min(i, steps - 1u);
                const float2 dd = *reinterpret_cast<const float2 *>(a.deltas + p * 4);
                const float tc = t + cp_scan_add(in ? dd.y : 0.0f);        // k_comp_fwd's t
                const float ti = a.nears ? t0 + (tc - dd.x) : tc;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float g = in ? a.g_xyzs[p * 3 + k] : 0.0f;
                    so[k] += cp_sum(g);
                    sd[k] += cp_sum(ti * g);
                }
                t = cp_lane(tc, 63);
            }
        }
        // lanes 0..2: d/d origin, lanes 3..5: d/d direction
        const float mine = lane == 0u ? so[0] : lane == 1u ? so[1] : lane == 2u ? so[2] : lane == 3u ? sd[0] : lane == 4u ? sd[1] : sd[2];
        if (lane < 3u) a.g_o[(size_t)index * 3 + lane] = mine;
        else if (lane < 6u) a.g_d[(size_t)index * 3 + (lane - 3u)] = mine;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// reconstruction loss: value and gradient in one pass
// ---------------------------------------------------------------------------------------------------------------------
struct LossArgs {
    const float *rgb_map, *classes;       // [N,3], [N,nc] (classes may be NULL: MSE only)
    const float *target_rgb;              // [P,3]
    const int64_t *target_cls;            // [P] (may be NULL)
    const int64_t *pix;                   // [N] rows of the targets (NULL: row n)
    uint32_t N, nc;
    float ce_lambda, factor;
    const float *scale;                   // device scalar (loss scale) or NULL
    float *g_rgb, *g_classes;             // [N,3], [N,nc]
    float *partials;                      // [blocks][2]
    float *out;                           // [3]: scaled total, mse, ce (both unscaled)
    uint32_t nblocks;
};
struct WLossArgs : LossArgs {             // ... with a weight per ray (importance sampling: error_map.hip)
    const float *ray_weight;              // [N] or NULL: 1
    float *ray_err;                       // [N] or NULL
};
struct ELossArgs : WLossArgs {            // ... and a gain per frame and colour channel (per-frame exposure and white balance)
    const float *exposure;                // [F,3] log2 gains
    const int32_t *seg_frame;             // [N / K]
    uint32_t F, K;
    float *term;                          // [N,3]
};

// the block's (mse, ce) to partials[blockIdx.x]; every thread of the block calls it
__device__ __forceinline__ void cp_loss_partials(const LossArgs &a, float mse, float ce, float (&red)[2][CP_BLOCK / 64]) {
    const float v[2] = {mse, ce};
    nsr_block_sum_stage(v, red);
    if (threadIdx.x == 0) {
        a.partials[blockIdx.x * 2] = nsr_block_sum_col<CP_BLOCK / 64>(red[0]);
        a.partials[blockIdx.x * 2 + 1] = nsr_block_sum_col<CP_BLOCK / 64>(red[1]);
    }
}

// The per-ray pass of the three losses, one body; Args says which one.
//   LossArgs    the plain loss.
//   WLossArgs   every per-ray term of value and gradient times ray_weight[n], the means still over N; ray_err (optional) gets
//               the ray's unweighted sum of squared colour differences, the fp32 differences' squares summed exactly in fp64
//               and rounded once.
//   ELossArgs   ray n of segment n / K, frame f = seg_frame[n / K], is modelled to have been observed as p = rgb_map *
//               exp2(exposure[f]) (a frame outside [0, F) reads no exposure row: gain 1); the difference, the value and the
//               per-ray error are those of p, the gradient towards rgb_map is the gradient towards p times the gain, and term =
//               (d loss / d p) * p, staged per ray and channel, is what the exposure segment sums below add up per frame (d p /
//               d exposure = ln2 * p).  p is a product rounded on its own (__fmul_rn: a contraction into the difference would
//               leave term without its operand).
// The operand-shape rule: a factor that a loss does not have is the constant 1 in the one expression all three share, so a weight
// of exactly 1 and an exposure of 0 (gain exactly 1) give every operation the operands it has in the loss without them -- (1 *
// df) * df + mse contracts like df * df + mse, 1 * (lse - logit) + ce like (lse - logit) + ce -- and the compiler folds the
// constant away: the plain kernel has no weight multiply, no fp64 error and no ray_err store, the weighted one no gain and no
// term store.  All three write partials for the same final pass.
template <typename Args>
__global__ void __launch_bounds__(CP_BLOCK)
k_recon_loss(Args a) {
    constexpr bool WEIGHTED = std::is_base_of_v<WLossArgs, Args>, EXPOSURE = std::is_base_of_v<ELossArgs, Args>;
    __shared__ float red[2][CP_BLOCK / 64];
    const float s = (a.scale ? a.scale[0] : 1.0f) * a.factor;
    const float inv3n = 1.0f / (3.0f * (float)a.N), invn = 1.0f / (float)a.N;
    float mse = 0.0f, ce = 0.0f;
    for (uint32_t n = blockIdx.x * CP_BLOCK + threadIdx.x; n < a.N; n += gridDim.x * CP_BLOCK) {
        const size_t row = a.pix ? (size_t)a.pix[n] : (size_t)n;
        const float w = [&] { if constexpr (WEIGHTED) return a.ray_weight ? a.ray_weight[n] : 1.0f; else return 1.0f; }();
        uint32_t f = 0u;
        bool named = false;
        if constexpr (EXPOSURE) { f = (uint32_t)a.seg_frame[n / a.K]; named = f < a.F; }
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float gain = 1.0f, p = a.rgb_map[(size_t)n * 3 + k];
            if constexpr (EXPOSURE) {
                gain = named ? exp2f(a.exposure[(size_t)f * 3 + k]) : 1.0f;
                p = __fmul_rn(p, gain);
            }
            const float df = p - a.target_rgb[row * 3 + k];
            const float wdf = w * df;
            mse += wdf * df;
            if constexpr (WEIGHTED) e += (double)df * (double)df;
            const float gp = 2.0f * df * inv3n * s * w;
            a.g_rgb[(size_t)n * 3 + k] = gp * gain;
            if constexpr (EXPOSURE) a.term[(size_t)n * 3 + k] = gp * p;
        }
        if constexpr (WEIGHTED) { if (a.ray_err) a.ray_err[n] = (float)e; }
        if (a.classes && a.nc) {
            // nn.CrossEntropyLoss (trainers/base.py:281): logsumexp(logits) - logits[label], mean over the rays
            const float *lg = a.classes + (size_t)n * a.nc;
            const uint32_t label = (uint32_t)a.target_cls[row];
            float mx = lg[0];
            for (uint32_t k = 1; k < a.nc; k++) mx = fmaxf(mx, lg[k]);
            float se = 0.0f;
            for (uint32_t k = 0; k < a.nc; k++) se += expf(lg[k] - mx);
            const float lse = mx + logf(se);
            ce += w * (lse - lg[min(label, a.nc - 1u)]);
            const float gk = a.ce_lambda * invn * s * w;
            for (uint32_t k = 0; k < a.nc; k++) a.g_classes[(size_t)n * a.nc + k] = (expf(lg[k] - lse) - (k == label ? 1.0f : 0.0f)) * gk;
        }
    }
    cp_loss_partials(a, mse, ce, red);
}

__global__ void __launch_bounds__(CP_BLOCK)
k_recon_loss_final(LossArgs a) {
    __shared__ float red[2][CP_BLOCK / 64];
    float v[2] = {0.0f, 0.0f};              // mse, ce
    for (uint32_t b = threadIdx.x; b < a.nblocks; b += CP_BLOCK) { v[0] += a.partials[b * 2]; v[1] += a.partials[b * 2 + 1]; }
    nsr_block_sum_stage(v, red);
    if (threadIdx.x == 0) {
        const float m = nsr_block_sum_col<CP_BLOCK / 64>(red[0]) / (3.0f * (float)a.N);
        const float c = nsr_block_sum_col<CP_BLOCK / 64>(red[1]) / (float)a.N * a.ce_lambda;
        const float s = (a.scale ? a.scale[0] : 1.0f) * a.factor;
        a.out[0] = (m + c) * s;
        a.out[1] = m;
        a.out[2] = c;
    }
}

// the per-ray pass of the loss that Args names, then the final pass they share
template <typename Args>
static void cp_loss_launch(const Args &a, hipStream_t s) {
    hipLaunchKernelGGL(k_recon_loss<Args>, dim3(a.nblocks), dim3(CP_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_recon_loss_final, dim3(1), dim3(CP_BLOCK), 0, s, static_cast<const LossArgs &>(a));
}

// grad_exposure[f] = ln2 * sum of term over the rays of the segments naming f, in fp64: the three parts of seg_sum.h with three
// sums per segment, seg_partials [S][B][3]; the frame's sum times ln2 is rounded to fp32 once.
struct ExpSegArgs {
    const float *term;                    // [S * K, 3]
    const int32_t *seg_frame;
    uint32_t F, S, K, B;
    double *seg_partials;
};

__device__ __forceinline__ auto cp_exposure_terms(const float *__restrict__ term) {
    return [=](uint32_t, size_t n0) {
        const float *t = term + n0 * 3;
        return [=](uint32_t k, double (&acc)[3]) {
#pragma unroll
            for (int c = 0; c < 3; c++) acc[c] += (double)t[(size_t)k * 3 + c];
        };
    };
}

__global__ void __launch_bounds__(SEG_BLOCK)
k_exposure_seg_thread(ExpSegArgs a) {
    seg_sum_thread<3>(a.seg_frame, a.F, a.S, a.K, a.seg_partials, cp_exposure_terms(a.term));
}

__global__ void __launch_bounds__(SEG_BLOCK)
k_exposure_seg_block(ExpSegArgs a) {
    __shared__ double red[3][SEG_BLOCK / 64];
    seg_sum_block<3>(a.seg_frame, a.F, a.K, a.B, a.seg_partials, red, cp_exposure_terms(a.term));
}

__global__ void __launch_bounds__(64)
k_exposure_final(const double *__restrict__ seg_partials, const int32_t *__restrict__ seg_frame, uint32_t S, uint32_t B,
                 float *__restrict__ grad_exposure) {
    const int32_t f = (int32_t)blockIdx.x;
    const double acc = seg_frame_sum(seg_frame, S, B, seg_partials, 3u, 0u, 3u, [f](int32_t named) { return named == f; });
    if (threadIdx.x < 3u) grad_exposure[(size_t)f * 3 + threadIdx.x] = (float)(0.6931471805599453 * acc);
}

// 256 CUs x 8 blocks of 4 waves: the persistent grid of the ray kernels, the cap of the loss grid and with it the loss workspace
static constexpr uint32_t CP_MAX_BLOCKS = 2048u;
static uint32_t cp_grid(uint32_t N) {       // fewer blocks when there are fewer rays
    const uint32_t want = nsr_div_up(N, CP_BLOCK / 64);
    return want < CP_MAX_BLOCKS ? (want ? want : 1u) : CP_MAX_BLOCKS;
}

template <bool BWD>
static int cp_launch(const CompArgs &a, hipStream_t s) {
    const dim3 g(cp_grid(a.N)), b(CP_BLOCK);
    const bool al16 = (((uintptr_t)a.rgbs | (uintptr_t)(BWD ? a.g_rgbs : a.rgbs)) & 15u) == 0;
    if (a.C == 8 && al16) {
        if (BWD) hipLaunchKernelGGL((k_comp_bwd<8>), g, b, 0, s, a); else hipLaunchKernelGGL((k_comp_fwd<8>), g, b, 0, s, a);
    } else if (a.C == 4 && al16) {
        if (BWD) hipLaunchKernelGGL((k_comp_bwd<4>), g, b, 0, s, a); else hipLaunchKernelGGL((k_comp_fwd<4>), g, b, 0, s, a);
    } else {
        if (BWD) hipLaunchKernelGGL((k_comp_bwd<0>), g, b, 0, s, a); else hipLaunchKernelGGL((k_comp_fwd<0>), g, b, 0, s, a);
    }
    return nsr_launch_status();
}

// what the four composite entry points share: the common pointers (an entry point checks its own first: the same status), the range
// of C (from 1, or from 3 with the epilogue), deltas aligned where the kernel loads delta pairs (the backwards read 4 bytes), the fields
static int cp_args(CompArgs &a, const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, uint32_t M, uint32_t N,
                   uint32_t C, float T_thresh, int is_ndc, uint32_t min_C, bool delta_pairs) {
    NSR_CHECK_PTR(sigmas); NSR_CHECK_PTR(rgbs); NSR_CHECK_PTR(deltas); NSR_CHECK_PTR(rays);
    if (C < min_C || C > CP_MAXC) return NSR_ERR_UNSUPPORTED;
    if (delta_pairs && ((uintptr_t)deltas & 7u) != 0) return NSR_ERR_INVALID_ARG;
    a = {};
    a.sigmas = sigmas; a.rgbs = rgbs; a.deltas = deltas; a.rays = rays; a.M = M; a.N = N; a.C = C; a.T_thresh = T_thresh; a.is_ndc = is_ndc;
    return NSR_OK;
}

static int cp_geom_args(GeomArgs &a, const float *sigmas, const float *deltas, const int32_t *rays, const float *nears, const float *fars,
                        uint32_t M, uint32_t N, float T_thresh, int is_ndc) {
    NSR_CHECK_PTR(sigmas); NSR_CHECK_PTR(deltas); NSR_CHECK_PTR(rays); NSR_CHECK_PTR(nears); NSR_CHECK_PTR(fars);
    if (((uintptr_t)deltas & 7u) != 0) return NSR_ERR_INVALID_ARG;
    a = {};
    a.sigmas = sigmas; a.deltas = deltas; a.rays = rays; a.nears = nears; a.fars = fars; a.M = M; a.N = N; a.T_thresh = T_thresh; a.is_ndc = is_ndc;
    return NSR_OK;
}

extern "C" {

int nsr_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays,
                                     uint32_t M, uint32_t N, uint32_t C, float T_thresh, int is_ndc, float *weights_sum,
                                     float *depth, float *image, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(weights_sum); NSR_CHECK_PTR(depth); NSR_CHECK_PTR(image);
    CompArgs a;
    if (const int e = cp_args(a, sigmas, rgbs, deltas, rays, M, N, C, T_thresh, is_ndc, 1u, true)) return e;
    a.weights_sum = weights_sum; a.depth = depth; a.image = image;
    return cp_launch<false>(a, (hipStream_t)stream);
}

int nsr_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image, const float *sigmas,
                                      const float *rgbs, const float *deltas, const int32_t *rays, int is_ndc,
                                      const float *weights_sum, const float *image, uint32_t M, uint32_t N, uint32_t C,
                                      float T_thresh, float *grad_sigmas, float *grad_rgbs, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(grad_weights_sum); NSR_CHECK_PTR(grad_image); NSR_CHECK_PTR(weights_sum); NSR_CHECK_PTR(image);
    NSR_CHECK_PTR(grad_sigmas); NSR_CHECK_PTR(grad_rgbs);
    CompArgs a;
    if (const int e = cp_args(a, sigmas, rgbs, deltas, rays, M, N, C, T_thresh, is_ndc, 1u, false)) return e;
    a.g_ws = grad_weights_sum; a.g_image = grad_image; a.ws_in = weights_sum; a.image_in = image;
    a.g_sigmas = grad_sigmas; a.g_rgbs = grad_rgbs; a.zero_fill = 1;
    return cp_launch<true>(a, (hipStream_t)stream);
}

int nsr_render_train_forward(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, const float *nears,
                             const float *fars, uint32_t M, uint32_t N, uint32_t C, float T_thresh, float *weights_sum,
                             float *depth, float *image, float *rgb_map, float *depth_norm, float *classes, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(nears); NSR_CHECK_PTR(fars);
    NSR_CHECK_PTR(weights_sum); NSR_CHECK_PTR(depth); NSR_CHECK_PTR(image); NSR_CHECK_PTR(rgb_map); NSR_CHECK_PTR(depth_norm);
    CompArgs a;
    if (const int e = cp_args(a, sigmas, rgbs, deltas, rays, M, N, C, T_thresh, 0, 3u, true)) return e;
    if (C > 3 && classes == nullptr) return NSR_ERR_INVALID_ARG;
    a.weights_sum = weights_sum; a.depth = depth; a.image = image; a.nears = nears; a.fars = fars; a.rgb_map = rgb_map;
    a.depth_norm = depth_norm; a.classes = classes; a.epilogue = 1;
    return cp_launch<false>(a, (hipStream_t)stream);
}

int nsr_render_train_backward(const float *grad_rgb_map, const float *grad_classes, const float *grad_weights_sum, const float *sigmas,
                              const float *rgbs, const float *deltas, const int32_t *rays, const float *weights_sum,
                              const float *image, uint32_t M, uint32_t N, uint32_t C, float T_thresh, float *grad_sigmas,
                              float *grad_rgbs, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(weights_sum); NSR_CHECK_PTR(image); NSR_CHECK_PTR(grad_sigmas); NSR_CHECK_PTR(grad_rgbs);
    CompArgs a;
    if (const int e = cp_args(a, sigmas, rgbs, deltas, rays, M, N, C, T_thresh, 0, 3u, false)) return e;
    a.g_ws = grad_weights_sum; a.g_rgb_map = grad_rgb_map; a.g_classes = grad_classes; a.ws_in = weights_sum; a.image_in = image;
    a.g_sigmas = grad_sigmas; a.g_rgbs = grad_rgbs; a.zero_fill = 1; a.epilogue = 1;
    return cp_launch<true>(a, (hipStream_t)stream);
}

int nsr_ray_geometry_forward(const float *sigmas, const float *deltas, const int32_t *rays, const float *nears, const float *fars,
                             uint32_t M, uint32_t N, float T_thresh, int is_ndc, float *depth, float *distortion, float *totals,
                             nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(depth); NSR_CHECK_PTR(distortion); NSR_CHECK_PTR(totals);
    GeomArgs a;
    if (const int e = cp_geom_args(a, sigmas, deltas, rays, nears, fars, M, N, T_thresh, is_ndc)) return e;
    a.depth = depth; a.distortion = distortion; a.totals = totals;
    hipLaunchKernelGGL(k_geom_fwd, dim3(cp_grid(N)), dim3(CP_BLOCK), 0, (hipStream_t)stream, a);
    return nsr_launch_status();
}

int nsr_ray_geometry_backward(const float *grad_depth, const float *grad_distortion, const float *sigmas, const float *deltas,
                              const int32_t *rays, const float *nears, const float *fars, const float *totals, uint32_t M,
                              uint32_t N, float T_thresh, int is_ndc, float *grad_sigmas, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(totals); NSR_CHECK_PTR(grad_sigmas);
    GeomArgs a;
    if (const int e = cp_geom_args(a, sigmas, deltas, rays, nears, fars, M, N, T_thresh, is_ndc)) return e;
    a.totals = const_cast<float *>(totals); a.g_depth = grad_depth; a.g_dist = grad_distortion; a.g_sigmas = grad_sigmas;
    hipLaunchKernelGGL(k_geom_bwd, dim3(cp_grid(N)), dim3(CP_BLOCK), 0, (hipStream_t)stream, a);
    return nsr_launch_status();
}

int nsr_rays_position_backward(const float *grad_xyzs, const float *deltas, const int32_t *rays, const float *nears, uint32_t M,
                                uint32_t N, int is_ndc, float *grad_rays_o, float *grad_rays_d, nsr_stream_t stream) {
    if (is_ndc) return NSR_ERR_UNSUPPORTED;     // an NDC sample is not o + t d of the rays the march was given
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(grad_xyzs); NSR_CHECK_PTR(deltas); NSR_CHECK_PTR(rays); NSR_CHECK_PTR(grad_rays_o); NSR_CHECK_PTR(grad_rays_d);
    if (((uintptr_t)deltas & 7u) != 0) return NSR_ERR_INVALID_ARG;
    PosArgs a;
    a.g_xyzs = grad_xyzs; a.deltas = deltas; a.nears = nears; a.rays = rays; a.M = M; a.N = N; a.g_o = grad_rays_o; a.g_d = grad_rays_d;
    hipLaunchKernelGGL(k_rays_pos_bwd, dim3(cp_grid(N)), dim3(CP_BLOCK), 0, (hipStream_t)stream, a);
    return nsr_launch_status();
}

uint64_t nsr_recon_loss_workspace_bytes(uint32_t N) {
    (void)N;
    return (uint64_t)CP_MAX_BLOCKS * 2 * sizeof(float);
}

// the checks and the argument block that the plain and the weighted loss share
static int cp_loss_args(LossArgs &a, const float *rgb_map, const float *classes, uint32_t N, uint32_t nc, const float *target_rgb,
                        const int64_t *target_cls, const int64_t *pix, float ce_lambda, float factor, const float *scale,
                        float *grad_rgb_map, float *grad_classes, float *loss_out, void *workspace) {
    NSR_CHECK_PTR(loss_out);
    if (N == 0) return NSR_ERR_INVALID_ARG;
    NSR_CHECK_PTR(rgb_map); NSR_CHECK_PTR(target_rgb); NSR_CHECK_PTR(grad_rgb_map); NSR_CHECK_PTR(workspace);
    const bool with_ce = classes != nullptr && nc > 0 && ce_lambda != 0.0f;
    if (with_ce && (target_cls == nullptr || grad_classes == nullptr)) return NSR_ERR_INVALID_ARG;
    a.rgb_map = rgb_map; a.classes = with_ce ? classes : nullptr; a.target_rgb = target_rgb; a.target_cls = target_cls; a.pix = pix;
    a.N = N; a.nc = with_ce ? nc : 0u; a.ce_lambda = ce_lambda; a.factor = factor; a.scale = scale;
    a.g_rgb = grad_rgb_map; a.g_classes = grad_classes; a.partials = (float *)workspace; a.out = loss_out;
    uint32_t nb = nsr_div_up(N, CP_BLOCK);
    if (nb > CP_MAX_BLOCKS) nb = CP_MAX_BLOCKS;
    a.nblocks = nb;
    return NSR_OK;
}

int nsr_recon_loss(const float *rgb_map, const float *classes, uint32_t N, uint32_t nc, const float *target_rgb,
                   const int64_t *target_cls, const int64_t *pix, float ce_lambda, float factor, const float *scale,
                   float *grad_rgb_map, float *grad_classes, float *loss_out, void *workspace, nsr_stream_t stream) {
    LossArgs a;
    if (const int e = cp_loss_args(a, rgb_map, classes, N, nc, target_rgb, target_cls, pix, ce_lambda, factor, scale, grad_rgb_map,
                                   grad_classes, loss_out, workspace)) return e;
    cp_loss_launch(a, (hipStream_t)stream);
    return nsr_launch_status();
}

int nsr_recon_loss_weighted(const float *rgb_map, const float *classes, uint32_t N, uint32_t nc, const float *target_rgb,
                            const int64_t *target_cls, const int64_t *pix, const float *ray_weight, float ce_lambda, float factor,
                            const float *scale, float *grad_rgb_map, float *grad_classes, float *ray_err, float *loss_out,
                            void *workspace, nsr_stream_t stream) {
    WLossArgs a;
    if (const int e = cp_loss_args(a, rgb_map, classes, N, nc, target_rgb, target_cls, pix, ce_lambda, factor, scale, grad_rgb_map,
                                   grad_classes, loss_out, workspace)) return e;
    a.ray_weight = ray_weight; a.ray_err = ray_err;
    cp_loss_launch(a, (hipStream_t)stream);
    return nsr_launch_status();
}

// the exposure loss's workspace: the loss's block partials, then seg_partials [S][B][3] f64, then term [N,3] f32
static constexpr uint64_t CP_EXP_WS_SEG = (uint64_t)CP_MAX_BLOCKS * 2 * sizeof(float);
static_assert(CP_EXP_WS_SEG % 8 == 0, "seg_partials are doubles");
static uint64_t cp_exp_ws_term(uint32_t S, uint32_t K) {
    return CP_EXP_WS_SEG + (uint64_t)S * seg_blocks(K) * 3 * sizeof(double);
}

uint64_t nsr_recon_loss_exposure_workspace_bytes(uint32_t N, uint32_t F, uint32_t S, uint32_t K) {
    (void)F;
    return (cp_exp_ws_term(S, K) + (uint64_t)N * 3 * sizeof(float) + 7u) & ~(uint64_t)7u;
}

int nsr_recon_loss_exposure(const float *rgb_map, const float *classes, uint32_t N, uint32_t nc, const float *target_rgb,
                            const int64_t *target_cls, const int64_t *pix, const float *ray_weight, const float *exposure, uint32_t F,
                            const int32_t *seg_frame, uint32_t S, uint32_t K, float ce_lambda, float factor, const float *scale,
                            float *grad_rgb_map, float *grad_classes, float *grad_exposure, float *ray_err, float *loss_out,
                            void *workspace, nsr_stream_t stream) {
    if (N == 0 || F == 0 || S == 0 || K == 0 || (uint64_t)S * K != (uint64_t)N) return NSR_ERR_INVALID_ARG;
    ELossArgs a;
    if (const int e = cp_loss_args(a, rgb_map, classes, N, nc, target_rgb, target_cls, pix, ce_lambda, factor, scale, grad_rgb_map,
                                   grad_classes, loss_out, workspace)) return e;
    NSR_CHECK_PTR(exposure); NSR_CHECK_PTR(seg_frame); NSR_CHECK_PTR(grad_exposure);
    if (F > 0x7fffffffu || !seg_sum_ok(N, S, K, workspace)) return NSR_ERR_INVALID_ARG;
    const uint32_t B = seg_blocks(K);
    double *seg_partials = (double *)((char *)workspace + CP_EXP_WS_SEG);
    a.ray_weight = ray_weight; a.ray_err = ray_err;
    a.exposure = exposure; a.seg_frame = seg_frame; a.F = F; a.K = K;
    a.term = (float *)((char *)workspace + cp_exp_ws_term(S, K));
    cp_loss_launch(a, (hipStream_t)stream);
    seg_sum_launch(k_exposure_seg_thread, k_exposure_seg_block, S, K, (hipStream_t)stream,
                   ExpSegArgs{a.term, seg_frame, F, S, K, B, seg_partials});
    hipLaunchKernelGGL(k_exposure_final, dim3(F), dim3(64), 0, (hipStream_t)stream, (const double *)seg_partials, seg_frame, S, B,
                       grad_exposure);
    return nsr_launch_status();
}

}   // extern "C"
