// Streaming render for gfx950: occupancy march -> hash encode -> density / colour / class MLPs on MFMA -> composite, in
// ONE kernel per frame with no sample buffer.  Two compile-time composites:
//   NSR_STREAM_INFER  the inference composite (reference: renderer.py:237-293, up to max_steps host iterations of
//                     march_rays / model / composite_rays; here: Renderer.render_test_fused);
//   NSR_STREAM_TRAIN  the training composite (raymarching.cu:806-879, k_comp_fwd of composite.hip) with render_train's
//                     epilogue (renderer.py:229-233) in the write-out: what Renderer.render_train gives without autograd
//                     (Renderer.render_train_fused).
//
// A wave owns 16 ray SLOTS.  Lane (s = lane & 15, g = lane >> 4) works on the current sample of slot s with the lane
// layout of k_field_fwd (field.hip), so the encode output is the MFMA B fragment as it stands.  The ray's state is in
// registers, replicated over the four g lanes of its slot: every lane of a slot runs the same serial march
// (rm_probe.h: the positions are bit for bit those of every other march here), lane g accumulates channels 4g..4g+3 of
// the pixel.  One iteration: every live slot advances to its next occupied sample, the wave shades the 16 samples, each
// slot composites its own with the arithmetic of k_composite_infer (raymarch_infer.hip) or of k_comp_fwd.  A ray that stopped
// (T < T_thresh), reached `far` or took max_steps samples writes its pixel, and the slot takes the next ray of the wave's
// contiguous piece of the work list (wave-uniform cursor + rank among the slots that ask): no atomics, no waiting on
// another wave, nothing dropped.  Work is proportional to the samples that contribute: what lies behind the first
// opaque surface is neither gathered nor shaded.
#include "field_common.h"
#include "rm_probe.h"

struct RenderInferArgs {
    FieldArgs f;                 // tables, params, bbox, density_scale, C_ch, level table (xyzs / sigmas / rgbs unused)
    const float *rays_o, *rays_d;
    const uint32_t *order;       // optional [N]: the ray handled k-th
    const float *nears, *fars;
    const uint8_t *grid;
    uint32_t N, rays_per_wave;
    float bound, dt_gamma;
    uint32_t max_steps, C, H;
    float T_thresh;
    float *weights_sum, *depth, *image;
    uint32_t *stats;             // optional {samples shaded, rays finished}
    // read by the instantiations other than NSR_STREAM_INFER only (each optional)
    int32_t *n_composited;       // [N]: samples accumulated for the ray
    float *rgb_map, *depth_norm, *classes;   // render_train's outputs: [N,3], [N], [N, C_ch - 3]
};

// The inference composite with the optional outputs.  NSR_STREAM_INFER itself has none of them, so that render_test_fused's
// kernel is instruction for instruction what it was before the training mode existed.
#define RI_STREAM_INFER_EXTRAS 2

template <typename TT, int CD, int MODE>
__global__ void __launch_bounds__(256)
k_render_infer(RenderInferArgs a) {
    constexpr bool TRAIN = MODE == NSR_STREAM_TRAIN;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    short *wl = reinterpret_cast<short *>(smem);
    NsrLevel *lds_lv = reinterpret_cast<NsrLevel *>(smem + FW_TOTAL * 2);
    field_build_fw<CD, false>(wl, a.f.params);
    if (threadIdx.x < 16) lds_lv[threadIdx.x] = a.f.lv[threadIdx.x];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const TT *tables = reinterpret_cast<const TT *>(a.f.tables);
    const RmCfg c = rm_cfg(a.bound, a.dt_gamma, a.max_steps, a.C, a.H, a.grid);
    // this wave's piece of the work list; neighbouring pieces (neighbouring pixels) go to one XCD's L2
    const uint64_t w_first = ((uint64_t)field_logical_block() * 4 + wave) * a.rays_per_wave;
    const uint32_t w_end = (uint32_t)min(w_first + a.rays_per_wave, (uint64_t)a.N);
    uint32_t cursor = (uint32_t)min(w_first, (uint64_t)a.N);      // wave-uniform

    // ---- slot state (the same in the four g lanes of a slot) ----
    bool active = false, done = false;
    uint32_t n = 0, steps = 0;
    RmRay r = {};
    float t = 0.f, last_t = 0.f, far = 0.f, t_phy = 0.f, ws = 0.f, d = 0.f;
    float T = 1.f;                                                 // TRAIN: the running product
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t n_shaded = 0, n_finished = 0;                         // wave-uniform

    for (;;) {
        // ---- until every slot holds a sample or the list is used up: write finished rays, refill, march ----
        bool got = false;
        float x = 0.f, y = 0.f, z = 0.f, dt = 0.f, tt = 0.f;
        for (;;) {
            n_finished += (uint32_t)__popcll(__ballot(done) & 0xFFFFull);
            if (done) {
                if (g == 0) {
                    a.weights_sum[n] = ws;
                    a.depth[n] = d;
                }
                float *dst = a.image + (size_t)n * a.f.C_ch;
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if ((uint32_t)(4 * g + e) < a.f.C_ch) dst[4 * g + e] = acc[e];
                if (MODE != NSR_STREAM_INFER) {
                    if (g == 0 && a.n_composited != nullptr) a.n_composited[n] = (int32_t)steps;
                    if (a.rgb_map != nullptr) {
                        // k_comp_fwd's epilogue (renderer.py:229-233): white background, depth normalised to [near, far]
#pragma clang fp contract(off)
                        const float bg = 1.0f - ws;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const uint32_t ch = (uint32_t)(4 * g + e);
                            if (ch < 3u) a.rgb_map[(size_t)n * 3 + ch] = acc[e] + bg;
                            else if (ch < a.f.C_ch) a.classes[(size_t)n * (a.f.C_ch - 3u) + (ch - 3u)] = acc[e];
                        }
                        if (g == 0) {
                            const float nr = a.nears[n];
                            a.depth_norm[n] = fmaxf(d - nr, 0.0f) / (far - nr);
                        }
                    }
                }
                active = false;
                done = false;
            }
            const uint32_t need = (uint32_t)(__ballot(!active) & 0xFFFFull);     // slots, from their g == 0 lanes
            if (need != 0u && cursor < w_end) {
                const uint32_t k = cursor + (uint32_t)__popc(need & ((1u << s) - 1u));
                if (!active && k < w_end) {
                    n = min(a.order ? a.order[k] : k, a.N - 1u);
                    r = rm_load_ray(a.rays_o, a.rays_d, n);
                    const float near = a.nears[n];
                    far = a.fars[n];
                    t = rm_start_t(c, near, 0.0f);
                    last_t = t;              // raymarching.cu:530
                    t_phy = TRAIN ? 0.f : near;   // :1163; training: t starts at 0 (:844)
                    T = 1.f;
                    ws = 0.f; d = 0.f; steps = 0;
                    acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
                    active = true;
                }
                cursor = min(cursor + (uint32_t)__popc(need), w_end);
            }
            if (active && !got) {
                // the reference's serial loop (:484-498); a ray that misses the box has near == far == FLT_MAX
                while (t < far && steps < a.max_steps) {
                    if (rm_probe(r, c, t, x, y, z, dt, tt)) { got = true; break; }
                    rm_skip(c, t, tt);
                }
                done = !got;
            }
            if (!(__ballot(done) != 0ull || (__ballot(!active) != 0ull && cursor < w_end))) break;
        }
        if (__ballot(active) == 0ull) break;       // nothing left in any slot (then the list is used up as well)
        n_shaded += (uint32_t)__popcll(__ballot(got) & 0xFFFFull);

        // ---- field of the 16 samples (k_field_fwd's body) ----
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        if (got) {
            u0 = field_unit(x, a.f.bmin[0], a.f.bsize[0]);
            u1 = field_unit(y, a.f.bmin[1], a.f.bsize[1]);
            u2 = field_unit(z, a.f.bmin[2], a.f.bsize[2]);
        }
        const bool live = got && field_in_unit_cube(u0, u1, u2);
        s8v xd, xc;
        field_encode<TT, CD, false, true>(lds_lv, tables, u0, u1, u2, live, g, xd, xc, a.f.fast_levels);
        const f4v o = field_density_net<CD>(wl, lane, xd);
        f4v rgb, cls;
        field_colour_nets<CD>(wl, lane, xc, rgb, cls);
        float v[4];
        field_cat(g, rgb, cls, v);
        // sigma sits on the g == 0 lane of the slot
        const float sigma = __shfl(expf(o[0]) * a.f.density_scale, s, 64);

        // ---- composite this sample ----
        if (TRAIN) {
            // k_comp_fwd's arithmetic (raymarching.cu:846-862), serial where that kernel scans; no contraction, as there
#pragma clang fp contract(off)
            if (got) {
                const float alpha = 1.0f - __expf(-sigma * dt);
                const float weight = alpha * T;
                ws += weight;
                t += dt;
                t_phy += t - last_t;        // t += deltas[1] (:854)
                last_t = t;
                steps++;
                d += weight * t_phy;
#pragma unroll
                for (int e = 0; e < 4; e++) acc[e] += weight * v[e];
                T *= 1.0f - alpha;
                if (T < a.T_thresh) done = true;   // :862: T after this sample
            }
        } else if (got) {
            // k_composite_infer's arithmetic and order
            const float alpha = 1.0f - __expf(-sigma * dt);
            const float T = 1 - ws;
            const float weight = alpha * T;
            ws += weight;
            t += dt;                    // :551
            t_phy += t - last_t;        // deltas[1] of the march
            last_t = t;
            steps++;
            d += weight * t_phy;
#pragma unroll
            for (int e = 0; e < 4; e++) acc[e] += weight * v[e];
            if (T < a.T_thresh) done = true;   // :1206: T before this sample, tested after accumulating it
        }
    }
    if (a.stats != nullptr) {
        if (lane == 0) atomicAdd(a.stats + 0, n_shaded);
        if (lane == 1) atomicAdd(a.stats + 1, n_finished);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <typename TT, int CD>
static int render_infer_launch(const RenderInferArgs &a, int mode, uint32_t nblocks, hipStream_t s) {
    const size_t lds = FW_TOTAL * 2 + 16 * sizeof(NsrLevel);
    if (mode == NSR_STREAM_TRAIN) hipLaunchKernelGGL((k_render_infer<TT, CD, NSR_STREAM_TRAIN>), dim3(nblocks), dim3(256), lds, s, a);
    else if (mode == RI_STREAM_INFER_EXTRAS) hipLaunchKernelGGL((k_render_infer<TT, CD, RI_STREAM_INFER_EXTRAS>), dim3(nblocks), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((k_render_infer<TT, CD, NSR_STREAM_INFER>), dim3(nblocks), dim3(256), lds, s, a);
    return nsr_launch_status();
}

// the one launcher behind both entry points (N != 0, composite checked)
static int render_stream(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *rays_o,
                         const float *rays_d, const uint32_t *order, uint32_t N, const float *nears, const float *fars,
                         const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, float T_thresh,
                         int composite, float *weights_sum, float *depth, float *image, float *rgb_map, float *depth_norm,
                         float *classes, int32_t *n_composited, uint32_t *stats, nsr_stream_t stream) {
    if (C > 16) return NSR_ERR_UNSUPPORTED;
    NSR_CHECK_PTR(desc); NSR_CHECK_PTR(tables); NSR_CHECK_PTR(mlp_params); NSR_CHECK_PTR(rays_o); NSR_CHECK_PTR(rays_d);
    NSR_CHECK_PTR(nears); NSR_CHECK_PTR(fars); NSR_CHECK_PTR(grid); NSR_CHECK_PTR(weights_sum); NSR_CHECK_PTR(depth);
    NSR_CHECK_PTR(image);
    if (max_steps == 0 || C == 0 || !rm_grid_size_ok(H) || !(bound > 0.0f)) return NSR_ERR_INVALID_ARG;
    RenderInferArgs a;
    uint32_t field_blocks;
    const int st = field_fill_args(desc, tables, mlp_params, a.f, N, field_blocks);      // num_classes > 13 -> NSR_ERR_UNSUPPORTED
    if (st != NSR_OK) return st;
    // the epilogue outputs come together: rgb_map and depth_norm, and classes exactly when there are class channels
    if ((rgb_map != nullptr) != (depth_norm != nullptr)) return NSR_ERR_INVALID_ARG;
    if ((classes != nullptr) != (rgb_map != nullptr && desc->num_classes != 0)) return NSR_ERR_INVALID_ARG;
    a.f.xyzs = nullptr; a.f.m_dev = nullptr; a.f.sigmas = nullptr;
    a.f.rgbs = nullptr; a.f.feats = nullptr; a.f.perm = nullptr;
    a.rays_o = rays_o; a.rays_d = rays_d; a.order = order; a.nears = nears; a.fars = fars; a.grid = grid;
    a.N = N; a.bound = bound; a.dt_gamma = dt_gamma; a.max_steps = max_steps; a.C = C; a.H = H; a.T_thresh = T_thresh;
    a.weights_sum = weights_sum; a.depth = depth; a.image = image; a.stats = stats;
    a.n_composited = n_composited; a.rgb_map = rgb_map; a.depth_norm = depth_norm; a.classes = classes;
    int mode = composite;
    if (composite == NSR_STREAM_INFER && (n_composited != nullptr || rgb_map != nullptr)) mode = RI_STREAM_INFER_EXTRAS;
    // A wave's piece of the list: at least 64 rays (four turns of its 16 slots, so that the tail where slots run empty stays
    // short against the piece), more when the frame has more than 2 048 workgroups' worth
    constexpr uint32_t max_blocks = 2048;
    uint32_t rpw = nsr_div_up(N, max_blocks * 4u);
    if (rpw < 64u) rpw = 64u;
    rpw = (rpw + 15u) & ~15u;
    a.rays_per_wave = rpw;
    const uint32_t nblocks = nsr_div_up(N, (uint64_t)rpw * 4u);
    hipStream_t s = (hipStream_t)stream;
    return field_dispatch(desc->table_dtype, desc->compute_dtype,
                          [&](auto tt, auto cd) { return render_infer_launch<decltype(tt), cd()>(a, mode, nblocks, s); });
}

extern "C" {

int nsr_render_rays_infer(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *rays_o,
                          const float *rays_d, const uint32_t *order, uint32_t N, const float *nears, const float *fars,
                          const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps, int is_ndc, uint32_t C, uint32_t H,
                          float T_thresh, float *weights_sum, float *depth, float *image, uint32_t *stats, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    if (is_ndc) return NSR_ERR_UNSUPPORTED;
    return render_stream(desc, tables, mlp_params, rays_o, rays_d, order, N, nears, fars, grid, bound, dt_gamma, max_steps, C, H,
                         T_thresh, NSR_STREAM_INFER, weights_sum, depth, image, nullptr, nullptr, nullptr, nullptr, stats, stream);
}

int nsr_render_rays_stream(const nsr_field_desc *desc, const void *tables, const float *mlp_params, const float *rays_o,
                           const float *rays_d, const uint32_t *order, uint32_t N, const float *nears, const float *fars,
                           const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                           float T_thresh, int composite, float *weights_sum, float *depth, float *image, float *rgb_map,
                           float *depth_norm, float *classes, int32_t *n_composited, uint32_t *stats, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    if (composite != NSR_STREAM_INFER && composite != NSR_STREAM_TRAIN) return NSR_ERR_INVALID_ARG;
    return render_stream(desc, tables, mlp_params, rays_o, rays_d, order, N, nears, fars, grid, bound, dt_gamma, max_steps, C, H,
                         T_thresh, composite, weights_sum, depth, image, rgb_map, depth_norm, classes, n_composited, stats, stream);
}

}   // extern "C"
