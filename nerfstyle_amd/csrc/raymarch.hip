// Occupancy-grid training march and sample compaction for gfx950.  The probe core is rm_probe.h, the inference march and
// composites are raymarch_infer.hip, the training composite is composite.hip.
// Behaviour follows hkust-vgd/nerfstyle raymarching/src/raymarching.cu (cited per function);
// the structure does not: offsets come from a wave64 shuffle scan + one look-up of per-block
// totals (deterministic, no atomics), the composite backward keeps its running sums in
// registers (no rgbs_buf round trip), and every entry point takes an explicit stream.
#include "rm_probe.h"

#define NSR_MARCH_WPR_MAX_RAYS 20480u   // batches up to this size march one wave per ray (k_march_wpr)

// ---------------------------------------------------------------------------------------------
// pieces the emitting kernels share
// ---------------------------------------------------------------------------------------------
// A dropped ray (point_index + num_steps >= M, :517): the reference's buffers are zero-filled before the launch
// (raymarching.py:238-240), here they are torch.empty -- write the in-buffer part, so that no consumer bounded by
// min(counter[0], M) ever reads uninitialised positions (a NaN bit pattern would poison the weight gradients as 0 * NaN).
// One thread calls it with (first, stride) = (0, 1), a wave with (lane, 64).
__device__ __forceinline__ void rm_zero_dropped(uint32_t point_index, uint32_t num_steps, uint32_t M, uint32_t first, uint32_t stride,
                                                float *xyzs, float *dirs, float *deltas) {
    for (uint32_t i = point_index + first; i < min(point_index + num_steps, M); i += stride) {
        xyzs[(size_t)i * 3 + 0] = 0.f; xyzs[(size_t)i * 3 + 1] = 0.f; xyzs[(size_t)i * 3 + 2] = 0.f;
        if (dirs) { dirs[(size_t)i * 3 + 0] = 0.f; dirs[(size_t)i * 3 + 1] = 0.f; dirs[(size_t)i * 3 + 2] = 0.f; }
        reinterpret_cast<float4 *>(deltas)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Start of a thread-per-ray emit (:505-517): the ray's offset from the block scan of the counts, its `rays` triple, and the
// zero-fill of a dropped ray.  Every thread of the block calls it (the scan synchronises); true = the ray emits samples.
__device__ __forceinline__ bool rm_thread_ray_begin(uint32_t n, uint32_t N, uint32_t M, const uint32_t *counts, const uint32_t *block_bases,
                                                    uint32_t *wave_sums, float *xyzs, float *dirs, float *deltas, int32_t *rays,
                                                    uint32_t &point_index, uint32_t &num_steps) {
    num_steps = n < N ? counts[n] : 0u;
    uint32_t total;
    point_index = block_bases[blockIdx.x] + rm_block_exclusive_scan(num_steps, wave_sums, total);
    if (n >= N) return false;
    rays[n * 3 + 0] = (int32_t)n;
    rays[n * 3 + 1] = (int32_t)point_index;
    rays[n * 3 + 2] = (int32_t)num_steps;
    if (num_steps == 0) return false;
    if (point_index + num_steps >= M) {
        rm_zero_dropped(point_index, num_steps, M, 0u, 1u, xyzs, dirs, deltas);
        return false;
    }
    return true;
}

// The same for a wave per ray: base of the ray's 256-ray block + the counts of the rays before it in the block.
__device__ __forceinline__ bool rm_wave_ray_begin(uint32_t n, uint32_t lane, uint32_t M, const uint32_t *counts, const uint32_t *block_bases,
                                                  float *xyzs, float *dirs, float *deltas, int32_t *rays, uint32_t &point_index,
                                                  uint32_t &num_steps) {
    const uint32_t blk0 = (n / RM_BLOCK) * RM_BLOCK;
    uint32_t part = 0;
    for (uint32_t i = blk0 + lane; i < n; i += 64) part += counts[i];
    point_index = block_bases[n / RM_BLOCK] + nsr_wave_sum(part);
    num_steps = counts[n];
    if (lane == 0) {
        rays[n * 3 + 0] = (int32_t)n;
        rays[n * 3 + 1] = (int32_t)point_index;
        rays[n * 3 + 2] = (int32_t)num_steps;
    }
    if (num_steps == 0) return false;
    if (point_index + num_steps >= M) {
        rm_zero_dropped(point_index, num_steps, M, lane, 64u, xyzs, dirs, deltas);
        return false;
    }
    return true;
}

// Constant step (LLFF: dt_gamma = 0): t_{j+1} = fl(t_j + dt).  Inside one binade every t_j is an integer multiple m_j of the
// binade's ulp u, and with f = dt / u the rounded sum is m_{j+1} = rne(m_j + f).  When the fractional part of f is not 1/2
// that is m_j + rne(f) for every integer m_j: a constant advance of the BIT PATTERN.  When it is exactly 1/2, every sum is a
// tie and goes to the EVEN neighbour: m_{j+1} is even whatever m_j was, and from an even m_j the advance is the even one of
// floor(f), floor(f) + 1 -- constant again, but only from the first even m_j on.  So the advance t_1 -> t_2 is the advance of
// every later step PROVIDED t_1 is itself the rounded result of an addition in this binade, i.e. t_0 is a multiple of u too:
// t_0 .. t_span must share an exponent, t_0 included.  (A t_0 in the binade below is a multiple of u / 2 only; t_0 + dt can
// then be an ODD multiple of u with no rounding at all, and t_1 -> t_2 rounds the other way from t_2 -> t_3: at max_steps =
// 257, t_0 = 0x407ff003 the sums go +0x6e6b, +0x6e6c, +0x6e6c, ...)  Two real additions give t_1 and t_2, c = bits(t_2) -
// bits(t_1), and t_j = bits(t_1) + (j - 1) c for j = 1..span -- the same floats as `span` serial additions.  Returns whether
// that holds for the sequence that starts at t, with b1 = bits(t_1) and cc = c; otherwise the caller adds serially.
__device__ __forceinline__ bool rm_const_step(const RmCfg &c, float t, uint32_t span, uint32_t &b1, uint32_t &cc) {
    bool closed = false;
    b1 = 0; cc = 0;
    if (c.dt_gamma == 0.0f && t > 0.0f) {
#pragma clang fp contract(off)
        const float dt0 = rm_clamp(t * c.dt_gamma, c.dt_min, c.dt_max);
        const float t1 = t + dt0, t2 = t1 + dt0;
        b1 = __float_as_uint(t1);
        const uint32_t b2 = __float_as_uint(t2);
        cc = b2 - b1;
        const uint32_t b_last = b1 + (span - 1u) * cc;
        // (bits(t) <= b1 <= b_last: with the ends in one binade, t_1 is in it too)
        closed = b2 > b1 && (__float_as_uint(t) >> 23) == (b_last >> 23) && cc < (1u << 23);
    }
    return closed;
}

// One sample of a thread-per-ray emit at the ray's walking pointers: position, direction (when asked for) and the leading
// deltas columns -- float2 (dt, t_next - last_t), or all four for NDC.
template <typename V>
__device__ __forceinline__ void rm_store_sample(const RmRay &r, float x, float y, float z, V del, float *&pxyz, float *&pdir, float *&pdel) {
    pxyz[0] = x; pxyz[1] = y; pxyz[2] = z;
    if (pdir) { pdir[0] = r.dx; pdir[1] = r.dy; pdir[2] = r.dz; pdir += 3; }
    reinterpret_cast<V *>(pdel)[0] = del;
    pxyz += 3; pdel += 4;
}

// ---------------------------------------------------------------------------------------------
// training march: count -> scan -> emit
// ---------------------------------------------------------------------------------------------
// pass 1 (raymarching.cu:455-501): per-ray sample count, per-block total.
__global__ void __launch_bounds__(RM_BLOCK)
k_march_count(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const uint8_t *__restrict__ grid,
              float bound, float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
              const float *__restrict__ nears, const float *__restrict__ fars, const float *__restrict__ noises,
              uint32_t *__restrict__ counts, uint32_t *__restrict__ block_sums, uint32_t *__restrict__ mask, uint32_t kcap) {
    __shared__ uint32_t wave_sums[RM_BLOCK / 64];
    const uint32_t n = blockIdx.x * RM_BLOCK + threadIdx.x;
    uint32_t num_steps = 0;
    if (n < N) {
        const RmCfg c = rm_cfg(bound, dt_gamma, max_steps, C, H, grid);
        const RmRay r = rm_load_ray(rays_o, rays_d, n);
        const float far = fars[n];
        float t = rm_start_t(c, nears[n], noises ? noises[n] : 0.0f);
        float x, y, z, dt, tt;
        if (mask == nullptr) {
            // NDC only: every other batch marches a wave per ray or records the mask (see nsr_march_rays_train)
            while (t < far && num_steps < max_steps) {
                if (rm_probe(r, c, t, x, y, z, dt, tt)) {
                    num_steps++;
                    t += dt;
                } else {
                    rm_skip(c, t, tt);
                }
            }
        } else {
            // Round 3: the probes are made ONCE.  Every parameter the loop visits is an element of the occupancy-independent
            // sequence t_0, t_{k+1} = t_k + clamp(t_k * dt_gamma, dt_min, dt_max) (both branches advance t by exactly that
            // expression), so the samples are fully described by WHICH k they sit at: a bit mask per ray, word w of ray n at
            // mask[w * N + n].  k_march_emit_mask replays the sequence (one addition per k, no probe) and emits the marked
            // elements -- bit-identical to re-marching, at a twentieth of the instructions.
            uint32_t k = 0, word = 0, wi = 0;
            const uint32_t wmax = (kcap + 31u) / 32u;
            while (t < far && num_steps < max_steps && k < kcap) {
                if (rm_probe(r, c, t, x, y, z, dt, tt)) {
                    word |= 1u << (k & 31u);
                    num_steps++;
                    t += dt;
                    k++;
                } else {
                    k += rm_skip(c, t, tt);
                }
                while (wi < (k >> 5) && wi < wmax) {     // completed words (a skip may pass several: zeros)
                    mask[(size_t)wi * N + n] = word;
                    word = 0;
                    wi++;
                }
            }
            if (wi <= wmax) mask[(size_t)wi * N + n] = word;      // (the mask holds wmax + 1 words per ray)
        }
        counts[n] = num_steps;
    }
    uint32_t total;
    rm_block_exclusive_scan(num_steps, wave_sums, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// Exclusive scan of the per-block totals by ONE block; also applies the reference's counter
// semantics (atomicAdd(counter, num_steps) / atomicAdd(counter+1, 1), :506-507): block bases
// start at the incoming counter[0]; counter[0] += total, counter[1] += N.
__global__ void __launch_bounds__(1024)
k_scan_block_sums(uint32_t *__restrict__ block_sums, uint32_t nblocks, int32_t *__restrict__ counter, uint32_t N) {
    __shared__ uint32_t wave_sums[1024 / 64];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = counter ? (uint32_t)counter[0] : 0u;
    __syncthreads();
    const uint32_t base0 = carry_s;
    uint32_t carry = base0;
    for (uint32_t start = 0; start < nblocks; start += 1024) {
        const uint32_t i = start + threadIdx.x;
        const uint32_t v = i < nblocks ? block_sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = rm_block_exclusive_scan(v, wave_sums, total);
        if (i < nblocks) block_sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0 && counter) {
        counter[0] = (int32_t)carry;
        counter[1] += (int32_t)N;
    }
}
// (host launcher, declared in rm_util.h: the alive-ray compaction of raymarch_infer.hip scans with the same kernel)
void rm_scan_block_sums(uint32_t *block_sums, uint32_t nblocks, int32_t *counter, uint32_t N, hipStream_t stream) {
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, stream, block_sums, nblocks, counter, N);
}

// pass 2 for NDC (raymarching.cu:505-588): offsets from the scan, then re-march and emit.  The NDC deltas need the
// previous sample's z, so this form probes the grid again where k_march_emit_mask only replays.
__global__ void __launch_bounds__(RM_BLOCK)
k_march_emit_ndc(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ z_hats,
                 const uint8_t *__restrict__ grid, float bound, float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C,
                 uint32_t H, uint32_t M, const float *__restrict__ nears, const float *__restrict__ fars,
                 const float *__restrict__ noises, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ block_bases,
                 float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas, int32_t *__restrict__ rays) {
    __shared__ uint32_t wave_sums[RM_BLOCK / 64];
    const uint32_t n = blockIdx.x * RM_BLOCK + threadIdx.x;
    uint32_t point_index, num_steps;
    if (!rm_thread_ray_begin(n, N, M, counts, block_bases, wave_sums, xyzs, dirs, deltas, rays, point_index, num_steps)) return;

    const RmCfg c = rm_cfg(bound, dt_gamma, max_steps, C, H, grid);
    const RmRay r = rm_load_ray(rays_o, rays_d, n);
    const float far = fars[n];
    float t = rm_start_t(c, nears[n], noises ? noises[n] : 0.0f);
    float *pxyz = xyzs + (size_t)point_index * 3;
    float *pdir = dirs ? dirs + (size_t)point_index * 3 : nullptr;
    float *pdel = deltas + (size_t)point_index * 4;
    uint32_t step = 0;
    float last_t = t;
    float last_z;
    {
#pragma clang fp contract(off)
        last_z = rm_clamp(r.oz + t * r.dz, -bound, bound);     // (contracted to an fma it is not the oracle's float)
    }
    float x, y, z, dt, tt;
    while (t < far && step < num_steps) {
        if (rm_probe(r, c, t, x, y, z, dt, tt)) {
#pragma clang fp contract(off)
            t += dt;
            const float new_z = rm_clamp(r.oz + t * r.dz, -bound, bound);
            const float zh = z_hats[n];
            rm_store_sample(r, x, y, z, make_float4(dt, t - last_t, (2 / (new_z - 1) - 2 / (z - 1)) / zh,
                                                    (2 / (new_z - 1) - 2 / (last_z - 1)) / zh), pxyz, pdir, pdel);
            last_z = z;   // :570
            last_t = t;
            step++;
        } else {
            rm_skip(c, t, tt);
        }
    }
}

// pass 2 without probes: replays the t sequence and emits the elements k_march_count marked (see there).  Not for NDC
// (its deltas need the previous sample's z, k_march_emit_ndc keeps that form).
__global__ void __launch_bounds__(RM_BLOCK)
k_march_emit_mask(const float *__restrict__ rays_o, const float *__restrict__ rays_d, float bound, float dt_gamma,
                  uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float *__restrict__ nears,
                  const float *__restrict__ noises, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ block_bases,
                  const uint32_t *__restrict__ mask, float *__restrict__ xyzs, float *__restrict__ dirs,
                  float *__restrict__ deltas, int32_t *__restrict__ rays) {
    __shared__ uint32_t wave_sums[RM_BLOCK / 64];
    const uint32_t n = blockIdx.x * RM_BLOCK + threadIdx.x;
    uint32_t point_index, num_steps;
    if (!rm_thread_ray_begin(n, N, M, counts, block_bases, wave_sums, xyzs, dirs, deltas, rays, point_index, num_steps)) return;
    const RmCfg c = rm_cfg(bound, dt_gamma, max_steps, C, H, nullptr);
    const RmRay r = rm_load_ray(rays_o, rays_d, n);
    float t = rm_start_t(c, nears[n], noises ? noises[n] : 0.0f);
    float *pxyz = xyzs + (size_t)point_index * 3;
    float *pdir = dirs ? dirs + (size_t)point_index * 3 : nullptr;
    float *pdel = deltas + (size_t)point_index * 4;
    uint32_t step = 0;
    float last_t = t;
    for (uint32_t w = 0; step < num_steps; w++) {
        uint32_t word = mask[(size_t)w * N + n];
        // Constant step (dt_gamma = 0) inside one binade: the word's 32 parameters are t, t_1 = t + dt and t_j = bits(t_1) +
        // (j - 1) (bits(t_2) - bits(t_1)) -- the floats the 32 serial additions give (rm_const_step has the argument) -- so only the
        // MARKED steps cost instructions.  Words that cross a binade keep the serial form.
        uint32_t b1, cc;
        if (rm_const_step(c, t, 32u, b1, cc)) {
            while (word != 0u && step < num_steps) {
#pragma clang fp contract(off)
                const uint32_t k = (uint32_t)__builtin_ctz(word);
                word &= word - 1u;
                const float tk = k == 0u ? t : __uint_as_float(b1 + (k - 1u) * cc);
                const float dt = rm_clamp(tk * dt_gamma, c.dt_min, c.dt_max);
                const float t_next = tk + dt;
                rm_store_sample(r, rm_clamp(r.ox + tk * r.dx, -bound, bound), rm_clamp(r.oy + tk * r.dy, -bound, bound),
                                rm_clamp(r.oz + tk * r.dz, -bound, bound), make_float2(dt, t_next - last_t), pxyz, pdir, pdel);
                last_t = t_next;
                step++;
            }
            t = __uint_as_float(b1 + 31u * cc);                  // t_32: the next word's first parameter
            continue;
        }
        for (uint32_t b = 0; b < 32u && step < num_steps; b++, word >>= 1) {
#pragma clang fp contract(off)
            const float dt = rm_clamp(t * dt_gamma, c.dt_min, c.dt_max);
            const float t_next = t + dt;
            if (word & 1u) {
                rm_store_sample(r, rm_clamp(r.ox + t * r.dx, -bound, bound), rm_clamp(r.oy + t * r.dy, -bound, bound),
                                rm_clamp(r.oz + t * r.dz, -bound, bound), make_float2(dt, t_next - last_t), pxyz, pdir, pdel);
                last_t = t_next;
                step++;
            }
            t = t_next;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// training march, one WAVE per ray (small batches)
// ---------------------------------------------------------------------------------------------
// The thread-per-ray march above is a serial chain of ~200-instruction probes per ray: 0.85 ms for a
// 4096-ray batch however idle the chip is.  The parameters the reference visits are the ray-independent
// sequence t_0 = near (+ noise), t_{k+1} = t_k + clamp(t_k * dt_gamma, dt_min, dt_max) -- both branches of
// the loop (:484-498) advance t by exactly that expression -- and the loop only decides WHICH t_k it
// probes: after an occupied probe the next one, after an empty probe the first t_j >= tt.  So a wave
// takes 64 consecutive t_k, all lanes probe speculatively (same rm_probe, same rounding), every empty
// lane finds its successor j by binary search over the wave's t values, and a scalar walk follows the
// successor links from the entry point: exactly the probes, in exactly the order, of the serial loop.
// Lanes the walk visits and finds occupied are the samples.

// per-block totals of counts[] (the tail of k_march_count)
__global__ void __launch_bounds__(RM_BLOCK)
k_march_block_sums(const uint32_t *__restrict__ counts, uint32_t N, uint32_t *__restrict__ block_sums) {
    __shared__ uint32_t wave_sums[RM_BLOCK / 64];
    const uint32_t n = blockIdx.x * RM_BLOCK + threadIdx.x;
    uint32_t total;
    rm_block_exclusive_scan(n < N ? counts[n] : 0u, wave_sums, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// The 64 consecutive march parameters that start at t_block -- lane j gets t_j of t_0 = t_block, t_{j+1} = t_j + clamp(t_j *
// dt_gamma, dt_min, dt_max) -- and t_64 (the next block's start).  Shared by the counting / re-marching kernel and the replaying
// emit, so that both see the same floats.
__device__ __forceinline__ void wpr_block_t(const RmCfg &c, float dt_gamma, float t_block, uint32_t lane, float &my_t, float &t_next) {
    float tc = t_block;
    my_t = t_block;
    uint32_t b1, cc;
    bool closed = false;        // (a flag and two ifs, not if / else: the shape whose instructions the timings here were taken with)
    if (rm_const_step(c, t_block, 64u, b1, cc)) {
        closed = true;
        my_t = lane == 0 ? t_block : __uint_as_float(b1 + (lane - 1u) * cc);
        tc = __uint_as_float(b1 + 63u * cc);
    }
    if (!closed) {
#pragma clang fp contract(off)
        for (uint32_t j = 0; j < 64; j++) {
            if (lane == j) my_t = tc;
            tc += rm_clamp(tc * dt_gamma, c.dt_min, c.dt_max);
        }
    }
    t_next = tc;
}

// Emits one block's samples: lane j holds parameter t_j with its position, step dt and t_after = t_j + dt (t += dt, :551);
// sample_mask marks the sample lanes, `steps` counts the ray's samples up to and including this block's, last_t is t after
// the previous sample's step (:530) and is carried on.  tl is the wave's 64 floats of LDS.
__device__ __forceinline__ void wpr_emit_block(const RmRay &r, unsigned long long sample_mask, uint32_t lane, uint32_t steps,
                                               uint32_t point_index, float x, float y, float z, float dt, float t_after, float *tl,
                                               float &last_t, float *xyzs, float *dirs, float *deltas) {
#pragma clang fp contract(off)
    const bool mine = (sample_mask >> lane) & 1ull;
    const uint32_t first_idx = steps - (uint32_t)__popcll(sample_mask);       // samples emitted before this block
    const uint32_t before = (uint32_t)__popcll(sample_mask & ((1ull << lane) - 1ull));
    __builtin_amdgcn_wave_barrier();
    tl[lane] = t_after;
    __builtin_amdgcn_wave_barrier();
    // t after the previous sample's step: previous sample lane of this block, or the carried one
    const unsigned long long below = sample_mask & ((1ull << lane) - 1ull);
    const float prev_t = below ? tl[63 - __builtin_clzll(below)] : last_t;
    if (mine) {
        const size_t o = (size_t)point_index + first_idx + before;
        xyzs[o * 3 + 0] = x; xyzs[o * 3 + 1] = y; xyzs[o * 3 + 2] = z;
        if (dirs) { dirs[o * 3 + 0] = r.dx; dirs[o * 3 + 1] = r.dy; dirs[o * 3 + 2] = r.dz; }
        reinterpret_cast<float2 *>(deltas + o * 4)[0] = make_float2(dt, t_after - prev_t);
    }
    last_t = tl[63 - __builtin_clzll(sample_mask)];
}

template <bool EMIT>
__global__ void __launch_bounds__(256)
k_march_wpr(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const uint8_t *__restrict__ grid, float bound,
            float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float *__restrict__ nears,
            const float *__restrict__ fars, const float *__restrict__ noises, uint32_t *__restrict__ counts,
            const uint32_t *__restrict__ block_bases, float *__restrict__ xyzs, float *__restrict__ dirs,
            float *__restrict__ deltas, int32_t *__restrict__ rays, uint32_t *__restrict__ slots, uint32_t slot_cap) {
    __shared__ float t_lds[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n = blockIdx.x * 4 + wave;
    if (n >= N) return;                                     // wave-uniform
    float *tl = t_lds[wave];
    const RmCfg c = rm_cfg(bound, dt_gamma, max_steps, C, H, grid);
    const RmRay r = rm_load_ray(rays_o, rays_d, n);
    const float far = fars[n];
    float t_block = rm_start_t(c, nears[n], noises ? noises[n] : 0.0f);
    uint32_t limit = max_steps, point_index = 0;
    if (EMIT && !rm_wave_ray_begin(n, lane, M, counts, block_bases, xyzs, dirs, deltas, rays, point_index, limit)) return;
    uint32_t steps = 0;
    float carry_tt = -INFINITY;       // the walk enters a block at its first t >= carry_tt
    float last_t = t_block;           // :530, t after the previous sample's step
    bool done = false;
    // (counting pass with `slots`: every block's start and sample mask are recorded -- [slot_cap][3] words per ray after the N
    // block counts -- and k_march_wpr_replay emits from them without probing again; slot_cap * 64 >= march_kcap, the bound the
    // thread-per-ray mask relies on)
    uint32_t nblk = 0;
    while (!done && t_block < far && (EMIT || slots == nullptr || nblk < slot_cap)) {
        // ---- the block's 64 parameters ----
        float my_t, tc;
        wpr_block_t(c, dt_gamma, t_block, lane, my_t, tc);
        const float t_next_block = tc;
        // ---- speculative probe ----
        const bool valid = my_t < far;
        float x = 0, y = 0, z = 0, dt = 0, tt = 0;
        const bool occ = valid && rm_probe(r, c, valid ? my_t : t_block, x, y, z, dt, tt);
        // ---- successor of an empty lane: first j > lane with t_j >= tt (do { t += dt; } while (t < tt), :497) ----
        tl[lane] = my_t;
        __builtin_amdgcn_wave_barrier();
        uint32_t lo = lane + 1, hi = 64;
#pragma unroll
        for (int it = 0; it < 6; it++) {
            const uint32_t mid = (lo + hi) >> 1;
            const float tm = tl[mid < 64 ? mid : 63];
            const bool go = lo < hi && tm < tt;
            const bool stay = lo < hi && !(tm < tt);
            lo = go ? mid + 1 : lo;
            hi = stay ? mid : hi;
        }
        const uint32_t nxt = occ ? lane + 1 : lo;
        // ---- walk the chain ----
        const unsigned long long occ_mask = __ballot(occ), valid_mask = __ballot(valid);
        uint32_t cur = 0;
        if (carry_tt != -INFINITY) {
            const unsigned long long ge = __ballot(my_t >= carry_tt);
            cur = ge ? (uint32_t)__builtin_ctzll(ge) : 64u;
        }
        unsigned long long sample_mask = 0ull;
        uint32_t last = 64;
        while (cur < 64) {
            if (!((valid_mask >> cur) & 1ull)) { done = true; break; }          // t >= far
            if ((occ_mask >> cur) & 1ull) {
                sample_mask |= 1ull << cur;
                steps++;
                if (steps == limit) { done = true; break; }
            }
            last = cur;
            cur = (uint32_t)__builtin_amdgcn_readlane((int)nxt, (int)cur);
        }
        if (!done && last < 64)
            carry_tt = ((occ_mask >> last) & 1ull) ? -INFINITY : __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tt), (int)last));
        // ---- emit this block's samples ----
        if (EMIT && sample_mask)
            wpr_emit_block(r, sample_mask, lane, steps, point_index, x, y, z, dt, my_t + dt, tl, last_t, xyzs, dirs, deltas);
        __builtin_amdgcn_wave_barrier();
        if (!EMIT && slots != nullptr) {
            if (lane < 3) {
                const uint32_t wv = lane == 0 ? __float_as_uint(t_block) : (lane == 1 ? (uint32_t)sample_mask : (uint32_t)(sample_mask >> 32));
                slots[(size_t)N + ((size_t)n * slot_cap + nblk) * 3 + lane] = wv;
            }
            nblk++;
        }
        t_block = t_next_block;
    }
    if (!EMIT && lane == 0) {
        counts[n] = steps;
        if (slots != nullptr) slots[n] = nblk;
    }
}

// Emitting pass of the wave-per-ray march from the counting pass's records: no occupancy probe, no successor search, no chain
// walk -- per recorded block with samples: the 64 parameters again (wpr_block_t), positions and step sizes of the marked lanes,
// the stores of wpr_emit_block.  Bit-identical output; 4 096-ray bf16 + graph step 1.09 -> 0.96 ms.
__global__ void __launch_bounds__(256)
k_march_wpr_replay(const float *__restrict__ rays_o, const float *__restrict__ rays_d, float bound, float dt_gamma, uint32_t max_steps,
                   uint32_t N, uint32_t C, uint32_t H, uint32_t M, const uint32_t *__restrict__ counts,
                   const uint32_t *__restrict__ block_bases, const uint32_t *__restrict__ slots, uint32_t slot_cap,
                   float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas, int32_t *__restrict__ rays) {
    __shared__ float t_lds[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n = blockIdx.x * 4 + wave;
    if (n >= N) return;                                     // wave-uniform
    float *tl = t_lds[wave];
    const RmCfg c = rm_cfg(bound, dt_gamma, max_steps, C, H, nullptr);
    const RmRay r = rm_load_ray(rays_o, rays_d, n);
    uint32_t point_index, limit;
    if (!rm_wave_ray_begin(n, lane, M, counts, block_bases, xyzs, dirs, deltas, rays, point_index, limit)) return;
    const uint32_t nblk = min(slots[n], min(slot_cap, 64u));
    // lane b holds block b's record
    const uint32_t *rec = slots + (size_t)N + (size_t)n * slot_cap * 3;
    uint32_t s_t = 0, s_lo = 0, s_hi = 0;
    if (lane < nblk) { s_t = rec[lane * 3]; s_lo = rec[lane * 3 + 1]; s_hi = rec[lane * 3 + 2]; }
    uint32_t steps = 0;
    float last_t = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)s_t));      // block 0 starts at the ray's first parameter
    for (uint32_t b = 0; b < nblk; b++) {
        const unsigned long long sample_mask = (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)s_lo, (int)b) |
                                               ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)s_hi, (int)b) << 32);
        if (sample_mask == 0ull) continue;
        const float t_block = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)s_t, (int)b));
        float my_t, t_next;
        wpr_block_t(c, dt_gamma, t_block, lane, my_t, t_next);
        steps += (uint32_t)__popcll(sample_mask);
        float x, y, z, dt, t_after;
        {
#pragma clang fp contract(off)
            x = rm_clamp(r.ox + my_t * r.dx, -c.bound, c.bound);         // rm_probe's expressions
            y = rm_clamp(r.oy + my_t * r.dy, -c.bound, c.bound);
            z = rm_clamp(r.oz + my_t * r.dz, -c.bound, c.bound);
            dt = rm_clamp(my_t * c.dt_gamma, c.dt_min, c.dt_max);
            t_after = my_t + dt;                                            // t += dt, :551
        }
        wpr_emit_block(r, sample_mask, lane, steps, point_index, x, y, z, dt, t_after, tl, last_t, xyzs, dirs, deltas);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

// step-index capacity of the sample mask: t runs from near to far (<= the AABB diagonal 2 sqrt(3) bound) in steps of at
// least dt_min = 2 sqrt(3) / max_steps, i.e. at most bound * max_steps additions; + slack for the rounding of the sums
static uint32_t march_kcap(float bound, uint32_t max_steps) { return (uint32_t)ceilf(fmaxf(bound, 1.0f) * (float)max_steps) + 96u; }
static bool march_uses_mask(uint32_t N, int is_ndc) { return !is_ndc && N > NSR_MARCH_WPR_MAX_RAYS; }
// wave-per-ray path: records per ray (block start + 64-bit sample mask), 0 = too many for a wave's lanes (re-marching emit)
static uint32_t march_wpr_slot_cap(float bound, uint32_t max_steps) {
    const uint32_t cap = (march_kcap(bound, max_steps) + 63u) / 64u + 1u;
    return cap <= 64u ? cap : 0u;
}

uint64_t nsr_march_rays_train_workspace_bytes(uint32_t N, float bound, uint32_t max_steps) {
    const uint64_t nblocks = (N + RM_BLOCK - 1) / RM_BLOCK;
    uint64_t words = (uint64_t)N + nblocks + 64;
    if (march_uses_mask(N, 0)) words += (uint64_t)N * ((march_kcap(bound, max_steps) + 31u) / 32u + 1u);
    else words += (uint64_t)N * (1u + 3u * march_wpr_slot_cap(bound, max_steps));
    return words * sizeof(uint32_t);
}

int nsr_march_rays_train(const float *rays_o, const float *rays_d, const float *z_hats, const uint8_t *grid, float bound,
                         float dt_gamma, uint32_t max_steps, int is_ndc, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                         const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas, int32_t *rays,
                         int32_t *counter, const float *noises, void *workspace, nsr_stream_t stream) {
    if (N == 0) return NSR_OK;
    NSR_CHECK_PTR(rays_o); NSR_CHECK_PTR(rays_d); NSR_CHECK_PTR(grid); NSR_CHECK_PTR(nears); NSR_CHECK_PTR(fars);
    NSR_CHECK_PTR(xyzs); NSR_CHECK_PTR(deltas); NSR_CHECK_PTR(rays); NSR_CHECK_PTR(counter); NSR_CHECK_PTR(workspace);
    if (is_ndc && z_hats == nullptr) return NSR_ERR_INVALID_ARG;
    if (max_steps == 0 || C == 0 || C > 8 || !rm_grid_size_ok(H)) return NSR_ERR_INVALID_ARG;
    if (((uintptr_t)deltas & 15u) != 0) return NSR_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nblocks = (N + RM_BLOCK - 1) / RM_BLOCK;
    uint32_t *counts = (uint32_t *)workspace;
    uint32_t *block_sums = counts + N;
    // Which input reaches which kernels (all bit-identical to the sequential reference):
    //   not NDC, N <= 20 480: k_march_wpr<false> counts and records, k_march_wpr_replay emits (k_march_wpr<true> when a ray can
    //                         need more records than a wave has lanes)
    //   not NDC, N >  20 480: k_march_count marks the samples in the mask, k_march_emit_mask replays it
    //   NDC, every N:         k_march_count without the mask, k_march_emit_ndc marches again
    // small batches: one wave per ray (k_march_wpr), bit-identical results
    if (!is_ndc && N <= NSR_MARCH_WPR_MAX_RAYS) {
        const uint32_t wblocks = (N + 3) / 4;
        // the counting pass records every block's start and sample mask; the emit replays them (no second probe).  When a
        // ray can need more records than a wave has lanes (slot_cap = 0), the emit marches again instead.
        const uint32_t slot_cap = march_wpr_slot_cap(bound, max_steps);
        uint32_t *slots = slot_cap ? block_sums + nblocks + 64 : nullptr;
        hipLaunchKernelGGL((k_march_wpr<false>), dim3(wblocks), dim3(256), 0, s, rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C,
                           H, M, nears, fars, noises, counts, (const uint32_t *)nullptr, (float *)nullptr, (float *)nullptr,
                           (float *)nullptr, (int32_t *)nullptr, slots, slot_cap);
        hipLaunchKernelGGL(k_march_block_sums, dim3(nblocks), dim3(RM_BLOCK), 0, s, counts, N, block_sums);
        rm_scan_block_sums(block_sums, nblocks, counter, N, s);
        if (slots)
            hipLaunchKernelGGL(k_march_wpr_replay, dim3(wblocks), dim3(256), 0, s, rays_o, rays_d, bound, dt_gamma, max_steps, N, C, H, M,
                               counts, block_sums, slots, slot_cap, xyzs, dirs, deltas, rays);
        else
            hipLaunchKernelGGL((k_march_wpr<true>), dim3(wblocks), dim3(256), 0, s, rays_o, rays_d, grid, bound, dt_gamma, max_steps, N,
                               C, H, M, nears, fars, noises, counts, block_sums, xyzs, dirs, deltas, rays, (uint32_t *)nullptr, 0u);
        return nsr_launch_status();
    }
    // large batches, thread per ray: the counting pass marks the samples in a per-ray bit mask, the emitting pass replays the
    // t sequence without probing the grid again (NDC keeps the re-marching emit)
    const bool use_mask = march_uses_mask(N, is_ndc);
    uint32_t *mask = use_mask ? block_sums + nblocks + 64 : nullptr;
    const uint32_t kcap = march_kcap(bound, max_steps);
    hipLaunchKernelGGL(k_march_count, dim3(nblocks), dim3(RM_BLOCK), 0, s, rays_o, rays_d, grid, bound, dt_gamma, max_steps, N,
                       C, H, nears, fars, noises, counts, block_sums, mask, kcap);
    // the reference's ray slots start at the incoming counter[1]; only 0 is supported without a
    // host read (renderer.py:213-214 zeroes the counter before every call)
    rm_scan_block_sums(block_sums, nblocks, counter, N, s);
    // The replaying emit is bound by its stores: every lane appends 12 + 8 bytes at a time to its own ray's two runs, and with
    // the ~30 waves per CU its 41 registers allow, more partially written lines are open than the L2 holds.  60 KB of (unused)
    // dynamic LDS per workgroup keeps two workgroups per CU: 1.12-1.20 -> 0.87-1.09 ms on the bench frame (box to box); the
    // closed-form step of k_march_emit_mask takes another ~15 us at that occupancy, nothing at full occupancy.
    constexpr size_t emit_lds = 61440;
    if (use_mask)
        hipLaunchKernelGGL(k_march_emit_mask, dim3(nblocks), dim3(RM_BLOCK), emit_lds, s, rays_o, rays_d, bound, dt_gamma, max_steps, N, C,
                           H, M, nears, noises, counts, block_sums, mask, xyzs, dirs, deltas, rays);
    else
        hipLaunchKernelGGL(k_march_emit_ndc, dim3(nblocks), dim3(RM_BLOCK), 0, s, rays_o, rays_d, z_hats, grid, bound, dt_gamma,
                           max_steps, N, C, H, M, nears, fars, noises, counts, block_sums, xyzs, dirs, deltas, rays);
    return nsr_launch_status();
}

}   // extern "C"
