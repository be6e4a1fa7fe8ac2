// The probe core of the occupancy-grid ray march for gfx950: what the training march (raymarch.hip) and the
// inference march (raymarch_infer.hip) both run per ray parameter.  Behaviour follows hkust-vgd/nerfstyle
// raymarching/src/raymarching.cu (cited per function).
#pragma once
#include "nsr_common.h"
#include "rm_util.h"

#define RM_BLOCK 256
#define RM_SQRT3 1.7320508075688772f

// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float rm_clamp(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }
__device__ __forceinline__ float rm_sign(float x) { return copysignf(1.0f, x); }

// ---------------------------------------------------------------------------------------------
// marching core (raymarching.cu:460-500, 530-588, 1059-1119)
// ---------------------------------------------------------------------------------------------
struct RmRay {
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz;
};
struct RmCfg {
    float bound, rbound, dt_gamma, dt_min, dt_max, rH, H3, Hf, halfH, Cf;
    uint32_t H;
    const uint8_t *grid;
};

__device__ __forceinline__ RmCfg rm_cfg(float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                                        const uint8_t *grid) {
    RmCfg c;
    c.bound = bound;
    c.rbound = 1 / bound;
    c.halfH = 0.5f * (float)H;
    c.dt_gamma = dt_gamma;
    c.dt_min = 2 * RM_SQRT3 / (float)max_steps;               // :446
    c.dt_max = 2 * RM_SQRT3 * (float)(1 << (C - 1)) / (float)H;  // :447
    c.rH = 1 / (float)H;
    c.H3 = (float)(H * H * H);
    c.Hf = (float)H;
    c.Cf = (float)C;
    c.H = H;
    c.grid = grid;
    return c;
}

__device__ __forceinline__ int rm_mip(float v, float max_cascade) {
    int e;
    frexpf(v, &e);
    return (int)fminf(max_cascade - 1, fmaxf(0.0f, (float)e));
}

// Evaluates the sample at parameter t.  Same operation order as the reference (and the oracle);
// contraction is off so that every rounding matches the restatement bit for bit.
__device__ __forceinline__ bool rm_probe(const RmRay &r, const RmCfg &c, float t, float &x, float &y, float &z,
                                         float &dt, float &tt) {
#pragma clang fp contract(off)
    x = rm_clamp(r.ox + t * r.dx, -c.bound, c.bound);
    y = rm_clamp(r.oy + t * r.dy, -c.bound, c.bound);
    z = rm_clamp(r.oz + t * r.dz, -c.bound, c.bound);
    dt = rm_clamp(t * c.dt_gamma, c.dt_min, c.dt_max);
    const int m1 = rm_mip(fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z))), c.Cf);   // :42-47
    const int m2 = rm_mip((dt * c.Hf) * 0.5f, c.Cf);                             // :49-54 (x 0.5 is exact in either width)
    const int level = max(m1, m2);
    const float mip_pow = scalbnf(1.0f, level);
    const float mip_bound = fminf(mip_pow, c.bound);
    // 1 / mip_bound (:474): the reciprocal of a power of two is exact, the other case is the loop-invariant
    // 1 / bound -- the same correctly rounded quotients as the division, without a division per probe
    const float mip_rbound = mip_pow < c.bound ? scalbnf(1.0f, -level) : c.rbound;
    // :475-477 computes 0.5 * (double)v * (double)H and narrows once.  v has 24 significant bits, H at most 11:
    // the double product is exact, so the single rounding of the float product v * (0.5f * H) gives the same
    // float (0.5f * H is exact too) -- no fp64 in the probe
    const int nx = (int)rm_clamp((x * mip_rbound + 1) * c.halfH, 0.0f, (float)(c.H - 1));
    const int ny = (int)rm_clamp((y * mip_rbound + 1) * c.halfH, 0.0f, (float)(c.H - 1));
    const int nz = (int)rm_clamp((z * mip_rbound + 1) * c.halfH, 0.0f, (float)(c.H - 1));
    const uint32_t index = (uint32_t)((float)level * c.H3 + (float)rm_morton3d(nx, ny, nz));   // :479
    const bool occ = c.grid[index / 8] & (1 << (index % 8));
    if (!occ) {
        // :491-495
        const float tx = ((((float)nx + 0.5f + 0.5f * rm_sign(r.dx)) * c.rH * 2 - 1) * mip_bound - x) * r.rdx;
        const float ty = ((((float)ny + 0.5f + 0.5f * rm_sign(r.dy)) * c.rH * 2 - 1) * mip_bound - y) * r.rdy;
        const float tz = ((((float)nz + 0.5f + 0.5f * rm_sign(r.dz)) * c.rH * 2 - 1) * mip_bound - z) * r.rdz;
        tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
    }
    return occ;
}

// Returns the number of additions made (the march's step index k advances by it: k_march_count's sample mask).
__device__ __forceinline__ uint32_t rm_skip(const RmCfg &c, float &t, float tt) {
#pragma clang fp contract(off)
    // do { t += clamp(t * dt_gamma, dt_min, dt_max); } while (t < tt);  (:497) -- the same additions in the same
    // order, four per trip: the first partial sum that is not below tt is the loop's result
    uint32_t adds = 0;
    for (;;) {
        const float t1 = t + rm_clamp(t * c.dt_gamma, c.dt_min, c.dt_max);
        const float t2 = t1 + rm_clamp(t1 * c.dt_gamma, c.dt_min, c.dt_max);
        const float t3 = t2 + rm_clamp(t2 * c.dt_gamma, c.dt_min, c.dt_max);
        const float t4 = t3 + rm_clamp(t3 * c.dt_gamma, c.dt_min, c.dt_max);
        const bool b1 = t1 < tt, b2 = t2 < tt, b3 = t3 < tt, b4 = t4 < tt;
        t = !b1 ? t1 : (!b2 ? t2 : (!b3 ? t3 : t4));
        adds += !b1 ? 1u : (!b2 ? 2u : (!b3 ? 3u : 4u));
        if (!(b1 && b2 && b3 && b4)) break;
    }
    return adds;
}

__device__ __forceinline__ RmRay rm_load_ray(const float *rays_o, const float *rays_d, uint32_t n) {
    RmRay r;
    r.ox = rays_o[n * 3 + 0]; r.oy = rays_o[n * 3 + 1]; r.oz = rays_o[n * 3 + 2];
    r.dx = rays_d[n * 3 + 0]; r.dy = rays_d[n * 3 + 1]; r.dz = rays_d[n * 3 + 2];
    r.rdx = 1 / r.dx; r.rdy = 1 / r.dy; r.rdz = 1 / r.dz;
    return r;
}

// The first parameter of a ray: its start plus `noise` steps (:452, :1053).
__device__ __forceinline__ float rm_start_t(const RmCfg &c, float t, float noise) {
#pragma clang fp contract(off)
    return t + rm_clamp(t * c.dt_gamma, c.dt_min, c.dt_max) * noise;
}
