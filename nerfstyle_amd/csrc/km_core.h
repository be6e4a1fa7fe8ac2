// One pixel row of the style-image k-means (include/nsr.h, "Style image clustering"): validity, the 5-D feature, the nearest
// centroid and the fixed-point form of the feature, written once in plain C++ for the device (kmeans.hip) and for the host
// (tests/kmeans_host.cpp compiles it with the host compiler).  Everything is fp64 from the f32 inputs and nothing is contracted
// (the pragma below; a host compiler that does not know it is given -ffp-contract=off), so that the device, the host program
// and the NumPy restatement (tests/kmeans_ref.py) run the same sequence of correctly rounded IEEE operations.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define KM_FN __host__ __device__ __forceinline__
#else
#define KM_FN static inline
#endif

#define KM_FEATS 5
#define KM_MAX_ROWS (1ull << 27)          // n <= 2^27 and |f| <= 8: |sum llrint(f 2^32)| <= 2^62
#define KM_FIXED_ONE 4294967296.0         // 2^32

// the layout of the rows and the weight of the position terms: m = max(H, W) as a double
struct KmGeom {
    uint32_t W, H;
    double wxy, m;
};
KM_FN KmGeom km_geom(uint32_t H, uint32_t W, double wxy) { return KmGeom{W, H, wxy, (double)(H > W ? H : W)}; }

// labelled: every colour component in [-8, 8] (NaN fails the comparison, an infinity is outside)
KM_FN bool km_valid(float r, float g, float b) { return fabsf(r) <= 8.0f && fabsf(g) <= 8.0f && fabsf(b) <= 8.0f; }

// f = (r, g, b, wxy * x / m, wxy * y / m) of row i, x = i % W, y = (i / W) % H; wxy == 0 gives +0.0 either way
KM_FN void km_feature(const KmGeom &G, uint32_t i, float r, float g, float b, double (&f)[KM_FEATS]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    f[0] = (double)r; f[1] = (double)g; f[2] = (double)b;
    f[3] = 0.0; f[4] = 0.0;
    if (G.wxy != 0.0) {
        const uint32_t q = i / G.W, x = i - q * G.W, y = q % G.H;
        f[3] = G.wxy * (double)x / G.m;
        f[4] = G.wxy * (double)y / G.m;
    }
}

// d = ((((t0 t0 + t1 t1) + t2 t2) + t3 t3) + t4 t4), t_j = f_j - c_j
KM_FN double km_dist(const double (&f)[KM_FEATS], const double *c) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double t0 = f[0] - c[0], t1 = f[1] - c[1], t2 = f[2] - c[2], t3 = f[3] - c[3], t4 = f[4] - c[4];
    return t0 * t0 + t1 * t1 + t2 * t2 + t3 * t3 + t4 * t4;
}

// the k of the smallest d_k, the lowest k among equals: k replaces the best so far only when d_k < d_best
KM_FN uint32_t km_assign(const double (&f)[KM_FEATS], const double *cent, uint32_t K, double &dbest) {
    uint32_t best = 0;
    dbest = km_dist(f, cent);
    for (uint32_t k = 1; k < K; k++) {
        const double d = km_dist(f, cent + k * KM_FEATS);
        if (d < dbest) { dbest = d; best = k; }
    }
    return best;
}

// f 2^32 is exact; llrint rounds to nearest, ties to even
KM_FN int64_t km_quant(double f) { return (int64_t)llrint(f * KM_FIXED_ONE); }
