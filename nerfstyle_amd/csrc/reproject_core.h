// One destination pixel of the view reprojection (include/nsr.h, "View reprojection"), steps 1 to 6, written once in plain
// C++ for the device (reproject.hip, a thread a (pair, pixel)) and for the host (tests/reproject_host.cpp compiles it with the
// host compiler).  Everything is fp64 from the f32 inputs, nothing is contracted (the pragma below; a host compiler that does
// not know it is given -ffp-contract=off), and every sum is written in the order the header states, so that the device, the
// host program and the NumPy restatement (tests/reproject_ref.py) run the same sequence of correctly rounded IEEE operations.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RP_FN __host__ __device__ __forceinline__
#else
#define RP_FN static inline
#endif

// the pinhole and the signs of the camera flip (ray_pose.h, ru_flip: bits [2, 1, 0] negate axes 0, 1, 2)
struct RpCamera {
    double fx, fy, cx, cy, f0, f1, f2;
    uint32_t W, H;
};
RP_FN RpCamera rp_camera(float fx, float fy, float cx, float cy, uint32_t W, uint32_t H, int camera_flip) {
    return RpCamera{(double)fx, (double)fy, (double)cx, (double)cy, (camera_flip >> 2) & 1 ? -1.0 : 1.0,
                    (camera_flip >> 1) & 1 ? -1.0 : 1.0, (camera_flip >> 0) & 1 ? -1.0 : 1.0, W, H};
}

// one frame: its pose [3,4] camera to world and its own H*W rows of dist and rgb
struct RpFrame {
    double R[3][3], o[3];
    const float *dist, *rgb;
};
RP_FN RpFrame rp_frame(const float *pose, const float *dist, const float *rgb) {
    RpFrame f;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) f.R[r][c] = (double)pose[r * 4 + c];
        f.o[r] = (double)pose[r * 4 + 3];
    }
    f.dist = dist; f.rgb = rgb;
    return f;
}

// "a surface": finite and > 0 (NaN fails both comparisons)
RP_FN bool rp_surface(float t) { return t > 0.0f && t <= 3.40282346638528859812e38f; }

// the bilinear mean of four taps: the two rows along x first, then along y
RP_FN double rp_bilinear(double v00, double v01, double v10, double v11, double ax, double ay) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double top = v00 * (1.0 - ax) + v01 * ax;
    const double bot = v10 * (1.0 - ax) + v11 * ax;
    return top * (1.0 - ay) + bot * ay;
}

// dst pixel p of frame A seen from frame B -> valid; out = the three bilinear colour means in fp64 (untouched when invalid)
RP_FN bool rp_reproject_pixel(const RpCamera &C, const RpFrame &A, const RpFrame &B, uint32_t p, double depth_tol, double (&out)[3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    // 1. the dst surface
    const float tf = A.dist[p];
    if (!rp_surface(tf)) return false;
    const double t = (double)tf;
    // 2. the ray of generate_rays and the world point
    const uint32_t py = p / C.W, px = p - py * C.W;
    const double c0 = (((double)px + 0.5 - C.cx) / C.fx) * C.f0, c1 = (((double)py + 0.5 - C.cy) / C.fy) * C.f1, c2 = C.f2;
    double v[3], X[3], dx[3];
    for (int r = 0; r < 3; r++) v[r] = A.R[r][0] * c0 + A.R[r][1] * c1 + A.R[r][2] * c2;
    const double nrm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int r = 0; r < 3; r++) {
        X[r] = A.o[r] + t * (v[r] / nrm);
        dx[r] = X[r] - B.o[r];
    }
    // 3. into the src camera
    const double q0 = B.R[0][0] * dx[0] + B.R[1][0] * dx[1] + B.R[2][0] * dx[2];
    const double q1 = B.R[0][1] * dx[0] + B.R[1][1] * dx[1] + B.R[2][1] * dx[2];
    const double q2 = B.R[0][2] * dx[0] + B.R[1][2] * dx[1] + B.R[2][2] * dx[2];
    const double z = q2 * C.f2;
    if (!(z > 0.0)) return false;
    // 4. index coordinates (pixel centres at the integers)
    const double u = C.fx * (q0 * C.f0 / z) + C.cx - 0.5, w = C.fy * (q1 * C.f1 / z) + C.cy - 0.5;
    const double umax = (double)(C.W - 1), wmax = (double)(C.H - 1);
    if (!(u >= 0.0 && u <= umax && w >= 0.0 && w <= wmax)) return false;
    const double xf = fmin(floor(u), umax - 1.0), yf = fmin(floor(w), wmax - 1.0);
    const double ax = u - xf, ay = w - yf;
    const uint32_t i00 = (uint32_t)yf * C.W + (uint32_t)xf, i01 = i00 + 1, i10 = i00 + C.W, i11 = i10 + 1;
    // 5. the depth test against the src surface
    const float t00 = B.dist[i00], t01 = B.dist[i01], t10 = B.dist[i10], t11 = B.dist[i11];
    if (!(rp_surface(t00) && rp_surface(t01) && rp_surface(t10) && rp_surface(t11))) return false;
    const double tbar = rp_bilinear((double)t00, (double)t01, (double)t10, (double)t11, ax, ay);
    const double r = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
    if (!(fabs(r - tbar) <= depth_tol * r)) return false;
    // 6. the colour
    for (int k = 0; k < 3; k++)
        out[k] = rp_bilinear((double)B.rgb[(size_t)i00 * 3 + k], (double)B.rgb[(size_t)i01 * 3 + k], (double)B.rgb[(size_t)i10 * 3 + k],
                             (double)B.rgb[(size_t)i11 * 3 + k], ax, ay);
    return true;
}

// the pixel's term of sse: ((e0^2 + e1^2) + e2^2), e = warped (fp64) - rgb of the dst pixel
RP_FN double rp_sq_error(const double (&wc)[3], const float *rgb_dst) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double e0 = wc[0] - (double)rgb_dst[0], e1 = wc[1] - (double)rgb_dst[1], e2 = wc[2] - (double)rgb_dst[2];
    return (e0 * e0 + e1 * e1) + e2 * e2;
}
