// The per-pixel body of the view reprojection (nerfstyle_amd/csrc/reproject_core.h) compiled for the host: the code a thread of
// k_reproject runs for its (pair, dst pixel), here in a loop.  Reads a file
//   {uint32 F, H, W, P; int32 camera_flip; float fx, fy, cx, cy; double depth_tol; poses [F,12] f32; dist [F,H*W] f32;
//    rgb [F,H*W,3] f32; pairs [P,2] int32}
// and writes {mask [P,H*W] uint8; warped [P,H*W,3] f32; stats [P,2] f64 (sse added in pixel order, n_valid)}.
// Built and run by tests/test_reproject_cpu.py:
//     c++ -O2 -std=c++17 -ffp-contract=off tests/reproject_host.cpp -o reproject_host && ./reproject_host in.bin out.bin
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nerfstyle_amd/csrc/reproject_core.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    uint32_t dims[4];
    int32_t flip;
    float k[4];
    double tol;
    if (!f || fread(dims, 4, 4, f) != 4 || fread(&flip, 4, 1, f) != 1 || fread(k, 4, 4, f) != 4 || fread(&tol, 8, 1, f) != 1) return 2;
    const uint32_t F = dims[0], H = dims[1], W = dims[2], P = dims[3];
    if (F < 1 || H < 2 || W < 2 || (uint64_t)H * W > (1u << 24) || F > 64 || P > 64) return 2;
    const size_t HW = (size_t)H * W;
    std::vector<float> poses(F * 12), dist(F * HW), rgb(F * HW * 3);
    std::vector<int32_t> pairs(P * 2);
    if (fread(poses.data(), 4, poses.size(), f) != poses.size() || fread(dist.data(), 4, dist.size(), f) != dist.size() ||
        fread(rgb.data(), 4, rgb.size(), f) != rgb.size() || fread(pairs.data(), 4, pairs.size(), f) != pairs.size())
        return 2;
    fclose(f);

    const RpCamera cam = rp_camera(k[0], k[1], k[2], k[3], W, H, flip);
    std::vector<uint8_t> mask(P * HW, 0);
    std::vector<float> warped(P * HW * 3, 0.0f);
    std::vector<double> stats(P * 2, 0.0);
    for (uint32_t i = 0; i < P; i++) {
        const uint32_t a = (uint32_t)pairs[2 * i], b = (uint32_t)pairs[2 * i + 1];
        if (a >= F || b >= F) continue;
        const RpFrame A = rp_frame(&poses[a * 12], &dist[a * HW], &rgb[a * HW * 3]);
        const RpFrame B = rp_frame(&poses[b * 12], &dist[b * HW], &rgb[b * HW * 3]);
        for (uint32_t p = 0; p < HW; p++) {
            double wc[3] = {0.0, 0.0, 0.0};
            if (!rp_reproject_pixel(cam, A, B, p, tol, wc)) continue;
            mask[i * HW + p] = 1;
            for (int c = 0; c < 3; c++) warped[(i * HW + p) * 3 + c] = (float)wc[c];
            stats[2 * i] += rp_sq_error(wc, A.rgb + (size_t)p * 3);
            stats[2 * i + 1] += 1.0;
        }
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o || fwrite(mask.data(), 1, mask.size(), o) != mask.size() || fwrite(warped.data(), 4, warped.size(), o) != warped.size() ||
        fwrite(stats.data(), 8, stats.size(), o) != stats.size())
        return 3;
    fclose(o);
    return 0;
}
