// The per-row core of the style-image k-means (nerfstyle_amd/csrc/km_core.h) compiled by the host compiler, for
// test_kmeans_cpu.py: one Lloyd step's labels, counts and int64 sums of the rows in a file.
//   in : u32 n, stride, H, W, K; f64 wxy; f64 centroids [K][5]; f32 rows [n][stride]
//   out: i32 labels [n]; i64 counts [K]; i64 sums [K][5]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../nerfstyle_amd/csrc/km_core.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t hdr[5];
    double wxy;
    if (fread(hdr, 4, 5, in) != 5 || fread(&wxy, 8, 1, in) != 1) return 4;
    const uint32_t n = hdr[0], stride = hdr[1], H = hdr[2], W = hdr[3], K = hdr[4];
    if (n == 0 || n > KM_MAX_ROWS || (stride != 3 && stride != 4) || K == 0 || K > 64) return 5;
    std::vector<double> cent((size_t)K * KM_FEATS);
    std::vector<float> rows((size_t)n * stride);
    if (fread(cent.data(), 8, cent.size(), in) != cent.size() || fread(rows.data(), 4, rows.size(), in) != rows.size()) return 6;
    fclose(in);
    const KmGeom G = km_geom(H, W, wxy);
    std::vector<int32_t> labels(n, -1);
    std::vector<int64_t> counts(K, 0), sums((size_t)K * KM_FEATS, 0);
    for (uint32_t i = 0; i < n; i++) {
        const float *p = &rows[(size_t)i * stride];
        if (!km_valid(p[0], p[1], p[2])) continue;
        double f[KM_FEATS], d;
        km_feature(G, i, p[0], p[1], p[2], f);
        const uint32_t k = km_assign(f, cent.data(), K, d);
        labels[i] = (int32_t)k;
        counts[k]++;
        for (int j = 0; j < KM_FEATS; j++) sums[(size_t)k * KM_FEATS + j] += km_quant(f[j]);
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 7;
    fwrite(labels.data(), 4, labels.size(), out);
    fwrite(counts.data(), 8, counts.size(), out);
    fwrite(sums.data(), 8, sums.size(), out);
    return fclose(out) == 0 ? 0 : 8;
}
