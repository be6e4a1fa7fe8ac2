// The labelling of the occupancy components (nerfstyle_amd/csrc/occ_cc_core.h over uf_core.h) compiled for the host and run
// from many threads: the code the union kernel runs a thread a bitfield byte, here a thread a stride of bytes.  Reads a file
// {uint32 C, uint32 H, C*H^3/8 bitfield bytes}, prints C*H^3 labels, one a line (the smallest cell id of the component, -1 at
// an unoccupied cell).  Built and run by tests/test_occ_cull_cpu.py:
//     c++ -O2 -std=c++17 -pthread tests/occ_cc_host.cpp -o occ_cc_host && ./occ_cc_host bitfield.bin [threads]
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../nerfstyle_amd/csrc/occ_cc_core.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const unsigned T = argc > 2 ? (unsigned)atoi(argv[2]) : 16u;
    FILE *f = fopen(argv[1], "rb");
    uint32_t dims[2];
    if (!f || fread(dims, 4, 2, f) != 2) return 2;
    const uint32_t C = dims[0], H = dims[1];
    if (C < 1 || C > 8 || H < 8 || H > 512 || (H & (H - 1)) || T < 1) return 2;
    const uint32_t N = C * (H * H * H / 8), cells = N * 8;
    std::vector<uint8_t> bits(N);
    if (fread(bits.data(), 1, N, f) != N) return 2;
    fclose(f);

    const uint32_t NONE = 0xffffffffu;
    std::vector<uint32_t> parent(cells);
    for (uint32_t u = 0; u < cells; u++) parent[u] = ((bits[u >> 3] >> (u & 7)) & 1) ? u : NONE;
    const auto all_threads = [&](auto body) {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < T; t++) pool.emplace_back(body, t);
        for (auto &th : pool) th.join();
    };
    // neighbouring bytes go to different threads, so the unions of one component race
    all_threads([&](unsigned t) {
        for (uint32_t n = t; n < N; n += T) occ_cc_unite_block(parent.data(), occ_cc_block(bits.data(), H, n));
    });
    all_threads([&](unsigned t) {
        for (uint32_t u = t; u < cells; u += T)
            if (uf_load(&parent[u]) != NONE) uf_min(&parent[u], uf_find(parent.data(), u));
    });
    for (uint32_t u = 0; u < cells; u++) printf("%d\n", (int)parent[u]);
    return 0;
}
