// The union-find core of the mesh cleaning (nerfstyle_amd/csrc/uf_core.h), compiled for the host and run from many threads:
// unite() over adversarial edge lists, the edges dealt round-robin so that neighbouring edges race, then the flattened labels
// against the sequential answer (the smallest id of every component).  Built and run by tests/test_mesh_clean_cpu.py:
//     c++ -O2 -std=c++17 -pthread tests/uf_stress.cpp -o uf_stress && ./uf_stress [threads] [rounds]
// Exit status 0 and "ok" when every list agrees.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../nerfstyle_amd/csrc/uf_core.h"

typedef std::vector<std::pair<uint32_t, uint32_t>> Edges;

static std::vector<uint32_t> sequential(uint32_t V, const Edges &edges) {
    std::vector<uint32_t> parent(V);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    for (const auto &e : edges) {
        const uint32_t a = find(e.first), b = find(e.second);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    std::vector<uint32_t> label(V);
    for (uint32_t v = 0; v < V; v++) label[v] = find(v);
    return label;
}

static std::vector<uint32_t> threaded(uint32_t V, const Edges &edges, unsigned threads) {
    std::vector<uint32_t> parent(V);
    std::iota(parent.begin(), parent.end(), 0u);
    uint32_t *p = parent.data();
    std::vector<std::thread> pool;
    std::atomic<unsigned> waiting(threads);         // the threads start their edges together
    for (unsigned t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            waiting.fetch_sub(1);
            while (waiting.load() != 0) std::this_thread::yield();
            for (size_t i = t; i < edges.size(); i += threads) uf_unite(p, edges[i].first, edges[i].second);
        });
    for (auto &th : pool) th.join();
    // the flatten pass, again from every thread: each label becomes the root (the kernel's k_mc_flatten)
    pool.clear();
    for (unsigned t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (uint32_t v = t; v < V; v += threads) uf_min(p + v, uf_find(p, v));
        });
    for (auto &th : pool) th.join();
    return parent;
}

static Edges relabel(const Edges &edges, const std::vector<uint32_t> &ids) {
    Edges out;
    for (const auto &e : edges) out.emplace_back(ids[e.first], ids[e.second]);
    return out;
}

int main(int argc, char **argv) {
    const unsigned threads = argc > 1 ? (unsigned)atoi(argv[1]) : 16u;
    const int rounds = argc > 2 ? atoi(argv[2]) : 3;
    const uint32_t V = 200000;
    std::mt19937 rng(12345);
    std::vector<uint32_t> ascending(V), descending(V), shuffled(V);
    std::iota(ascending.begin(), ascending.end(), 0u);
    for (uint32_t v = 0; v < V; v++) descending[v] = V - 1 - v;
    shuffled = ascending;
    std::shuffle(shuffled.begin(), shuffled.end(), rng);

    Edges chain, star, strip, sparse;
    for (uint32_t v = 0; v + 1 < V; v++) chain.emplace_back(v, v + 1);
    for (uint32_t v = 0; v + 1 < V; v++) star.emplace_back(V - 1, v);              // every union contends for one root
    for (uint32_t v = 0; v + 2 < V; v++) strip.emplace_back(v, v + 1), strip.emplace_back(v + 1, v + 2);
    for (uint32_t i = 0; i < V / 2; i++) sparse.emplace_back(rng() % V, rng() % V);  // many components, self loops among them

    struct Case {
        std::string name;
        Edges edges;
    };
    std::vector<Case> cases = {{"chain ascending", chain},
                               {"chain descending", relabel(chain, descending)},
                               {"chain shuffled", relabel(chain, shuffled)},
                               {"star hub V-1", star},
                               {"star shuffled", relabel(star, shuffled)},
                               {"strip shuffled", relabel(strip, shuffled)},
                               {"sparse random", sparse}};
    int failures = 0;
    for (const auto &c : cases) {
        const std::vector<uint32_t> want = sequential(V, c.edges);
        for (int r = 0; r < rounds; r++) {
            const std::vector<uint32_t> got = threaded(V, c.edges, threads);
            if (got != want) {
                size_t bad = 0;
                while (got[bad] == want[bad]) bad++;
                printf("MISMATCH %s round %d: label[%zu] = %u, sequential %u\n", c.name.c_str(), r, bad, got[bad], want[bad]);
                failures++;
            }
        }
    }
    printf("%s: %zu edge lists x %d rounds, %u threads\n", failures ? "FAILED" : "ok", cases.size(), rounds, threads);
    return failures ? 1 : 0;
}
