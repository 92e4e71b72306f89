// scripts/exp/planner_time.cpp -- host planning time of build_plan and
// build_affine_plan (bioinfo1_amd/csrc/ta_planner.cpp), no GPU:
//   g++ -std=c++17 -O2 -I bioinfo1_amd/csrc scripts/exp/planner_time.cpp bioinfo1_amd/csrc/ta_planner.cpp -o planner_time
//   ./planner_time        one line "SHAPE linear_ns affine_ns" per shape (ns per call)
// Shapes: 1 and 3 pairs of 1 kb (the drop-in call), 10,000 pairs of 1 kb
// (config 2), 10,000 and 100,000 ragged pairs of 200..3000 (configs 3, 5).
// scripts/exp/planner_stages_ab.py builds it against two planners and alternates them.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ta_planner.h"

namespace {

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ns per call of fn, over at least 0.1 s and 3 calls
template <class F>
double time_ns(F fn) {
    using clock = std::chrono::steady_clock;
    fn();  // warm the allocator
    uint64_t calls = 0;
    const auto t0 = clock::now();
    double ns = 0;
    do {
        fn();
        ++calls;
        ns = std::chrono::duration<double, std::nano>(clock::now() - t0).count();
    } while (ns < 1e8 || calls < 3);
    return ns / calls;
}

}  // namespace

int main() {
    struct Shape {
        const char* name;
        uint32_t pairs;
        bool ragged;
    };
    const Shape shapes[] = {{"1x1kb", 1, false}, {"3x1kb", 3, false}, {"10000x1kb", 10000, false},
                            {"10000xragged", 10000, true}, {"100000xragged", 100000, true}};
    uint64_t sink = 0;
    for (const Shape& sh : shapes) {
        std::vector<uint32_t> q(sh.pairs, 1000), t(sh.pairs, 1000);
        uint64_t s = 0x7374616765ull;
        if (sh.ragged)
            for (uint32_t p = 0; p < sh.pairs; ++p) {
                q[p] = 200 + (uint32_t)(splitmix(s) % 2801);
                t[p] = 200 + (uint32_t)(splitmix(s) % 2801);
            }
        ta::Plan pl;
        const double linear = time_ns([&] {
            ta::build_plan(pl, sh.pairs, q.data(), t.data(), ta::kLocal, 1, -1, -1, true, 1ull << 30, 0, 1024);
            sink += pl.chunks.size();
        });
        ta::AffinePlan ap;
        const double affine = time_ns([&] {
            ta::build_affine_plan(ap, sh.pairs, q.data(), t.data(), ta::kGlobal, 1, -1, -2, -1, true, 1ull << 30, 0, 1024);
            sink += ap.chunks.size();
        });
        std::printf("%s %.1f %.1f\n", sh.name, linear, affine);
    }
    return sink == 0;
}
