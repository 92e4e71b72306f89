// tests/cpp/anchored_zdrop_plan_check.cpp -- the host side of z-drop on anchored
// alignment, built with g++ -fsanitize=address,undefined and run on its own
// (tests/test_anchored_zdrop_ref.py).
//   * ta_planner.cpp build_band_plan / build_band_affine_plan with Z on random
//     batches: a zdrop < 0 plan equals the anchored plan field by field, its
//     device block included; a zdrop >= 0 plan equals it in every sized field
//     (order, chunks, code, boundary and slot offsets, totals) and its block
//     grows by the one per-pair array of step counts; Z is ignored outside
//     Mode kAnchored.
//   * ta_layout.h band_drop_steps / band_drop_segments / band_drop_tau /
//     band_drop_swept_steps against a brute-force enumeration of the fill's
//     step loop (lane l at column c0 + t - l at step t) over random (n, m, w),
//     multi-pass pairs and passes with c0 > 1 included.
// Prints "ok <plans> <shapes> <multi-pass shapes> <passes with c0 > 1>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "ta_plan_block.h"
#include "ta_planner.h"

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "FAIL line %d: %s (round %d)\n", __LINE__, #c, g_round); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static int g_round = 0;

template <class P>
static void same_sized(const P& a, const P& b) {
    CHECK(a.type == ta::kAnchored && b.type == ta::kAnchored);
    CHECK(a.n_pairs == b.n_pairs && a.want_cigar == b.want_cigar && a.match == b.match && a.mismatch == b.mismatch);
    CHECK(a.qlen == b.qlen && a.tlen == b.tlen && a.band == b.band && a.order == b.order);
    CHECK(a.ptr_off == b.ptr_off && a.bnd_off == b.bnd_off && a.slot_off == b.slot_off);
    CHECK(a.slots_bytes == b.slots_bytes && a.band_cells == b.band_cells && a.swept_cells == b.swept_cells);
    CHECK(a.chunks.size() == b.chunks.size());
    for (size_t c = 0; c < a.chunks.size(); ++c)
        CHECK(a.chunks[c].begin == b.chunks[c].begin && a.chunks[c].count == b.chunks[c].count);
}

template <class P>
static void check_blocks(const P& off, const P& neg, const P& on) {
    ta::BandArrays d0, d1, d2;
    const ta::BlockSpan s0 = ta::layout_block(off, d0), s1 = ta::layout_block(neg, d1), s2 = ta::layout_block(on, d2);
    CHECK(s0.upload == s1.upload && s0.scratch == s1.scratch && s0.bytes == s1.bytes);
    CHECK(s2.upload == s0.upload && s2.scratch == s0.scratch);
    CHECK(s2.bytes == s0.bytes + ((4ull * on.n_pairs + 255) & ~255ull));
    // bound: the step counts lie behind the goal cells, inside the block
    std::vector<uint8_t> mem(s2.bytes + 1);
    ta::bind_block(on, d2, mem.data(), s2);
    if (on.n_pairs) {
        CHECK((uint8_t*)d2.d_swept >= (uint8_t*)d2.d_goal_j + 4ull * on.n_pairs);
        CHECK((uint8_t*)d2.d_swept + 4ull * on.n_pairs <= mem.data() + s2.bytes);
    }
}

static void check_plans(std::mt19937_64& rng, uint64_t& plans) {
    const uint32_t P = (uint32_t)(rng() % 48);
    const uint32_t maxlen = (g_round % 4 == 0) ? 4200u : 300u;  // some plans with multi-pass pairs
    std::vector<uint32_t> q(P), t(P), band(P);
    for (uint32_t p = 0; p < P; ++p) {
        q[p] = (uint32_t)(rng() % (maxlen + 1));
        t[p] = (rng() % 3) ? (uint32_t)std::max<int64_t>(0, (int64_t)q[p] + (int64_t)(rng() % 81) - 40)
                           : (uint32_t)(rng() % (maxlen + 1));
        const uint32_t kinds[] = {0u, 1u, 16u, 37u, 700u, 0xFFFFFFFFu};
        band[p] = kinds[rng() % 6];
    }
    const bool cigar = g_round % 5 != 0;
    const uint64_t budgets[] = {1ull, 4096ull, 1ull << 16, 1ull << 20, 1ull << 34};
    const uint64_t budget = budgets[rng() % 5];
    const int32_t zs[] = {0, 1, 40, 1000000, INT32_MAX};
    const int32_t z = zs[rng() % 5];
    const int32_t negs[] = {-1, -2, INT32_MIN};
    const int32_t neg = negs[rng() % 3];
    {
        ta::BandPlan off, a, b, g;
        ta::build_band_plan(off, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -4, cigar, budget);
        ta::build_band_plan(a, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -4, cigar, budget, neg);
        ta::build_band_plan(b, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -4, cigar, budget, z);
        ta::build_band_plan(g, P, q.data(), t.data(), band.data(), ta::kGlobal, 2, -4, -4, cigar, budget, z);
        CHECK(off.zdrop == -1 && a.zdrop == -1 && b.zdrop == z && g.zdrop == -1);
        same_sized(a, off);
        same_sized(b, off);
        CHECK(a.gap == off.gap && b.gap == off.gap);
        CHECK(a.ws_ptr_dwords == off.ws_ptr_dwords && a.ws_bnd_words == off.ws_bnd_words);
        CHECK(b.ws_ptr_dwords == off.ws_ptr_dwords && b.ws_bnd_words == off.ws_bnd_words);
        for (size_t c = 0; c < off.chunks.size(); ++c) {
            CHECK(a.chunks[c].ptr_dwords == off.chunks[c].ptr_dwords && a.chunks[c].bnd_words == off.chunks[c].bnd_words);
            CHECK(b.chunks[c].ptr_dwords == off.chunks[c].ptr_dwords && b.chunks[c].bnd_words == off.chunks[c].bnd_words);
        }
        check_blocks(off, a, b);
        plans += 3;
    }
    {
        ta::BandAffinePlan off, a, b;
        ta::build_band_affine_plan(off, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -3, -1, cigar, budget);
        ta::build_band_affine_plan(a, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -3, -1, cigar, budget, neg);
        ta::build_band_affine_plan(b, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -3, -1, cigar, budget, z);
        CHECK(off.zdrop == -1 && a.zdrop == -1 && b.zdrop == z);
        same_sized(a, off);
        same_sized(b, off);
        CHECK(a.open == off.open && a.extend == off.extend && b.open == off.open && b.extend == off.extend);
        CHECK(a.ws_ptr_entries == off.ws_ptr_entries && a.ws_bnd_entries == off.ws_bnd_entries);
        CHECK(b.ws_ptr_entries == off.ws_ptr_entries && b.ws_bnd_entries == off.ws_bnd_entries);
        for (size_t c = 0; c < off.chunks.size(); ++c) {
            CHECK(a.chunks[c].ptr_entries == off.chunks[c].ptr_entries && a.chunks[c].bnd_entries == off.chunks[c].bnd_entries);
            CHECK(b.chunks[c].ptr_entries == off.chunks[c].ptr_entries && b.chunks[c].bnd_entries == off.chunks[c].bnd_entries);
        }
        check_blocks(off, a, b);
        plans += 3;
    }
}

// The fill's step loop, enumerated: pass p, step t, lane l, row r.
static void check_geometry(uint32_t n, uint32_t m, uint32_t w_in, uint64_t& multipass, uint64_t& c0_above_1) {
    const uint32_t w = ta::band_clamp(n, m, w_in);
    const int lo = ta::band_lo(n, m, w), hi = ta::band_hi(n, m, w);
    const uint32_t passes = ta::n_passes(n);
    multipass += passes > 1;
    uint64_t cells = 0, total = 0;
    std::vector<uint32_t> steps_of(passes);
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t row_base = p * ta::kPassRows;
        const uint32_t nrows = std::min<uint32_t>(ta::kPassRows, n - row_base);
        const uint32_t nl = (nrows + ta::kRows - 1) / ta::kRows;
        const uint32_t c0 = ta::band_c0(n, m, w, p), c1 = ta::band_c1(n, m, w, p);
        c0_above_1 += c0 > 1;
        const uint32_t steps = c1 - c0 + 1 + nl - 1;
        CHECK(ta::band_drop_steps(n, m, w, p) == steps);
        CHECK(steps <= ta::band_pass_steps(n, m, w, p));  // the code layout holds every executed step
        CHECK(ta::band_drop_segments(n, m, w, p) == (steps + 63) / 64);
        steps_of[p] = steps;
        uint32_t last_step_with_a_cell = 0;
        for (uint32_t t = 0; t < steps; ++t)
            for (uint32_t l = 0; l < nl; ++l) {
                if (t < l || t - l > c1 - c0) continue;  // the lane is not at a column of the pass
                const uint32_t j = c0 + t - l;
                for (uint32_t r = 0; r < (uint32_t)ta::kRows; ++r) {
                    const uint32_t i = row_base + l * ta::kRows + r + 1;
                    if (i > n) break;
                    const int d = (int)j - (int)i;
                    if (d < lo || d > hi) continue;
                    CHECK(ta::band_drop_tau(n, m, w, i, j) == t);  // ... and so its segment is t / 64
                    ++cells;
                    last_step_with_a_cell = t;
                }
            }
        CHECK(last_step_with_a_cell == steps - 1);  // no trailing step without a cell
        for (uint32_t s = 0; s < (steps + 63) / 64; ++s)
            CHECK(ta::band_drop_swept_steps(n, m, w, p, s) == total + std::min<uint32_t>(64 * (s + 1), steps));
        total += steps;
    }
    CHECK(cells == ta::band_cells(n, m, w));  // every in-band interior cell has exactly one step
    CHECK(ta::band_drop_swept_steps(n, m, w, passes, 0) == total);
}

int main() {
    std::mt19937_64 rng(0x2D209u);
    uint64_t plans = 0, shapes = 0, multipass = 0, c0_above_1 = 0;
    for (g_round = 0; g_round < 60; ++g_round) check_plans(rng, plans);
    const uint32_t fixed[][3] = {{1, 1, 0},       {16, 16, 0},     {17, 1, 3},       {1024, 1040, 16}, {1025, 1041, 16},
                                 {2100, 2110, 16}, {2049, 2000, 0}, {3000, 3100, 64}, {50, 5, 8},       {5, 50, 8}};
    for (const auto& f : fixed) {
        check_geometry(f[0], f[1], f[2], multipass, c0_above_1);
        ++shapes;
    }
    for (g_round = 0; g_round < 330; ++g_round) {
        const uint32_t maxlen = (g_round % 3 == 0) ? 3300u : 200u;
        const uint32_t n = 1 + (uint32_t)(rng() % maxlen);
        const uint32_t m = (rng() % 4) ? (uint32_t)std::max<int64_t>(1, (int64_t)n + (int64_t)(rng() % 161) - 80)
                                       : 1 + (uint32_t)(rng() % maxlen);
        const uint32_t kinds[] = {0u, 1u, 15u, 16u, 17u, 64u, 0xFFFFFFFFu};
        const uint32_t w = (n > 600 && m > 600) ? kinds[rng() % 6] : kinds[rng() % 7];  // (full band: small pairs only)
        check_geometry(n, m, w, multipass, c0_above_1);
        ++shapes;
    }
    CHECK(ta::band_drop_swept_steps(0, 5, 3, 0, 0) == 0 && ta::band_drop_swept_steps(5, 0, 3, 0, 0) == 0);
    std::printf("ok %llu %llu %llu %llu\n", (unsigned long long)plans, (unsigned long long)shapes,
                (unsigned long long)multipass, (unsigned long long)c0_above_1);
    return 0;
}
