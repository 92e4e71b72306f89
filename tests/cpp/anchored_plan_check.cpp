// tests/cpp/anchored_plan_check.cpp -- the host planner of the two banded
// families in Mode kAnchored (ta_planner.cpp build_band_plan /
// build_band_affine_plan) on random batches, built with g++
// -fsanitize=address,undefined and run on its own (tests/test_anchored_ref.py).
// Checks, per batch and family: the plan carries the new mode; every pair in
// exactly one chunk; and its order, chunks, code, boundary and slot offsets and
// all its totals equal the global plan's of the same batch -- an anchored plan
// is sized as a global one.  Prints "ok <plans> <chunks>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ta_planner.h"

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "FAIL line %d: %s (plan %d)\n", __LINE__, #c, g_plan); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static int g_plan = 0;

template <class P>
static void same_base(const P& a, const P& g, uint32_t n) {
    CHECK(a.type == ta::kAnchored && g.type == ta::kGlobal);
    CHECK(a.n_pairs == n && g.n_pairs == n && a.want_cigar == g.want_cigar);
    CHECK(a.match == g.match && a.mismatch == g.mismatch);
    CHECK(a.qlen == g.qlen && a.tlen == g.tlen && a.band == g.band && a.order == g.order);
    CHECK(a.ptr_off == g.ptr_off && a.bnd_off == g.bnd_off && a.slot_off == g.slot_off);
    CHECK(a.slots_bytes == g.slots_bytes && a.band_cells == g.band_cells && a.swept_cells == g.swept_cells);
    CHECK(a.chunks.size() == g.chunks.size());
    std::vector<int> seen(n, 0);
    uint32_t at = 0;
    for (size_t c = 0; c < a.chunks.size(); ++c) {
        CHECK(a.chunks[c].begin == g.chunks[c].begin && a.chunks[c].count == g.chunks[c].count);
        CHECK(a.chunks[c].begin == at && a.chunks[c].count > 0);
        for (uint32_t k = at; k < at + a.chunks[c].count; ++k) {
            CHECK(a.order[k] < n);
            ++seen[a.order[k]];
        }
        at += a.chunks[c].count;
    }
    CHECK(at == n);
    for (uint32_t p = 0; p < n; ++p) CHECK(seen[p] == 1);
}

int main() {
    std::mt19937_64 rng(0xA2C4u);
    uint64_t chunks = 0;
    for (g_plan = 0; g_plan < 160; ++g_plan) {
        const uint32_t P = (uint32_t)(rng() % 48);
        const uint32_t maxlen = (g_plan % 4 == 0) ? 4200u : 300u;  // some plans with multi-pass pairs
        std::vector<uint32_t> q(P), t(P), band(P);
        for (uint32_t p = 0; p < P; ++p) {
            q[p] = (uint32_t)(rng() % (maxlen + 1));
            t[p] = (rng() % 3) ? (uint32_t)std::max<int64_t>(0, (int64_t)q[p] + (int64_t)(rng() % 81) - 40)
                               : (uint32_t)(rng() % (maxlen + 1));
            const uint32_t kinds[] = {0u, 1u, 16u, 37u, 700u, 0xFFFFFFFFu};
            band[p] = kinds[rng() % 6];
        }
        const bool cigar = g_plan % 5 != 0;
        const uint64_t budgets[] = {1ull, 4096ull, 1ull << 16, 1ull << 20, 1ull << 34};
        const uint64_t budget = budgets[rng() % 5];
        {
            ta::BandPlan a, g;
            ta::build_band_plan(a, P, q.data(), t.data(), band.data(), ta::kAnchored, 1, -1, -1, cigar, budget);
            ta::build_band_plan(g, P, q.data(), t.data(), band.data(), ta::kGlobal, 1, -1, -1, cigar, budget);
            same_base(a, g, P);
            CHECK(a.gap == -1 && a.ws_ptr_dwords == g.ws_ptr_dwords && a.ws_bnd_words == g.ws_bnd_words);
            for (size_t c = 0; c < a.chunks.size(); ++c)
                CHECK(a.chunks[c].ptr_dwords == g.chunks[c].ptr_dwords && a.chunks[c].bnd_words == g.chunks[c].bnd_words);
            uint64_t codes = 0;
            for (uint32_t p = 0; p < P; ++p) codes += cigar ? ta::band_ptr_dwords(q[p], t[p], a.band[p]) : 0;
            uint64_t in_chunks = 0;
            for (const auto& c : a.chunks) in_chunks += c.ptr_dwords;
            CHECK(codes == in_chunks);
            chunks += a.chunks.size();
        }
        {
            ta::BandAffinePlan a, g;
            ta::build_band_affine_plan(a, P, q.data(), t.data(), band.data(), ta::kAnchored, 1, -1, -2, -1, cigar, budget);
            ta::build_band_affine_plan(g, P, q.data(), t.data(), band.data(), ta::kGlobal, 1, -1, -2, -1, cigar, budget);
            same_base(a, g, P);
            CHECK(a.open == -2 && a.extend == -1);
            CHECK(a.ws_ptr_entries == g.ws_ptr_entries && a.ws_bnd_entries == g.ws_bnd_entries);
            for (size_t c = 0; c < a.chunks.size(); ++c)
                CHECK(a.chunks[c].ptr_entries == g.chunks[c].ptr_entries &&
                      a.chunks[c].bnd_entries == g.chunks[c].bnd_entries);
            chunks += a.chunks.size();
        }
    }
    std::printf("ok %d %llu\n", 2 * g_plan, (unsigned long long)chunks);
    return 0;
}
