// tests/cpp/band_affine_plan_check.cpp -- the host planner of the banded
// affine family (ta_planner.cpp build_band_affine_plan) on random batches,
// built with g++ -fsanitize=address,undefined and run on its own
// (tests/test_banded_affine_ref.py).  Checks, per plan: every pair in exactly
// one chunk; a chunk's code bytes within the budget unless it holds a single
// pair; the pairs' code and boundary regions disjoint inside their chunk and
// sized band_ptr_dwords / bnd_words entries; the totals of band and swept
// cells; the workspace the largest chunk's.  Prints "ok <plans> <chunks>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
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

static bool disjoint(std::vector<std::pair<uint64_t, uint64_t>> v, uint64_t limit) {
    std::sort(v.begin(), v.end());
    uint64_t at = 0;
    for (const auto& r : v) {
        if (r.first < at) return false;
        at = r.first + r.second;
    }
    return at <= limit;
}

int main() {
    std::mt19937_64 rng(0xBAFFu);
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
        ta::BandAffinePlan pl;
        ta::build_band_affine_plan(pl, P, q.data(), t.data(), band.data(), (int)(g_plan % 3), 1, -1, -2, -1, cigar,
                                   budget);
        CHECK(pl.n_pairs == P && pl.open == -2 && pl.extend == -1 && pl.want_cigar == cigar);
        CHECK(pl.order.size() == P && pl.band.size() == P && pl.ptr_off.size() == P && pl.bnd_off.size() == P);
        std::vector<int> seen(P, 0);
        uint64_t ws_ptr = 0, ws_bnd = 0, at = 0, cells = 0, swept = 0, slots = 0;
        for (const auto& c : pl.chunks) {
            CHECK(c.begin == at && c.count > 0);
            at += c.count;
            std::vector<std::pair<uint64_t, uint64_t>> codes, bnds;
            uint64_t need = 0;
            for (uint32_t k = c.begin; k < c.begin + c.count; ++k) {
                const uint32_t p = pl.order[k];
                CHECK(p < P);
                ++seen[p];
                CHECK(pl.band[p] == ta::band_clamp(q[p], t[p], band[p]));
                const uint64_t e = cigar ? ta::band_ptr_dwords(q[p], t[p], pl.band[p]) : 0;
                codes.push_back({pl.ptr_off[p], e});
                bnds.push_back({pl.bnd_off[p], ta::bnd_words(q[p], t[p])});
                need += e;
            }
            CHECK(need == c.ptr_entries);
            CHECK(disjoint(codes, c.ptr_entries));
            CHECK(disjoint(bnds, c.bnd_entries));
            if (c.ptr_entries * 8 > budget) CHECK(c.count == 1);
            ws_ptr = std::max(ws_ptr, c.ptr_entries);
            ws_bnd = std::max(ws_bnd, c.bnd_entries);
            ++chunks;
        }
        CHECK(at == P);
        for (uint32_t p = 0; p < P; ++p) {
            CHECK(seen[p] == 1);
            cells += ta::band_cells(q[p], t[p], band[p]);
            swept += ta::band_swept_cells(q[p], t[p], band[p]);
            CHECK(pl.slot_off[p] == slots);
            slots += ta::cigar_slot_bytes(q[p], t[p]);
        }
        CHECK(pl.band_cells == cells && pl.swept_cells == swept && pl.slots_bytes == slots);
        CHECK(pl.ws_ptr_entries == ws_ptr && pl.ws_bnd_entries == ws_bnd);
        // launch order: descending swept cells
        for (uint32_t k = 1; k < P; ++k)
            CHECK(ta::band_swept_cells(q[pl.order[k - 1]], t[pl.order[k - 1]], band[pl.order[k - 1]]) >=
                  ta::band_swept_cells(q[pl.order[k]], t[pl.order[k]], band[pl.order[k]]));
    }
    std::printf("ok %d %llu\n", g_plan, (unsigned long long)chunks);
    return 0;
}
