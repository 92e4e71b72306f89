// tests/cpp/anchored_zdrop_stripe_check.cpp -- the host side of the row-stripe
// z-drop rule, built with g++ -fsanitize=address,undefined and run on its own
// (tests/test_anchored_zdrop_stripe_ref.py).
//   * ta_layout.h band_stripes / band_stripe_tau_done / band_stripe_swept_steps
//     against a brute-force enumeration of the fill's step loop (lane l at
//     column c0 + t - l at step t) over random (n, m, w), multi-pass pairs and
//     passes with c0 > 1 included: tau_done is the last step at which the
//     stripe's lane computes an in-band cell of a row <= n, it strictly
//     increases with the lane, it is below the pass's step count, and the
//     swept steps of a drop at stripe g are the whole passes above plus the
//     first check (every 64th step, and the pass's last) after tau_done.
//   * ta_planner.cpp build_band_plan / build_band_affine_plan: a stripe plan
//     equals the segment plan field by field, its device block included, and
//     carries only the rule; the rule is ignored where z-drop is off.
// Prints "ok <plans> <shapes> <multi-pass shapes> <passes with c0 > 1> <stripes>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
static void same_plan(const P& a, const P& b) {
    CHECK(a.type == b.type && a.n_pairs == b.n_pairs && a.want_cigar == b.want_cigar);
    CHECK(a.match == b.match && a.mismatch == b.mismatch && a.zdrop == b.zdrop);
    CHECK(a.qlen == b.qlen && a.tlen == b.tlen && a.band == b.band && a.order == b.order);
    CHECK(a.ptr_off == b.ptr_off && a.bnd_off == b.bnd_off && a.slot_off == b.slot_off);
    CHECK(a.slots_bytes == b.slots_bytes && a.band_cells == b.band_cells && a.swept_cells == b.swept_cells);
    CHECK(a.chunks.size() == b.chunks.size());
    for (size_t c = 0; c < a.chunks.size(); ++c)
        CHECK(a.chunks[c].begin == b.chunks[c].begin && a.chunks[c].count == b.chunks[c].count);
    ta::BandArrays da, db;
    const ta::BlockSpan sa = ta::layout_block(a, da), sb = ta::layout_block(b, db);
    CHECK(sa.upload == sb.upload && sa.scratch == sb.scratch && sa.bytes == sb.bytes);
    std::vector<uint8_t> ma(sa.bytes + 1), mb(sb.bytes + 1);
    ta::bind_block(a, da, ma.data(), sa);
    ta::bind_block(b, db, mb.data(), sb);
    CHECK((uint8_t*)da.d_goal_j - ma.data() == (uint8_t*)db.d_goal_j - mb.data());
    if (a.zdrop >= 0 && a.n_pairs) {  // the step counts: the same array, inside the block
        CHECK((uint8_t*)da.d_swept - ma.data() == (uint8_t*)db.d_swept - mb.data());
        CHECK((uint8_t*)db.d_swept + 4ull * b.n_pairs <= mb.data() + sb.bytes);
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
    {
        ta::BandPlan seg, dflt, str, off, glob;
        ta::build_band_plan(dflt, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -4, cigar, budget, z);
        ta::build_band_plan(seg, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -4, cigar, budget, z,
                            ta::kZdropSegment);
        ta::build_band_plan(str, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -4, cigar, budget, z,
                            ta::kZdropStripe);
        ta::build_band_plan(off, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -4, cigar, budget, -1,
                            ta::kZdropStripe);
        ta::build_band_plan(glob, P, q.data(), t.data(), band.data(), ta::kGlobal, 2, -4, -4, cigar, budget, z,
                            ta::kZdropStripe);
        CHECK(dflt.zdrop_rule == ta::kZdropSegment && seg.zdrop_rule == ta::kZdropSegment);
        CHECK(str.zdrop_rule == ta::kZdropStripe && str.zdrop == z);
        CHECK(off.zdrop == -1 && off.zdrop_rule == ta::kZdropSegment);    // z-drop off: no rule to carry
        CHECK(glob.zdrop == -1 && glob.zdrop_rule == ta::kZdropSegment);  // ... and outside Mode kAnchored
        same_plan(seg, dflt);
        same_plan(str, seg);
        CHECK(str.gap == seg.gap && str.ws_ptr_dwords == seg.ws_ptr_dwords && str.ws_bnd_words == seg.ws_bnd_words);
        for (size_t c = 0; c < seg.chunks.size(); ++c)
            CHECK(str.chunks[c].ptr_dwords == seg.chunks[c].ptr_dwords && str.chunks[c].bnd_words == seg.chunks[c].bnd_words);
        plans += 2;
    }
    {
        ta::BandAffinePlan seg, str, off;
        ta::build_band_affine_plan(seg, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -3, -1, cigar, budget, z);
        ta::build_band_affine_plan(str, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -3, -1, cigar, budget, z,
                                   ta::kZdropStripe);
        ta::build_band_affine_plan(off, P, q.data(), t.data(), band.data(), ta::kAnchored, 2, -4, -3, -1, cigar, budget,
                                   -7, ta::kZdropStripe);
        CHECK(seg.zdrop_rule == ta::kZdropSegment && str.zdrop_rule == ta::kZdropStripe && str.zdrop == z);
        CHECK(off.zdrop == -1 && off.zdrop_rule == ta::kZdropSegment);
        same_plan(str, seg);
        CHECK(str.open == seg.open && str.extend == seg.extend);
        CHECK(str.ws_ptr_entries == seg.ws_ptr_entries && str.ws_bnd_entries == seg.ws_bnd_entries);
        for (size_t c = 0; c < seg.chunks.size(); ++c)
            CHECK(str.chunks[c].ptr_entries == seg.chunks[c].ptr_entries &&
                  str.chunks[c].bnd_entries == seg.chunks[c].bnd_entries);
        plans += 2;
    }
}

// The fill's step loop, enumerated: pass p, step t, lane l, row r.
static void check_geometry(uint32_t n, uint32_t m, uint32_t w_in, uint64_t& multipass, uint64_t& c0_above_1,
                           uint64_t& stripes) {
    const uint32_t w = ta::band_clamp(n, m, w_in);
    const int lo = ta::band_lo(n, m, w), hi = ta::band_hi(n, m, w);
    const uint32_t passes = ta::n_passes(n);
    multipass += passes > 1;
    CHECK(ta::band_stripes(n) == (n + 15) / 16);
    uint64_t total = 0;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t row_base = p * ta::kPassRows;
        const uint32_t nrows = std::min<uint32_t>(ta::kPassRows, n - row_base);
        const uint32_t nl = (nrows + ta::kRows - 1) / ta::kRows;
        const uint32_t c0 = ta::band_c0(n, m, w, p), c1 = ta::band_c1(n, m, w, p);
        c0_above_1 += c0 > 1;
        const uint32_t steps = c1 - c0 + 1 + nl - 1;
        std::vector<int64_t> last(nl, -1);  // per lane, the last step with an in-band cell of a row <= n
        for (uint32_t t = 0; t < steps; ++t)
            for (uint32_t l = 0; l < nl; ++l) {
                if (t < l || t - l > c1 - c0) continue;  // the lane is not at a column of the pass
                const uint32_t j = c0 + t - l;
                for (uint32_t r = 0; r < (uint32_t)ta::kRows; ++r) {
                    const uint32_t i = row_base + l * ta::kRows + r + 1;
                    if (i > n) break;
                    const int d = (int)j - (int)i;
                    if (d >= lo && d <= hi) last[l] = t;
                }
            }
        for (uint32_t l = 0; l < nl; ++l) {
            const uint32_t g = p * ta::kWave + l;
            CHECK(last[l] >= 0);  // no stripe is empty
            const uint32_t td = ta::band_stripe_tau_done(n, m, w, g);
            CHECK((int64_t)td == last[l]);
            CHECK(td < steps);
            if (l) CHECK(td > ta::band_stripe_tau_done(n, m, w, g - 1));  // the finished stripes are a prefix
            // the first check after step td: t = 64, 128, .. and t = steps, t counting the steps done
            uint32_t seen = 0;
            for (uint32_t t = 1; t <= steps && !seen; ++t)
                if ((t % 64 == 0 || t == steps) && td < t) seen = t;
            CHECK(seen && ta::band_stripe_swept_steps(n, m, w, g) == total + seen);
            ++stripes;
        }
        total += steps;
    }
    CHECK(ta::band_stripe_swept_steps(n, m, w, ta::band_stripes(n)) == total);
    CHECK(ta::band_stripe_swept_steps(n, m, w, ta::band_stripes(n) + 5) == total);
    CHECK(total == ta::band_drop_swept_steps(n, m, w, passes, 0));
}

int main() {
    std::mt19937_64 rng(0x2D20Au);
    uint64_t plans = 0, shapes = 0, multipass = 0, c0_above_1 = 0, stripes = 0;
    for (g_round = 0; g_round < 60; ++g_round) check_plans(rng, plans);
    const uint32_t fixed[][3] = {{1, 1, 0},        {16, 16, 0},      {17, 1, 3},      {1024, 1040, 16}, {1025, 1041, 16},
                                 {2100, 2110, 16}, {2049, 2000, 0},  {3000, 3100, 64}, {50, 5, 8},      {5, 50, 8},
                                 {300, 120, 16},   {2000, 2064, 64}, {2000, 2128, 128}, {1100, 1110, 16}};
    for (const auto& f : fixed) {
        check_geometry(f[0], f[1], f[2], multipass, c0_above_1, stripes);
        ++shapes;
    }
    for (g_round = 0; g_round < 330; ++g_round) {
        const uint32_t maxlen = (g_round % 3 == 0) ? 3300u : 200u;
        const uint32_t n = 1 + (uint32_t)(rng() % maxlen);
        const uint32_t m = (rng() % 4) ? (uint32_t)std::max<int64_t>(1, (int64_t)n + (int64_t)(rng() % 161) - 80)
                                       : 1 + (uint32_t)(rng() % maxlen);
        const uint32_t kinds[] = {0u, 1u, 15u, 16u, 17u, 64u, 0xFFFFFFFFu};
        const uint32_t w = (n > 600 && m > 600) ? kinds[rng() % 6] : kinds[rng() % 7];  // (full band: small pairs only)
        check_geometry(n, m, w, multipass, c0_above_1, stripes);
        ++shapes;
    }
    CHECK(ta::band_stripe_swept_steps(0, 5, 3, 0) == 0 && ta::band_stripe_swept_steps(5, 0, 3, 0) == 0);
    std::printf("ok %llu %llu %llu %llu %llu\n", (unsigned long long)plans, (unsigned long long)shapes,
                (unsigned long long)multipass, (unsigned long long)c0_above_1, (unsigned long long)stripes);
    return 0;
}
