// bioinfo1_amd/csrc/ta_planner.cpp -- host planning of linear-gap, affine and
// banded batches (ta_planner.h).  No HIP: the device drivers (ta_api.hip,
// ta_affine.hip, ta_banded.hip) upload what this computes.  A plan is built in
// stages: census, units, layout and walk choice (linear only),
// then the chunk assembly and the ticketing the families share.
#include "ta_planner.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <numeric>

namespace ta {

// The flexible fill keeps V = S - O within a wave's span: 1,024 rows + 2 x 64
// columns of cells whose neighbours differ by at most |score| + |gap| <= 2*mag
// (plus the 64-step drift between rebases).  Global / semi keep S = H - ma*j +
// gap*(j - i): a vertical step of S lies in [0, hs - 2*gap] (H moves by
// [gap, hs - gap] down a column) and a horizontal one within 4*mag, so the span
// is at most (3*1024 + 8*64 + 8)*mag -- inside the same bound for mag <= 6.
// Local mode also ranks a column's 16 rows by 16 * (V_r - V_0) + 15 - r,
// within 16 * 15 * 2 * mag.
bool flex_fits(int mode, int ma, int mi, int gap) {
    (void)mode;
    const long long mag = std::max({1LL, std::llabs(ma), std::llabs(mi), std::llabs(gap)});
    return (kPassRows + 3LL * kWave) * 2 * mag * 2 <= 30000;
}

// Local mode: the values a wave holds lie in [0, 0x7BFF] (ta_flex.hip: the
// three-input max on f16 bit patterns) -- the frame of ta_layout.h
// flex_local_c0: above the lane-uniform clamp base zu (kept within 64 steps of
// drift of c0) by at most 15 rows of |gap| plus H <= hmax, candidates one step
// (mag) below or above.
bool flex_local_fits(uint32_t n, uint32_t m, int ma, int mi, int gap) {
    const long long mag = std::max({1LL, std::llabs(ma), std::llabs(mi), std::llabs(gap)});
    const long long hmax = (long long)std::min(n, m) * std::max({0LL, (long long)ma, (long long)mi}) +
                           ((long long)n + m) * std::max(0LL, (long long)gap);
    const long long c0 = flex_local_c0(ma, mi, gap);
    const long long hi = c0 + 64LL * std::max(0, gap - ma) + 15LL * std::max(0, -gap) + hmax + 16 * mag;
    return mag <= 64 && hi <= 0x7BFF && hmax + 3LL * kWave * std::llabs(ma) + 8 * mag <= 30000;
}

// Checkpoints of the flexible fill hold H itself as int16 (ta_flex.hip CK), and the
// recomputing walk keeps a window of a global / semi pair as S minus its corner's bias
// part, H plus at most (|gap| + |gap - ma|) x 48 (ta_walk_ck.hip): H must lie within
// +-30,000 for rows to n + 15 (semi H >= gap min(i, j), global (i + j) min(0, gap);
// H <= hs min(i, j) + (i + j) max(0, gap)); local values also meet flex_local_fits.
bool flex_ck_fits(int mode, uint32_t n, uint32_t m, int ma, int mi, int gap) {
    const long long N = (long long)n + 16, M = m, g = gap, K = std::min(N, M);
    const long long mag = std::max({1LL, std::llabs(ma), std::llabs(mi), std::llabs(gap)});
    const long long hi = K * std::max({0LL, (long long)ma, (long long)mi}) + (N + M) * std::max(0LL, g);
    const long long lo = mode == kLocal ? 0 : mode == kSemi ? K * std::min(0LL, g) : (N + M) * std::min(0LL, g);
    return lo - 100 * mag >= -30000 && hi + 100 * mag <= 30000 &&
           (mode != kLocal || flex_local_fits(n, m, ma, mi, gap));
}

// The semi-global packed fills (ta_dual.hip, ta_affine.hip) keep the column of row n's
// best in a 16-bit half beside the value.  The value bounds below cap m for most
// scorings, but with match == gap (affine: match == extend) the bias -ma*j + gap*(j - i)
// does not depend on j and they admit any m: the cap is stated on its own.
constexpr uint32_t kSemiColumnMax = 65535;

// Bounds of the biased 16-bit values of ta_dual.hip (S and every candidate),
// with a margin; pairs that do not fit run in the int32 kernel.
bool fits_int16(int mode, uint32_t n, uint32_t m, int ma, int mi, int gap) {
    if (n == 0 || m == 0) return false;
    if (mode == kSemi && m > kSemiColumnMax) return false;
    const long long N = n, M = m;
    const long long mag = std::max({1LL, std::llabs(ma), std::llabs(mi), std::llabs(gap)});
    const long long hmax = std::min(N, M) * std::max({0LL, (long long)ma, (long long)mi}) + (N + M) * std::max(0LL, (long long)gap);
    long long lo, hi;
    if (mode == kLocal) {
        const long long z = 1 - 16LL * ma;  // S = 16H + z*j - i
        hi = 16 * hmax + std::max(0LL, z) * M + 32 * mag;
        lo = std::min(0LL, z) * M - N - 32 * mag;
        if (16 * hmax + 15 > 32767) return false;  // the argmax key 16H + 15 - r
    } else {
        // S = H - ma*j + gap*(j - i) over the rows 0..n+15 (the last lane's padding
        // rows) and columns 0..m.  H >= gap*min(i, j) (semi: gap steps from a 0
        // boundary) or (i + j)*min(0, gap) (global), H <= hs*min(i, j) + (i + j)*gp.
        // Both bounds and the bias are linear on either side of i = j, so their
        // extremes lie on the vertices of the two triangles; the row-n values
        // H - gap*n that the semi-global kernel also keeps packed are covered too.
        const long long N1 = N + 16, g = gap, K = std::min(N1, M);
        const long long hs = std::max({0LL, (long long)ma, (long long)mi}), gp = std::max(0LL, g);
        const long long pts[5][2] = {{0, 0}, {N1, 0}, {0, M}, {N1, M}, {K, K}};
        lo = LLONG_MAX;
        hi = LLONG_MIN;
        for (const auto& pt : pts) {
            const long long i = pt[0], j = pt[1], mn = std::min(i, j);
            const long long hl = (mode == kGlobal) ? (i + j) * std::min(0LL, g) : std::min(0LL, g) * mn;
            const long long hh = hs * mn + (i + j) * gp;
            const long long b = -(long long)ma * j + g * (j - i);
            lo = std::min({lo, hl + b, hl - g * N1, hl - g * N});
            hi = std::max({hi, hh + b, hh - g * N1, hh - g * N});
        }
        lo -= 8 * mag;
        hi += 8 * mag;
    }
    return hi <= 32000 && lo >= -32000;
}

// Every packed value of aff_dual_pass within int16, with margins.  The kernel
// keeps S = V - ma*j + X*(j - i) for V = H, E, F.  Per cell (i, j), rows up to
// n + 15 (the last lane's padding rows):
//   H >= min(0, O + X*min(i, j))            semi (a gap run from a 0 boundary;
//        (O + X*max(i, j) when X > 0)         0 on the boundary itself)
//   H >= 2*min(0, O) + (i + j)*min(0, X)    global (down the column, then right)
//   H <= hs*min(i, j) + (i + j)*(max(0, O) + max(0, X))
// E and F lie within one gap step (|O| + |X|) of an H, the -inf stand-ins are
// H - K, candidates one more step.  The lower bounds are concave and the upper
// one linear on either side of i = j, so their extremes over the grid lie on
// the vertices of the two triangles; the semi row-n values H - X*n are
// covered too.
bool affine_fits_int16(int mode, uint32_t n, uint32_t m, int ma, int mi, int open, int ext) {
    if (mode == kLocal || n == 0 || m == 0) return false;
    if (mode == kSemi && m > kSemiColumnMax) return false;  // (row n's column is a 16-bit half)
    const long long N = n, N1 = N + 16, M = m, O = open, X = ext;
    const long long hs = std::max({0LL, (long long)ma, (long long)mi});
    const long long gp = std::max(0LL, O) + std::max(0LL, X);
    const long long k = std::llabs(O) + std::llabs(X) + 2;
    const long long marg = 2 * k + 2 * std::llabs(ma) + std::llabs(mi) + 8;
    const long long K = std::min(N1, M);
    const long long pts[5][2] = {{0, 0}, {N1, 0}, {0, M}, {N1, M}, {K, K}};
    long long lo = LLONG_MAX, hi = LLONG_MIN;
    for (const auto& pt : pts) {
        const long long i = pt[0], j = pt[1], mn = std::min(i, j), mx = std::max(i, j);
        const long long hl = (mode == kGlobal) ? 2 * std::min(0LL, O) + (i + j) * std::min(0LL, X)
                                               : std::min(0LL, O + X * (X <= 0 ? mn : mx));
        const long long hh = hs * mn + (i + j) * gp;
        const long long b = -(long long)ma * j + X * (j - i);
        lo = std::min({lo, hl + b, hl - X * N});
        hi = std::max({hi, hh + b, hh - X * N});
    }
    return lo - marg >= -32000 && hi + marg <= 32000;
}

namespace {

// Pairs by descending cells (fewer stragglers: the big ones start first),
// equal shapes adjacent so they can be coupled for the two-pair kernels.
std::vector<uint32_t> by_cells(uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen) {
    std::vector<uint32_t> o(n_pairs);
    std::iota(o.begin(), o.end(), 0u);
    bool uniform = true;
    for (uint32_t p = 1; p < n_pairs && uniform; ++p) uniform = qlen[p] == qlen[0] && tlen[p] == tlen[0];
    if (uniform) return o;  // already in order (stable)
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t ca = (uint64_t)qlen[a] * tlen[a], cb = (uint64_t)qlen[b] * tlen[b];
        if (ca != cb) return ca > cb;
        return qlen[a] != qlen[b] ? qlen[a] > qlen[b] : tlen[a] > tlen[b];
    });
    return o;
}

// What every family's plan starts from: the batch itself and the CIGAR slots.
void init_plan(PlanBase& pl, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen, int type, int match,
               int mismatch, bool want_cigar) {
    pl.n_pairs = n_pairs;
    pl.type = type;
    pl.match = match;
    pl.mismatch = mismatch;
    pl.want_cigar = want_cigar;
    pl.qlen.assign(qlen, qlen + n_pairs);
    pl.tlen.assign(tlen, tlen + n_pairs);
    pl.slot_off.resize(n_pairs);
    for (uint32_t p = 0; p < n_pairs; ++p) {
        pl.slot_off[p] = pl.slots_bytes;
        pl.slots_bytes += cigar_slot_bytes(qlen[p], tlen[p]);
    }
}

// Work units, what the chunk assembly cuts: one pair (int32 fill; every banded pair), an
// equal-shape couple (dual fill) or a couple of different shapes (flexible dual fill).
// b == a: a single pair, or a pair coupled with itself.
enum UnitKind : int { kSingle = 0, kDual = 1, kFlex = 2 };
struct Unit {
    int kind;
    uint32_t a, b;
    uint64_t cost;  // cells one wave sweeps (linear: the launch order)
};
inline bool two_pairs(const Unit& u) { return u.kind != kSingle && u.a != u.b; }

// A linear batch as the stages see it, with the rules that speak of one pair.
struct LinearBatch {
    uint32_t n_pairs;
    const uint32_t *qlen, *tlen;
    int type, match, mismatch, gap;
    bool want_cigar;
    uint32_t flags;
    bool flag(uint32_t f) const { return (flags & f) != 0; }
    uint64_t cells(uint32_t p) const { return (uint64_t)qlen[p] * tlen[p]; }
    bool dual() const { return !flag(kPlanInt32Only); }
    // (< 64 passes: the hand-off tags epoch * 64 + pass + 1 never wrap to 0, ta_dual.hip)
    bool dual_fits(uint32_t p) const { return n_passes(qlen[p]) < 64 && fits_int16(type, qlen[p], tlen[p], match, mismatch, gap); }
    // A pair left without a partner (an odd pair of equal shapes, a ragged pair no
    // neighbour couples with) runs coupled with itself in the dual kernel, like a
    // lone pair, rather than in the int32 fill: a drop-in batch of 3 x 1 kb went
    // 1.12 -> 0.78 ms with the packed fill and walk for all of its pairs
    // (profiles/bench/r05_batch_latency.txt).
    // (tiny pairs keep the int32 fill: alone, its one fused launch is the shortest --
    // unless checkpoints are forced, kPlanCk: the tests' way into the checkpoint walks)
    bool lone_dual(uint32_t p) const { return dual() && (cells(p) >= 4096 || flag(kPlanCk)) && dual_fits(p); }
    Unit alone(uint32_t p) const { return {lone_dual(p) ? kDual : kSingle, p, p, cells(p)}; }
};

// ---- Stage 1 (linear), the census: one pass over the pairs.  The size rules
// read nothing else of the batch.
struct Census {
    uint32_t n_pairs = 0;
    uint64_t cells = 0;    // sum of n * m
    uint64_t longest = 0;  // largest n + m
    uint64_t len_sum = 0;  // sum of n + m
    uint64_t mag = 1;      // largest |score| (at least 1)
    // Local mode keeps V = 32*score + row tag in int32; take the unscaled
    // ("wide") kernel when any local value could reach 2^25 in magnitude.
    bool wide(int type) const { return type == kLocal && longest * mag >= (1ull << 25); }
    // Checkpoints save the fill ~0.3 of its time but the recomputing walk is a
    // longer chain per pair than the band walk (one window per 16 rows): they pay
    // once the cells per unit of the longest path pass ~2.5e6 (1 kb pairs: from
    // ~5,000 pairs on; 8 to 4,096 measured slower, profiles/bench/r05_ck_batches.txt).
    bool ck_size(uint32_t flags) const { return (flags & kPlanCk) || cells >= 2500000ull * std::max<uint64_t>(longest, 1); }
    // short enough for the lane, two-pair and band walks (an average of 6,000 bases a pair)
    bool short_pairs() const { return len_sum <= 6000ull * std::max<uint32_t>(n_pairs, 1); }
    // 24-bit multiplies of the scores in the run walks
    bool scores_24bit() const { return mag < (1ull << 22); }
};

Census take_census(const LinearBatch& b) {
    Census cs;
    cs.n_pairs = b.n_pairs;
    for (uint32_t p = 0; p < b.n_pairs; ++p) {
        const uint64_t len = (uint64_t)b.qlen[p] + b.tlen[p];
        cs.cells += b.cells(p);
        cs.len_sum += len;
        cs.longest = std::max(cs.longest, len);
    }
    cs.mag = std::max<uint64_t>({1ull, (uint64_t)std::llabs(b.match), (uint64_t)std::llabs(b.mismatch),
                                 (uint64_t)std::llabs(b.gap)});
    return cs;
}

// The guard every blocked-layout decision shares: a CIGAR is wanted, the walks' multiplies
// hold the scores, and no flag asks for the [step][lane] codes or for a run walk.  On top of it:
//   ck_allowed (checkpoints)   not kPlanNoCk, and the batch is large (ck_size)
//   ck_wanted, flex_ck         ck_allowed; local walks need gap <= 0
//   edge_ck                    ck_allowed; global / semi, equal-shape couples only
//   local_blk                  blk_allowed; kPlanNoCk, or ck_size and gap <= 0
bool blk_allowed(const LinearBatch& b, const Census& cs) {
    return b.want_cigar && cs.scores_24bit() && !b.flag(kPlanNoBlk | kPlanWalk1 | kPlanWalk2);
}
bool ck_allowed(const LinearBatch& b, const Census& cs) {
    return blk_allowed(b, cs) && !b.flag(kPlanNoCk) && cs.ck_size(b.flags);
}
// a plan that may take checkpoints couples its leftover ragged pairs with themselves in
// the flexible fill (not the int32 fill, which only stores codes)
bool ck_wanted(const LinearBatch& b, const Census& cs) {
    return ck_allowed(b, cs) && (b.type != kLocal || b.gap <= 0);
}

// ---- Stage 2 (linear), the units: which fill every pair runs in.
// Flexible couples of the pairs that found no equal-shape partner: same pass
// count and n mod 16 (same rows in the last lane), neighbours by (n, m), at
// most 25 % of the wave's cells wasted.
void flexible_units(const LinearBatch& b, bool ck_want, const std::vector<uint32_t>& rest, std::vector<Unit>& units) {
    const uint32_t *qlen = b.qlen, *tlen = b.tlen;
    std::vector<uint32_t> cand;
    for (uint32_t p : rest) {
        if (qlen[p] && tlen[p] && (b.type != kLocal || flex_local_fits(qlen[p], tlen[p], b.match, b.mismatch, b.gap)) &&
            (!ck_want || flex_ck_fits(b.type, qlen[p], tlen[p], b.match, b.mismatch, b.gap)))
            cand.push_back(p);
        else
            units.push_back({kSingle, p, p, b.cells(p)});
    }
    auto key = [&](uint32_t p) { return ((uint64_t)n_passes(qlen[p]) << 4) | (qlen[p] & 15u); };
    std::stable_sort(cand.begin(), cand.end(), [&](uint32_t x, uint32_t y) {
        if (key(x) != key(y)) return key(x) < key(y);
        if (qlen[x] != qlen[y]) return qlen[x] > qlen[y];
        return tlen[x] > tlen[y];
    });
    for (size_t i = 0; i < cand.size();) {
        const uint32_t A = cand[i];
        if (i + 1 < cand.size() && key(cand[i + 1]) == key(A) && n_passes(qlen[A]) < 64) {
            const uint32_t B = cand[i + 1];
            const uint64_t wave = (uint64_t)qlen[A] * std::max(tlen[A], tlen[B]);
            const uint64_t useful = b.cells(A) + b.cells(B);
            if (4 * useful >= 3 * 2 * wave) {  // waste <= 25 %
                units.push_back({kFlex, A, B, wave});
                i += 2;
                continue;
            }
        }
        // a long pair without a partner is coupled with itself: one wave per pass;
        // a shorter one in the dual kernel when it fits int16 (lone_dual)
        const uint32_t ps = n_passes(qlen[A]);
        if ((ps >= 4 || (ck_want && !b.lone_dual(A))) && ps < 64)
            units.push_back({kFlex, A, A, b.cells(A)});
        else
            units.push_back(b.alone(A));
        ++i;
    }
}

// Equal-shape couples first, flexible couples of what they leave, the rest
// alone; then longest first.
std::vector<Unit> linear_units(const LinearBatch& b, bool ck_want) {
    const std::vector<uint32_t> order = by_cells(b.n_pairs, b.qlen, b.tlen);
    std::vector<Unit> units;
    units.reserve(b.n_pairs);
    std::vector<uint32_t> rest;
    for (uint32_t k = 0; k < b.n_pairs;) {
        const uint32_t p = order[k];
        // (equal shapes within int16 stay on the dual fill even when multi-pass: measured faster
        // than the pipelined flexible fill on config 5, 4,056 vs 3,765 GCUPS)
        const bool couple = b.dual() && k + 1 < b.n_pairs && b.qlen[order[k + 1]] == b.qlen[p] &&
                            b.tlen[order[k + 1]] == b.tlen[p] && b.dual_fits(p);
        // A lone pair (one-pair batches: the drop-in call) runs coupled with
        // itself in the packed kernel -- both halves compute it, its codes are
        // written once -- whose wave and lane walk finish sooner than one int32
        // wave walking inside the fill, except for tiny pairs where the one
        // fused launch wins.  (Not lone_dual: kPlanCk does not lower the size,
        // and the pair never reaches the flexible couples.)
        const bool self = b.dual() && b.n_pairs == 1 && b.cells(p) >= 4096 && b.dual_fits(p);
        if (couple || self) units.push_back({kDual, p, couple ? order[k + 1] : p, b.cells(p)});
        else rest.push_back(p);
        k += couple ? 2 : 1;
    }
    if (b.dual() && !b.flag(kPlanNoFlex) && flex_fits(b.type, b.match, b.mismatch, b.gap))
        flexible_units(b, ck_want, rest, units);
    else
        for (uint32_t p : rest) units.push_back(b.alone(p));
    std::stable_sort(units.begin(), units.end(), [](const Unit& x, const Unit& y) { return x.cost > y.cost; });
    return units;
}

// Affine units: couples of equal shape for the packed fill (global / semi,
// values within int16), else single pairs; by descending cells.
std::vector<Unit> affine_units(uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen, const AffinePlan& pl, uint32_t flags) {
    const std::vector<uint32_t> byc = by_cells(n_pairs, qlen, tlen);
    const bool dual_ok = !(flags & kPlanInt32Only);
    std::vector<Unit> units;
    units.reserve(n_pairs / 2 + 1);  // (all couples, config 5; singles grow it)
    for (uint32_t k = 0; k < n_pairs;) {
        const uint32_t x = byc[k];
        if (dual_ok && k + 1 < n_pairs && qlen[byc[k + 1]] == qlen[x] && tlen[byc[k + 1]] == tlen[x] &&
            n_passes(qlen[x]) < 64 &&  // hand-off tags epoch * 64 + pass + 1 never wrap (ta_affine.hip)
            affine_fits_int16(pl.type, qlen[x], tlen[x], pl.match, pl.mismatch, pl.open, pl.extend)) {
            units.push_back({kDual, x, byc[k + 1], 0});
            k += 2;
        } else {
            units.push_back({kSingle, x, x, 0});
            ++k;
        }
    }
    return units;
}

// ---- Stage 3 (linear): the code layout (pl.blk, pl.ck) and the walk (pl.walk_group).
void choose_layout(Plan& pl, const LinearBatch& b, const Census& cs, const std::vector<Unit>& units, bool ck_want) {
    bool all_dual = !units.empty(), all_packed = !units.empty(), any_flex = false;
    for (const Unit& u : units) {
        all_dual = all_dual && u.kind == kDual;
        all_packed = all_packed && u.kind != kSingle;
        any_flex = any_flex || u.kind == kFlex;
    }
    // Local walks of short pairs in plans of equal-shape couples only run as band
    // walks (one lane per pair, ta_walk_band.h) over the blocked code layout:
    // the dual fill stages each stripe's 16 steps and writes them as 64
    // contiguous bytes, the unit a walk following its stripe reads.
    // Local plans take the blocked layout only with checkpoints (ck_size, gap <= 0) or
    // under TA_PLAN_NO_CK (blocked codes and band walks): below the checkpoint size the
    // [step][lane] codes (whose fill reads its per-step operands from the LDS list) and
    // the lane walks finish sooner at every batch size measured, 8-4096 pairs of
    // 200-1000 bases (3-6 %, scripts/exp/batch_latency.py, profiles/bench/r06s_batch_latency.txt).
    // (Batches of fewer than 8 pairs keep the lane walks with any flag.)
    const bool local_blk = blk_allowed(b, cs) && b.type == kLocal && all_dual && cs.short_pairs() && b.n_pairs >= 8 &&
                           (b.flag(kPlanNoCk) || (cs.ck_size(b.flags) && b.gap <= 0));
    // Global / semi-global plans of equal-shape couples (config 5) take checkpoints
    // and recomputing walks by the same rule, whatever their lengths: their walks end
    // on row 0 / column 0 (ta_walk_ck.hip) and need no cost, so no gap-sign condition.
    const bool edge_ck = ck_allowed(b, cs) && b.type != kLocal && all_dual;
    // Plans with flexible couples (config 3: ragged reads) in any mode, when every unit
    // is packed and every flexible pair's H fits the checkpoints (flex_ck_fits; local
    // walks need gap <= 0, ck_want)
    bool flex_fit = true;
    for (const Unit& u : units)
        if (u.kind == kFlex)
            flex_fit = flex_fit && flex_ck_fits(b.type, b.qlen[u.a], b.tlen[u.a], b.match, b.mismatch, b.gap) &&
                       flex_ck_fits(b.type, b.qlen[u.b], b.tlen[u.b], b.match, b.mismatch, b.gap);
    const bool flex_ck = ck_want && any_flex && all_packed && flex_fit && !b.flag(kPlanNoFlexCk);
    pl.blk = local_blk || edge_ck || flex_ck;
    // Local walks of short pairs: lane walks (one lane per pair steps cell by cell
    // through LDS tiles, ta_walk_lane.h; indel costs kept as int8).  Two pairs per
    // wave (32 lanes each, ta_walk2.h): 0.65 vs 0.77 ms for one pair per wave on
    // config 2; their runs are clipped to 32 cells, so batches of long pairs (long
    // M runs) keep the one-pair walk (config 3 local: 4.1 vs 6.3 ms).  24-bit
    // multiplies of the scores in the run walks.
    // (local: a positive gap lowers the cost in gap runs -- the one-pair walk)
    if (pl.blk) pl.walk_group = (b.gap <= 0 || b.type != kLocal) ? 64 : 0;
    else if (b.flag(kPlanWalk1) || !cs.scores_24bit() || !cs.short_pairs()) pl.walk_group = 0;
    else if (b.flag(kPlanWalk2) || b.gap < -128 || b.gap > 127) pl.walk_group = 32;
    else pl.walk_group = 16;
    pl.ck = pl.blk && pl.walk_group == 64 && !b.flag(kPlanNoCk) && cs.ck_size(b.flags);
}

// ---- Stage 4 (all families): chunk assembly.
// Chunk boundaries over units in launch order: a chunk closes when the next
// unit's codes would exceed the budget.  A chunk closed by the budget is then
// trimmed to a whole number of "rounds" -- multiples of wave_quantum waves (one
// wave per SIMD) -- when it holds at least one: the fill is VALU-bound, so a
// chunk takes as long as its busiest SIMD, and 2,500 waves on 1,024 SIMDs
// (3 on some, 2 on others) run at 2.44 / 3 of the rate of 2,048 (config 5
// affine: 100k pairs in 20 chunks of 5,000 vs 25 of 4,096).
template <class Codes, class Waves>
std::vector<size_t> chunk_starts(size_t n_units, uint64_t budget, uint32_t wave_quantum, Codes codes, Waves waves) {
    std::vector<size_t> starts;
    size_t k = 0;
    while (k < n_units) {
        const size_t start = k;
        uint64_t used = 0, w = 0;
        while (k < n_units) {
            const uint64_t c = codes(k);
            if (k > start && used + c > budget) break;
            used += c;
            w += waves(k);
            ++k;
        }
        if (k < n_units && wave_quantum && w >= wave_quantum) {
            const uint64_t target = w / wave_quantum * wave_quantum;
            while (w > target && k > start + 1) {
                --k;
                w -= waves(k);
            }
        }
        starts.push_back(start);
    }
    return starts;
}

// One chunk as the assembly leaves it; each family keeps the members it has.
struct Cut {
    uint32_t begin = 0, count = 0;        // all pairs (plan order)
    uint32_t kbegin[3] = {}, kcount[3] = {};  // per unit kind: units
    uint32_t cbegin = 0;                  // couples (dual + flex) before this chunk
    uint64_t codes = 0, bnd = 0;          // code and boundary entries
    uint32_t dpasses = 0, spasses = 0;    // largest pass count of the dual couples / the pipelined singles
};
struct Assembly {
    std::vector<uint32_t> list[3];  // per unit kind: pair ids (singles 1, couples 2 each)
    std::vector<Cut> cuts;
    uint64_t ws_codes = 0, ws_bnd = 0;  // the largest chunk's
    bool piped = false;                 // some chunk runs multi-pass singles one wave per (pair, pass)
};

// Cuts units (in launch order) into chunks of at most `budget` code entries
// and lays every pair's codes and boundary region out inside its chunk:
// pl.order, pl.ptr_off, pl.bnd_off, and the rest in the Assembly.
// pair_codes(p): code entries of pair p; pair_bnd(u, h): boundary entries of
// half h of unit u -- the families' own sizes.  Packed fills and pipelined
// int32 pairs (pipe_singles) run one wave per (unit, pass), else one per pair.
template <class Codes, class Bnd>
Assembly assemble_chunks(PlanBase& pl, const std::vector<Unit>& units, uint64_t budget, uint32_t wave_quantum,
                         bool pipe_singles, Codes pair_codes, Bnd pair_bnd) {
    auto codes = [&](uint32_t p) -> uint64_t { return pl.want_cigar ? pair_codes(p) : 0; };
    auto passes = [&](const Unit& u) { return n_passes(pl.qlen[u.a]); };
    auto piped = [&](const Unit& u) { return (u.kind != kSingle || pipe_singles) && pl.qlen[u.a] && pl.tlen[u.a]; };
    const std::vector<size_t> starts = chunk_starts(
        units.size(), budget, wave_quantum,
        [&](size_t k) { return codes(units[k].a) + (two_pairs(units[k]) ? codes(units[k].b) : 0); },
        [&](size_t k) -> uint64_t { return piped(units[k]) ? passes(units[k]) : 1; });
    Assembly as;
    pl.order.reserve(pl.n_pairs);
    pl.ptr_off.assign(pl.n_pairs, 0);
    pl.bnd_off.assign(pl.n_pairs, 0);
    uint32_t couples = 0;
    for (size_t s = 0; s < starts.size(); ++s) {
        Cut c;
        c.begin = (uint32_t)pl.order.size();
        c.cbegin = couples;
        for (int kind = 0; kind < 3; ++kind) c.kbegin[kind] = (uint32_t)(as.list[kind].size() / (kind == kSingle ? 1 : 2));
        const size_t end = s + 1 < starts.size() ? starts[s + 1] : units.size();
        for (size_t k = starts[s]; k < end; ++k) {
            const Unit& u = units[k];
            const uint32_t ids[2] = {u.a, u.b};
            for (int h = 0; h < (two_pairs(u) ? 2 : 1); ++h) {
                pl.ptr_off[ids[h]] = c.codes;
                pl.bnd_off[ids[h]] = c.bnd;
                c.codes += codes(ids[h]);
                c.bnd += pair_bnd(u, h);
                pl.order.push_back(ids[h]);
                ++c.count;
            }
            as.list[u.kind].push_back(u.a);
            if (u.kind != kSingle) as.list[u.kind].push_back(u.b);
            ++c.kcount[u.kind];
            if (u.kind == kDual) c.dpasses = std::max(c.dpasses, passes(u));
            if (u.kind == kSingle && piped(u)) c.spasses = std::max(c.spasses, passes(u));
            if (u.kind != kSingle) ++couples;
        }
        as.ws_codes = std::max(as.ws_codes, c.codes);
        as.ws_bnd = std::max(as.ws_bnd, c.bnd);
        as.piped |= c.spasses > 1;
        as.cuts.push_back(c);
    }
    return as;
}

// ---- Stage 5: ticketing.
// Ticket order of one chunk's pass tasks (units first .. first+count-1, unit
// w with off[w+1] - off[w] passes).  A task's predecessor (the same unit's
// pass - 1) must hold an earlier ticket: its wave is then running, so every
// poll ends.  Pass-major (start-aligned): every unit's pass 0, then every
// pass 1, ...; the longest units' last passes get the last tickets and run
// alone at the end of the launch.  End-aligned (default): level L = pass -
// passes, ascending, so every unit's last pass is in the last level and the
// long chains start first.  Within a level: plan order (most cells first).
template <class Emit>
void order_pass_tasks(const std::vector<uint32_t>& off, uint32_t first, uint32_t count, bool end_aligned, Emit emit) {
    uint32_t maxp = 0;
    for (uint32_t w = first; w < first + count; ++w) maxp = std::max(maxp, off[w + 1] - off[w]);
    for (uint32_t lv = 0; lv < maxp; ++lv)
        for (uint32_t w = first; w < first + count; ++w) {
            const uint32_t P = off[w + 1] - off[w];
            if (end_aligned) {
                if (lv + P >= maxp) emit(w, lv + P - maxp);
            } else if (lv < P) {
                emit(w, lv);
            }
        }
}

// The flexible fill's tasks, one per (couple, pass): couple * 64 + pass.
void ticket_flexes(Plan& pl, const std::vector<Cut>& cuts) {
    pl.flex_task_off.assign(1, 0);
    for (size_t w = 0; w < pl.flexes.size() / 2; ++w)
        pl.flex_task_off.push_back(pl.flex_task_off.back() + n_passes(pl.qlen[pl.flexes[2 * w]]));
    pl.flex_tasks.assign(pl.flex_task_off.back(), 0u);
    for (const Cut& c : cuts) {
        uint32_t at = pl.flex_task_off[c.kbegin[kFlex]];
        order_pass_tasks(pl.flex_task_off, c.kbegin[kFlex], c.kcount[kFlex], pl.end_aligned,
                         [&](uint32_t w, uint32_t ps) { pl.flex_tasks[at++] = w * 64u + ps; });
    }
}

// The pipelined int32 fill's tasks (linear and affine), one per (single, pass)
// of the chunks whose singles are multi-pass: single << 32 | pass.
template <class P>
void ticket_singles(P& pl, const std::vector<Cut>& cuts) {
    pl.single_task_off.assign(1, 0);
    for (uint32_t p : pl.singles)
        pl.single_task_off.push_back(pl.single_task_off.back() + (pl.qlen[p] && pl.tlen[p] ? n_passes(pl.qlen[p]) : 0));
    pl.single_tasks.assign(pl.single_task_off.back(), 0ull);
    for (const Cut& c : cuts) {
        if (c.spasses < 2) continue;  // single-pass singles: the one-wave-per-pair fill
        uint32_t at = pl.single_task_off[c.kbegin[kSingle]];
        order_pass_tasks(pl.single_task_off, c.kbegin[kSingle], c.kcount[kSingle], pl.end_aligned,
                         [&](uint32_t w, uint32_t ps) { pl.single_tasks[at++] = ((uint64_t)w << 32) | ps; });
    }
}

}  // namespace

void build_plan(Plan& pl, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen, int type, int match,
                int mismatch, int gap, bool want_cigar, uint64_t budget, uint32_t flags, uint32_t wave_quantum) {
    pl = Plan{};
    init_plan(pl, n_pairs, qlen, tlen, type, match, mismatch, want_cigar);
    pl.gap = gap;
    pl.end_aligned = !(flags & kPlanPassMajor);
    const LinearBatch b{n_pairs, qlen, tlen, type, match, mismatch, gap, want_cigar, flags};
    const Census cs = take_census(b);
    const bool ck_want = ck_wanted(b, cs);
    const std::vector<Unit> units = linear_units(b, ck_want);
    choose_layout(pl, b, cs, units, ck_want);
    pl.wide = cs.wide(type);
    // Multi-pass int32 pairs run one wave per (pair, pass) like the packed
    // fills (their passes overlap instead of following each other on one
    // wave); the walk then runs in the traceback kernel.
    const bool pipe_singles = !(flags & kPlanSerialPasses);
    Assembly as = assemble_chunks(
        pl, units, std::max<uint64_t>(budget / 4, 1), wave_quantum, pipe_singles,
        [&](uint32_t p) { return ptr_dwords_any(qlen[p], tlen[p], pl.blk); },
        [&](const Unit& u, int h) {
            const uint32_t x = h ? u.b : u.a;
            const bool records = h == 0 && n_passes(qlen[u.a]) > 1;  // pair A of a multi-pass unit
            uint64_t bw = bnd_words(qlen[x], tlen[x]);
            // flex: pair A holds both pairs' absolute int32 boundary rows, interleaved;
            // each pair keeps a region of its own for the int32 fallback ('-' in a query)
            if (u.kind == kFlex && records) bw = std::max<uint64_t>(bw, 8ull * ((uint64_t)std::max(tlen[u.a], tlen[u.b]) + 1));
            // dual: pair A holds the couple's packed hand-off records, 2 buffers x 8 bytes per column;
            // pipelined int32 fill: the pair's hand-off records, 2 buffers x 8 bytes per column
            if ((u.kind == kDual || (u.kind == kSingle && pipe_singles)) && records)
                bw = std::max<uint64_t>(bw, 4ull * ((uint64_t)tlen[u.a] + 1));
            return bw + (bw & 1);  // keep every region 8-byte aligned (64-bit hand-off records)
        });
    pl.singles = std::move(as.list[kSingle]);
    pl.duals = std::move(as.list[kDual]);
    pl.flexes = std::move(as.list[kFlex]);
    for (const Cut& c : as.cuts)
        pl.chunks.push_back({{c.begin, c.count}, c.kbegin[kSingle], c.kcount[kSingle], c.kbegin[kDual], c.kcount[kDual],
                             c.kbegin[kFlex], c.kcount[kFlex], c.cbegin, c.codes, c.bnd, c.dpasses, c.spasses});
    pl.n_dual_pairs = (uint32_t)(pl.duals.size() + pl.flexes.size());
    pl.ws_ptr_dwords = as.ws_codes;
    pl.ws_bnd_words = as.ws_bnd;
    // A fill kernel that walks its own pair only pays when nothing else of the
    // chunk runs in the separate traceback kernel anyway.
    // (Each dual wave walking its own two pairs right after its fill measured
    // slower: config 2 3.10 ms vs 2.19 + 0.65; the walk inherits the fill's
    // register allocation and all waves finish their fills together anyway.)
    pl.fused = want_cigar && pl.n_dual_pairs == 0 && !(flags & kPlanUnfused) && !as.piped;
    ticket_flexes(pl, as.cuts);
    if (as.piped) ticket_singles(pl, as.cuts);
}

void build_affine_plan(AffinePlan& pl, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen, int type,
                       int match, int mismatch, int gap_open, int gap_extend, bool want_cigar, uint64_t budget,
                       uint32_t flags, uint32_t wave_quantum) {
    pl = AffinePlan{};
    init_plan(pl, n_pairs, qlen, tlen, type, match, mismatch, want_cigar);
    pl.open = gap_open;
    pl.extend = gap_extend;
    pl.end_aligned = !(flags & kPlanPassMajor);
    const std::vector<Unit> units = affine_units(n_pairs, qlen, tlen, pl, flags);
    // the packed fill runs one wave per (couple, pass); the int32 fill one per
    // pair, or one per (pair, pass) when pipelined
    const bool pipe_singles = !(flags & kPlanSerialPasses);
    Assembly as = assemble_chunks(
        pl, units, std::max<uint64_t>(budget / 8, 1), wave_quantum, pipe_singles,
        [&](uint32_t p) { return ptr_dwords(qlen[p], tlen[p]); },
        [&](const Unit& u, int h) {
            const uint32_t p = h ? u.b : u.a;
            // a multi-pass couple's pair A holds the pass hand-off records: 2 buffers x
            // (H, F) x 8 bytes per column = 4 int2 entries; pair B keeps its own
            // boundary row for the int32 fallback ('-' in a query)
            // a pipelined single: its own records, the same 4 entries per column
            const bool records = (u.kind == kDual ? h == 0 : pipe_singles) && n_passes(qlen[p]) > 1;
            const uint64_t bw = bnd_words(qlen[p], tlen[p]);
            return records ? std::max<uint64_t>(bw, 4ull * ((uint64_t)tlen[p] + 1)) : bw;  // (no padding: 8-byte entries)
        });
    pl.singles = std::move(as.list[kSingle]);
    pl.duals = std::move(as.list[kDual]);
    for (const Cut& c : as.cuts)
        pl.chunks.push_back({{c.begin, c.count}, c.kbegin[kSingle], c.kcount[kSingle], c.kbegin[kDual], c.kcount[kDual],
                             c.codes, c.bnd, c.dpasses, c.spasses});
    pl.ws_ptr_entries = as.ws_codes;
    pl.ws_bnd_entries = as.ws_bnd;
    if (as.piped) ticket_singles(pl, as.cuts);
}

// The degenerate case of the assembly: single pairs by descending swept cells,
// no wave quantum, no hand-off records.  Both banded families: the entry
// counts are the same (band_ptr_dwords code entries, bnd_words boundary
// entries); the families differ in the size of an entry.
namespace {

template <class P>
Assembly assemble_band(P& pl, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen, const uint32_t* band,
                       uint64_t budget_entries) {
    pl.band.resize(n_pairs);
    std::vector<Unit> units(n_pairs);
    for (uint32_t p = 0; p < n_pairs; ++p) {
        pl.band[p] = band_clamp(qlen[p], tlen[p], band[p]);
        units[p] = {kSingle, p, p, band_swept_cells(qlen[p], tlen[p], pl.band[p])};
        pl.swept_cells += units[p].cost;
        pl.band_cells += band_cells(qlen[p], tlen[p], pl.band[p]);
    }
    std::stable_sort(units.begin(), units.end(), [](const Unit& x, const Unit& y) { return x.cost > y.cost; });
    return assemble_chunks(
        pl, units, std::max<uint64_t>(budget_entries, 1), 0, false,
        [&](uint32_t p) { return band_ptr_dwords(qlen[p], tlen[p], pl.band[p]); },
        [&](const Unit& u, int) { return bnd_words(qlen[u.a], tlen[u.a]); });
}

}  // namespace

void build_band_plan(BandPlan& pl, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen, const uint32_t* band,
                     int type, int match, int mismatch, int gap, bool want_cigar, uint64_t budget, int32_t zdrop,
                     int zdrop_rule) {
    pl = BandPlan{};
    init_plan(pl, n_pairs, qlen, tlen, type, match, mismatch, want_cigar);
    pl.gap = gap;
    pl.zdrop = (type == kAnchored && zdrop >= 0) ? zdrop : -1;
    pl.zdrop_rule = (pl.zdrop >= 0 && zdrop_rule == kZdropStripe) ? kZdropStripe : kZdropSegment;
    const Assembly as = assemble_band(pl, n_pairs, qlen, tlen, band, budget / 4);
    for (const Cut& c : as.cuts) pl.chunks.push_back({{c.begin, c.count}, c.codes, c.bnd});
    pl.ws_ptr_dwords = as.ws_codes;
    pl.ws_bnd_words = as.ws_bnd;
}

void build_band_affine_plan(BandAffinePlan& pl, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen,
                            const uint32_t* band, int type, int match, int mismatch, int gap_open, int gap_extend,
                            bool want_cigar, uint64_t budget, int32_t zdrop, int zdrop_rule) {
    pl = BandAffinePlan{};
    init_plan(pl, n_pairs, qlen, tlen, type, match, mismatch, want_cigar);
    pl.open = gap_open;
    pl.extend = gap_extend;
    pl.zdrop = (type == kAnchored && zdrop >= 0) ? zdrop : -1;
    pl.zdrop_rule = (pl.zdrop >= 0 && zdrop_rule == kZdropStripe) ? kZdropStripe : kZdropSegment;
    const Assembly as = assemble_band(pl, n_pairs, qlen, tlen, band, budget / 8);
    for (const Cut& c : as.cuts) pl.chunks.push_back({{c.begin, c.count}, c.codes, c.bnd});
    pl.ws_ptr_entries = as.ws_codes;
    pl.ws_bnd_entries = as.ws_bnd;
}

uint64_t host_batch_code_bytes(uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen, uint64_t bytes_per_entry) {
    uint64_t need = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) need += ptr_dwords_blk(qlen[p], tlen[p]) * bytes_per_entry;
    return need;
}

}  // namespace ta
