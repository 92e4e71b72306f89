// bioinfo1_amd/csrc/ta_layout.h -- geometry of the fill and of the HBM
// workspace, shared by the kernels (hipcc) and the host planner
// (ta_planner.cpp, which also builds with plain g++ for the CPU sanitizer
// tests).  No HIP runtime types here.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define TA_HD __host__ __device__
#else
#define TA_HD
#endif

namespace ta {

// One wave64 per pair; lane l owns kRows consecutive query rows; a "pass" is
// the 64*kRows = 1024 rows one wave covers at once.
constexpr int kRows = 16;
constexpr int kWave = 64;
constexpr int kPassRows = kRows * kWave;
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWave * kWavesPerBlock;

// kAnchored (the ta_anchored_* family only; never a caller's AlignmentType):
// global boundaries and recurrence, the goal at the best in-band interior cell.
enum Mode : int { kGlobal = 0, kLocal = 1, kSemi = 2, kAnchored = 3 };

// Local dual fill (ta_dual.hip) with three-input maxima: its biased values
// S = 16H + z*j - i and every candidate, shifted by the returned offset, lie in
// [0, 0x7BFF] -- non-negative int16 whose bit patterns, read as f16, are
// finite and ordered like the integers, so v_pk_maximum3_f16 takes their max.
// Two frames (local_max3_z): z = 1 - 16*ma, where a match's diagonal gain is 0
// (the fills that store codes), and the equal-gain frame z = -1 (eq: the
// checkpoint and score-only fills), where the up and left gains are both
// 16*gap - 1 -- one gain add on the larger of the two -- and the diagonal gain
// 16*s - 2 comes from a byte table (local_eq_gains: s in [-7, 8]).
// Bounds: a local path into (i, j) has at most min(i, j) diagonal steps and
// i + j gap steps, so
//   H <= hs*j + gp*(i + j)   (hs = max(0, ma, mi), gp = max(0, gap))
//   S <= (16hs + 16gp + z)*j + (16gp - 1)*i,   S >= z*j - i (the clamp),
// rows up to n + 15 (the last lane's padding rows), candidates one step
// (<= 16*mag) below the clamp; lane l holds S + (z + 16)*l (its frame, so
// that the clamp bases of a step are the same in every lane), l < 64.
// -1: does not fit (the max/max kernel runs).
TA_HD inline bool local_eq_gains(int ma, int mi) {
    return ma >= -7 && ma <= 8 && mi >= -7 && mi <= 8;  // 16 s - 2 + 128 in [0, 255]
}
TA_HD inline int local_max3_z(int ma, bool eq) { return eq ? -1 : 1 - 16 * ma; }
TA_HD inline int local_max3_offset(uint32_t n, uint32_t m, int ma, int mi, int gap, bool eq = false) {
    if (eq && !local_eq_gains(ma, mi)) return -1;
    const long long N = (long long)n + 16, M = m;
    const long long ama = ma < 0 ? -ma : ma, ami = mi < 0 ? -mi : mi, ag = gap < 0 ? -gap : gap;
    const long long mag = ama > ami ? (ama > ag ? ama : ag) : (ami > ag ? ami : ag);
    const long long hs = ma > mi ? (ma > 0 ? ma : 0) : (mi > 0 ? mi : 0);
    const long long gp = gap > 0 ? gap : 0;
    const long long z = local_max3_z(ma, eq);
    const long long cj = 16 * hs + 16 * gp + z, ci = 16 * gp - 1;
    const long long fl = 63 * (z + 16);  // lane frame
    const long long hi = (cj > 0 ? cj * M : 0) + (ci > 0 ? ci * N : 0) + 32 * (mag + 1) + (fl > 0 ? fl : 0);
    const long long lo = (z < 0 ? z * M : 0) - N - 32 * (mag + 1) + (fl < 0 ? fl : 0);
    if (hi - lo > 0x7BFF) return -1;
    return (int)(-lo);
}

// Local flexible fill (ta_flex.hip): the value of a cell is
//   V = H - ma*j + gap*(j - i) - O + (17*gap - ma)*lane,
// so that the up candidate is the value above itself and the clamp base of a
// step (H = 0) is the same in every lane: zu - gap*r for row r of a stripe.
// Every 64 steps the wave is rebased so that zu = flex_local_c0; between
// rebases zu moves by (gap - ma) per step.  Values and candidates then lie in
// [c0 - 64*max(0, ma - gap) - 15*max(0, gap) - 16*mag, c0 + 64*max(0, gap - ma)
// + 15*max(0, -gap) + hmax + 16*mag]; c0 puts the low end at >= 64.
TA_HD inline int flex_local_c0(int ma, int mi, int gap) {
    const int ama = ma < 0 ? -ma : ma, ami = mi < 0 ? -mi : mi, ag = gap < 0 ? -gap : gap;
    const int mx = ama > ami ? (ama > ag ? ama : ag) : (ami > ag ? ami : ag), mag = mx < 1 ? 1 : mx;
    return 64 * (ma > gap ? ma - gap : 0) + 15 * (gap > 0 ? gap : 0) + 16 * mag + 64;
}

// Steps of one pass over an m-column target: m + 63 (lane skew).
TA_HD inline uint32_t pass_steps(uint32_t m) { return m + kWave - 1; }
TA_HD inline uint32_t n_passes(uint32_t n) { return (n + kPassRows - 1) / kPassRows; }
// Pointer-matrix dwords for an n x m pair: passes x steps x 64 lanes.
TA_HD inline uint64_t ptr_dwords(uint32_t n, uint32_t m) {
    return (n == 0 || m == 0) ? 0 : (uint64_t)n_passes(n) * pass_steps(m) * kWave;
}
// Blocked code layout (plans with `blk`): per pass, blocks of 16
// steps, [block][lane][16 steps] dwords -- the 16 consecutive steps of one
// stripe (a 16 x 16 square of cells) are 64 contiguous bytes, the unit a walk
// that follows a stripe reads, instead of 16 dwords 256 bytes apart in the
// [step][lane] layout.
constexpr int kBlkSteps = 16;
TA_HD inline uint32_t blk_count(uint32_t m) { return (pass_steps(m) + kBlkSteps - 1) / kBlkSteps; }
TA_HD inline uint64_t ptr_dwords_blk(uint32_t n, uint32_t m) {
    return (n == 0 || m == 0) ? 0 : (uint64_t)n_passes(n) * blk_count(m) * kBlkSteps * kWave;
}
TA_HD inline uint64_t ptr_dwords_any(uint32_t n, uint32_t m, bool blk) {
    return blk ? ptr_dwords_blk(n, m) : ptr_dwords(n, m);
}
// dword of (pass, step t, lane) in the blocked layout (nb = blk_count(m))
TA_HD inline uint64_t blk_index(uint32_t pass, uint32_t t, uint32_t lane, uint32_t nb) {
    return (((uint64_t)pass * nb + (t >> 4)) * kWave + lane) * kBlkSteps + (t & 15u);
}
// Checkpoint layout (ck plans): instead of codes, the local dual
// fill leaves in a pair's blocked region (nb * 2048 int16 per pass) the packed
// values a recomputing walk restarts from --
//   rows: [block][lane][16 steps]  the stripe's bottom row after each step
//   cols: [block][lane][16 rows]   the stripe's 16 rows after the block's last step
// (lane l: column t - l + 1 at step t, so block b's column is 16 (b + 1) - l).
// Both are int16 indexes into the pair's region.
TA_HD inline uint64_t ck_row_index(uint32_t pass, uint32_t t, uint32_t lane, uint32_t nb) {
    return ((uint64_t)pass * nb * 2 * kWave + (uint64_t)(t >> 4) * kWave + lane) * kBlkSteps + (t & 15u);
}
TA_HD inline uint64_t ck_col_index(uint32_t pass, uint32_t b, uint32_t lane, uint32_t nb, uint32_t r) {
    return (((uint64_t)pass * 2 + 1) * nb * kWave + (uint64_t)b * kWave + lane) * kBlkSteps + r;
}
// H of the cell (i, j) (1-based) from the packed value s the local dual fill
// held for it in lane l of its pass: s = off + 16 H + z j - i + dl l, with
// off = local_max3_offset(.., eq = true), z = -1 and dl = z + 16 = 15 in the
// checkpoint fill's three-input-max frame (off >= 0; ta_dual.hip M3 / UZ / EQ),
// off = dl = 0 and z = 1 - 16 ma otherwise.
TA_HD inline int ck_decode(int s, int off, int zstep, int dl, int i, int j, int l) {
    return (s - off - zstep * j + i - dl * l) >> 4;
}
// Pass-boundary row (int32 per column) needed only when the query spans > 1 pass.
TA_HD inline uint64_t bnd_words(uint32_t n, uint32_t m) {
    return n_passes(n) > 1 ? (uint64_t)m + 1 + kWave : 0;
}
// ---- Banded extension (ta_banded.hip; the definition is in
// include/team_align_c.h).  Cell (i, j) is in band iff lo <= j - i <= hi with
// lo = min(0, m - n) - w and hi = max(0, m - n) + w; a band of w >= max(n, m)
// holds every cell, so w is clamped there and every figure fits an int32.
TA_HD inline uint32_t band_clamp(uint32_t n, uint32_t m, uint32_t w) {
    const uint32_t full = n > m ? n : m;
    return w < full ? w : full;
}
TA_HD inline int band_lo(uint32_t n, uint32_t m, uint32_t w) {
    const int d = (int)m - (int)n;
    return (d < 0 ? d : 0) - (int)band_clamp(n, m, w);
}
TA_HD inline int band_hi(uint32_t n, uint32_t m, uint32_t w) {
    const int d = (int)m - (int)n;
    return (d > 0 ? d : 0) + (int)band_clamp(n, m, w);
}
// Pass p (rows 1024 p + 1 ..) sweeps the columns c0 .. c1 that hold an in-band
// cell of one of its rows; c0 <= c1 always, because every row has one.
TA_HD inline uint32_t band_c0(uint32_t n, uint32_t m, uint32_t w, uint32_t pass) {
    const int c = (int)(pass * kPassRows) + 1 + band_lo(n, m, w);
    return c > 1 ? (uint32_t)c : 1u;
}
TA_HD inline uint32_t band_c1(uint32_t n, uint32_t m, uint32_t w, uint32_t pass) {
    const uint32_t row_base = pass * kPassRows;
    const uint32_t nrows = n - row_base < (uint32_t)kPassRows ? n - row_base : (uint32_t)kPassRows;
    const uint32_t c = row_base + nrows + (uint32_t)band_hi(n, m, w);
    return c < m ? c : m;
}
// Steps whose codes pass p stores: its columns plus the lane skew.
TA_HD inline uint32_t band_pass_steps(uint32_t n, uint32_t m, uint32_t w, uint32_t pass) {
    return band_c1(n, m, w, pass) - band_c0(n, m, w, pass) + 1 + (kWave - 1);
}
// First code dword of pass p in the pair's region ([step][lane] within a pass).
TA_HD inline uint64_t band_pass_offset(uint32_t n, uint32_t m, uint32_t w, uint32_t pass) {
    uint64_t steps = 0;
    for (uint32_t p = 0; p < pass; ++p) steps += band_pass_steps(n, m, w, p);
    return steps * kWave;
}
TA_HD inline uint64_t band_ptr_dwords(uint32_t n, uint32_t m, uint32_t w) {
    return (n == 0 || m == 0) ? 0 : band_pass_offset(n, m, w, n_passes(n));
}
// ---- Z-drop on anchored alignment (the rule is DEFINED in include/team_align_c.h
// and restated in tests/anchored_zdrop_ref.py).  The drop is tied to the fill's
// sweep order: pass p executes band_drop_steps steps (its columns plus the skew
// of the stripes in use -- not the 63 of the code layout), the in-band interior
// cell (i, j) is computed at step band_drop_tau of its pass, and the rule is
// applied once per segment of kDropSteps steps.
constexpr int kDropSteps = 64;
TA_HD inline uint32_t band_drop_steps(uint32_t n, uint32_t m, uint32_t w, uint32_t pass) {
    const uint32_t row_base = pass * kPassRows;
    const uint32_t nrows = n - row_base < (uint32_t)kPassRows ? n - row_base : (uint32_t)kPassRows;
    const uint32_t nl = (nrows + kRows - 1) / kRows;
    return band_c1(n, m, w, pass) - band_c0(n, m, w, pass) + 1 + nl - 1;
}
TA_HD inline uint32_t band_drop_segments(uint32_t n, uint32_t m, uint32_t w, uint32_t pass) {
    return (band_drop_steps(n, m, w, pass) + kDropSteps - 1) / kDropSteps;
}
// 1 <= i <= n, 1 <= j <= m, (i, j) in band
TA_HD inline uint32_t band_drop_tau(uint32_t n, uint32_t m, uint32_t w, uint32_t i, uint32_t j) {
    return j - band_c0(n, m, w, (i - 1) / kPassRows) + ((i - 1) % kPassRows) / kRows;
}
// Steps a pair executes when it drops in segment s of pass p; p == n_passes(n): when nothing drops.
TA_HD inline uint64_t band_drop_swept_steps(uint32_t n, uint32_t m, uint32_t w, uint32_t pass, uint32_t seg) {
    if (n == 0 || m == 0) return 0;
    uint64_t steps = 0;
    for (uint32_t p = 0; p < pass; ++p) steps += band_drop_steps(n, m, w, p);
    if (pass < n_passes(n)) {
        const uint32_t sp = band_drop_steps(n, m, w, pass), cut = (uint32_t)kDropSteps * (seg + 1);
        steps += cut < sp ? cut : sp;
    }
    return steps;
}
// ---- The row-stripe z-drop rule (TA_ZDROP_STRIPE; DEFINED in include/team_align_c.h
// and restated in tests/anchored_zdrop_stripe_ref.py).  A stripe is the 16 rows one lane
// of the fill owns: stripe g is rows 16 g + 1 .. min(16 g + 16, n), lane g % 64 of pass
// g / 64.  The rule is tied to rows; only the step count follows the sweep: the fill
// tests the rule after every kDropSteps-th step of a pass and after its last step, on
// the stripes whose last cell has been computed by then.
constexpr int kZdropSegment = 0, kZdropStripe = 1;  // TA_ZDROP_SEGMENT / TA_ZDROP_STRIPE
TA_HD inline uint32_t band_stripes(uint32_t n) { return (n + kRows - 1) / kRows; }
// The step of its pass at which stripe g's last cell (row i_last, column min(m, i_last + hi))
// is computed; it strictly increases with the lane, and is below band_drop_steps.
TA_HD inline uint32_t band_stripe_tau_done(uint32_t n, uint32_t m, uint32_t w, uint32_t g) {
    const uint32_t i_last = n < kRows * g + kRows ? n : kRows * g + kRows;
    const uint32_t jl = i_last + (uint32_t)band_hi(n, m, w);
    return (jl < m ? jl : m) - band_c0(n, m, w, g / kWave) + g % kWave;
}
// Steps a pair executes when it drops at stripe g; g == band_stripes(n): when nothing drops.
TA_HD inline uint64_t band_stripe_swept_steps(uint32_t n, uint32_t m, uint32_t w, uint32_t g) {
    if (n == 0 || m == 0) return 0;
    if (g >= band_stripes(n)) return band_drop_swept_steps(n, m, w, n_passes(n), 0);
    return band_drop_swept_steps(n, m, w, g / kWave, band_stripe_tau_done(n, m, w, g) / kDropSteps);
}

// In-band interior cells (1 <= i <= n, 1 <= j <= m) and the cells the passes sweep.
TA_HD inline uint64_t band_cells(uint32_t n, uint32_t m, uint32_t w) {
    if (n == 0 || m == 0) return 0;
    const long long lo = band_lo(n, m, w), hi = band_hi(n, m, w);
    const long long N = n, M = m;
    // row i holds columns max(1, i + lo) .. min(m, i + hi): sum both ends over i = 1 .. n
    long long k1 = M - hi;  // rows i <= k1 end at i + hi, the others at m
    k1 = k1 < 0 ? 0 : (k1 > N ? N : k1);
    const long long ends = k1 * (k1 + 1) / 2 + k1 * hi + (N - k1) * M;
    long long k2 = -lo;  // rows i <= k2 begin at column 1, the others at i + lo
    k2 = k2 > N ? N : k2;
    const long long begins = k2 + (N * (N + 1) / 2 - k2 * (k2 + 1) / 2) + (N - k2) * lo;
    return (uint64_t)(ends - begins + N);
}
TA_HD inline uint64_t band_swept_cells(uint32_t n, uint32_t m, uint32_t w) {
    if (n == 0 || m == 0) return 0;
    uint64_t cells = 0;
    for (uint32_t p = 0; p < n_passes(n); ++p) {
        const uint32_t nrows = n - p * kPassRows < (uint32_t)kPassRows ? n - p * kPassRows : (uint32_t)kPassRows;
        cells += (uint64_t)(band_c1(n, m, w, p) - band_c0(n, m, w, p) + 1) * nrows;
    }
    return cells;
}

// ---- Exact banded alignment (ta_band_exact.hip; the rule is DEFINED in
// include/team_align_c.h and restated in tests/band_exact_ref.py).  w is the
// pair's clamped band.  Linear callers pass gap_open = 0, gap_extend = gap.
// Arithmetic: inside the families' range rule ((n + m + 2) * max step < 2^26)
// hs * k < 2^26, |gap_extend| * (|m - n| + 2 (w + 1)) <= |gap_extend| * (n + m)
// < 2^26 and 2 |gap_open| < 2^27, so |U| < 2^28 and int32 would suffice; the
// terms are formed in int64 all the same, which costs one lane a few
// instructions and holds for any int arguments.
TA_HD inline uint32_t band_exact_min(uint32_t n, uint32_t m) { return n < m ? n : m; }
// Every cell in band: w >= min(n, m), or a degenerate pair.
TA_HD inline bool band_exact_full(uint32_t n, uint32_t m, uint32_t w) {
    return n == 0 || m == 0 || w >= band_exact_min(n, m);
}
// Nothing short of the full band is certified when a gap step can gain.
TA_HD inline bool band_exact_certifiable(int gap_open, int gap_extend) { return gap_open <= 0 && gap_extend <= 0; }
// U(w): no path that touches a diagonal outside the band scores above it.  w < min(n, m).
TA_HD inline long long band_exact_bound(int type, uint32_t n, uint32_t m, uint32_t w, int match, int mismatch,
                                        int gap_open, int gap_extend, uint64_t dashes) {
    const long long hs = match > mismatch ? match : mismatch;
    const long long k = (long long)band_exact_min(n, m) - (long long)w - 1;  // diagonal steps at the most
    long long u = (hs > 0 ? hs : 0) * k;
    if (type == kGlobal) {
        const long long d = (long long)m - (long long)n;
        const long long steps = (d < 0 ? -d : d) + 2 * ((long long)w + 1);  // gap steps at the least
        const long long paid = steps - (long long)dashes;                  // at most `dashes` of them are free
        u += (long long)gap_extend * (paid > 0 ? paid : 0);
        if (dashes == 0) u += 2 * (long long)gap_open;  // one I run and one D run at the least
    }
    return u;
}
// The pair run at w scored s: is that the unbanded result?
TA_HD inline bool band_exact_certified(int type, uint32_t n, uint32_t m, uint32_t w, int match, int mismatch,
                                       int gap_open, int gap_extend, uint64_t dashes, long long s) {
    if (band_exact_full(n, m, w)) return true;
    if (!band_exact_certifiable(gap_open, gap_extend)) return false;
    return s > band_exact_bound(type, n, m, w, match, mismatch, gap_open, gap_extend, dashes);
}
// needed(w, s): the smallest w' > w with U(w') < s, else min(n, m) (the full
// band).  U does not increase with w, so a binary search finds it.  w < min(n, m).
TA_HD inline uint32_t band_exact_needed(int type, uint32_t n, uint32_t m, uint32_t w, int match, int mismatch,
                                        int gap_open, int gap_extend, uint64_t dashes, long long s) {
    const uint32_t full = band_exact_min(n, m);
    if (!band_exact_certifiable(gap_open, gap_extend)) return full;
    uint32_t lo = w + 1, hi = full;  // the answer is in [lo, hi]; U(hi) is not asked for
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (band_exact_bound(type, n, m, mid, match, mismatch, gap_open, gap_extend, dashes) < s) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// The start band of the host entries when the caller gives none.  A choice, not a measurement.
TA_HD inline uint32_t band_exact_default_start(uint32_t n, uint32_t m) {
    const uint32_t c = (band_exact_min(n, m) + 15) / 16;
    return c > 64 ? c : 64;
}

// Upper bound on any run-length CIGAR of an n x m pair (team_alignment.cpp:145-160).
TA_HD inline uint64_t cigar_slot_bytes(uint32_t n, uint32_t m) {
    return 2ull * ((uint64_t)n + m) + 2;
}

}  // namespace ta
