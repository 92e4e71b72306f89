// tests/cpp/band_exact_check.cpp -- the exact-band rule of ta_layout.h
// (band_exact_bound, band_exact_needed; the definition is in
// include/team_align_c.h) against a restatement of its own and a brute-force
// loop over w, built with g++ -fsanitize=address,undefined and run on its own
// (tests/test_band_exact_ref.py).  Random (n, m, w, scoring, dashes) with the
// corners: k = 0 (w = min(n, m) - 1), dashes at and beyond the gap steps G,
// and the largest lengths and scores the range rule allows (there the needed
// band is pinned by its defining property, not by the loop).
// Prints "ok <cases> <needed below the full band>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "ta_layout.h"

static long g_case = 0;

#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            std::fprintf(stderr, "FAIL line %d: %s (case %ld)\n", __LINE__, #c, g_case); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

struct Case {
    int type;
    uint32_t n, m, w;
    int ma, mi, go, ge;
    uint64_t dashes;
};

// The definition, written out once more.
static long long U(const Case& c, uint32_t w) {
    const long long mn = std::min(c.n, c.m), hs = std::max({c.ma, c.mi, 0});
    long long u = hs * (mn - (long long)w - 1);
    if (c.type == ta::kGlobal) {
        const long long G = std::llabs((long long)c.m - (long long)c.n) + 2 * ((long long)w + 1);
        u += (long long)c.ge * std::max<long long>(0, G - (long long)c.dashes);
        if (c.dashes == 0) u += 2ll * c.go;
    }
    return u;
}

static bool in_range(const Case& c) {
    const long long step = std::max({std::llabs(c.ma), std::llabs(c.mi), std::llabs(c.go) + std::llabs(c.ge)});
    return ((long long)c.n + c.m + 2) * step < (1ll << 26);
}

static long g_below = 0;

static void check(const Case& c, long long s, bool brute) {
    const uint32_t full = std::min(c.n, c.m);
    CHECK(c.w < full && in_range(c));
    const long long u = ta::band_exact_bound(c.type, c.n, c.m, c.w, c.ma, c.mi, c.go, c.ge, c.dashes);
    CHECK(u == U(c, c.w));
    CHECK(u > -(1ll << 28) && u < (1ll << 28));  // int32 would do inside the range rule
    CHECK(ta::band_exact_certified(c.type, c.n, c.m, c.w, c.ma, c.mi, c.go, c.ge, c.dashes, s) ==
          (c.go <= 0 && c.ge <= 0 && s > u));
    CHECK(ta::band_exact_certified(c.type, c.n, c.m, full, c.ma, c.mi, c.go, c.ge, c.dashes, s));
    const uint32_t r = ta::band_exact_needed(c.type, c.n, c.m, c.w, c.ma, c.mi, c.go, c.ge, c.dashes, s);
    CHECK(r > c.w && r <= full);
    if (c.go > 0 || c.ge > 0) {
        CHECK(r == full);
        return;
    }
    // the defining property: the first w' past w with U(w') < s (U does not increase)
    CHECK(r == full || U(c, r) < s);
    CHECK(r == c.w + 1 || U(c, r - 1) >= s);
    if (r + 1 < full) CHECK(U(c, r + 1) <= U(c, r));
    g_below += r < full;
    if (!brute) return;
    uint32_t want = full;
    long long prev = u;
    for (uint32_t v = c.w + 1; v < full; ++v) {
        const long long uv = U(c, v);
        CHECK(uv <= prev);
        prev = uv;
        if (uv < s && want == full) want = v;
    }
    CHECK(r == want);
}

int main() {
    std::mt19937_64 rng(0xBE7Au);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (uint64_t)(hi - lo + 1)); };
    // small pairs: the loop over every w
    for (; g_case < 6000; ++g_case) {
        Case c;
        c.type = (int)(g_case % 3);
        c.n = (uint32_t)pick(1, 400);
        c.m = (g_case % 4) ? (uint32_t)std::max<long long>(1, (long long)c.n + pick(-30, 30)) : (uint32_t)pick(1, 400);
        const uint32_t full = std::min(c.n, c.m);
        c.w = (g_case % 7 == 0) ? full - 1 : (uint32_t)pick(0, full - 1);  // k = 0 among them
        c.ma = (int)pick(-2, 5);
        c.mi = (int)pick(-6, 2);
        c.go = (g_case % 2) ? 0 : (int)pick(-6, (g_case % 11 == 0) ? 2 : 0);
        c.ge = (int)pick(-4, (g_case % 13 == 0) ? 2 : 0);
        const uint64_t G = (uint64_t)std::llabs((long long)c.m - (long long)c.n) + 2 * ((uint64_t)c.w + 1);
        switch (g_case % 5) {
            case 0: c.dashes = 0; break;
            case 1: c.dashes = G; break;          // every gap step free
            case 2: c.dashes = G + pick(1, 50); break;
            case 3: c.dashes = G ? G - 1 : 0; break;
            default: c.dashes = (uint64_t)pick(0, (long long)c.n + c.m); break;
        }
        const long long lo = U(c, full - 1) - 8, hi = U(c, c.w) + 8;
        check(c, pick(std::min(lo, hi), std::max(lo, hi)), true);
        check(c, U(c, c.w), true);      // the strict comparison, at the bound
        check(c, U(c, c.w) + 1, true);  // ... and one above it
    }
    // the range rule's edge: the longest pairs at unit scores, the largest scores at short pairs
    for (int k = 0; k < 600; ++k, ++g_case) {
        Case c;
        c.type = k % 3;
        if (k % 2) {
            c.n = (1u << 25) - 2 - (uint32_t)pick(0, 3);
            c.m = (1u << 26) - 3 - c.n;  // n + m + 2 = 2^26 - 1
            c.ma = 1;
            c.mi = (int)pick(-1, 1);
            c.go = (k % 4 == 1) ? 0 : -1;
            c.ge = (c.go == 0) ? -1 : 0;
        } else {
            c.n = (uint32_t)pick(1, 30);
            c.m = (uint32_t)pick(1, 30);
            const long long step = ((1ll << 26) - 1) / ((long long)c.n + c.m + 2);
            c.ma = (int)step;
            c.mi = -(int)step;
            c.go = -(int)(step / 2);
            c.ge = -(int)(step - step / 2);
        }
        const uint32_t full = std::min(c.n, c.m);
        c.w = (k % 5 == 0) ? full - 1 : (uint32_t)pick(0, full - 1);
        const uint64_t G = (uint64_t)std::llabs((long long)c.m - (long long)c.n) + 2 * ((uint64_t)c.w + 1);
        c.dashes = (k % 3 == 0) ? 0 : (k % 3 == 1) ? G + 7 : (uint64_t)pick(0, (long long)c.n + c.m);
        const long long lo = U(c, full - 1) - 8, hi = U(c, c.w) + 8;
        check(c, pick(std::min(lo, hi), std::max(lo, hi)), full <= 64);
        check(c, U(c, c.w), full <= 64);
    }
    // the start rule
    CHECK(ta::band_exact_default_start(0, 0) == 64 && ta::band_exact_default_start(1024, 5000) == 64);
    CHECK(ta::band_exact_default_start(1025, 5000) == 65 && ta::band_exact_default_start(40000, 32768) == 2048);
    std::printf("ok %ld %ld\n", g_case, g_below);
    return 0;
}
