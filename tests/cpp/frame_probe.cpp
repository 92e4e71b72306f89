// tests/cpp/frame_probe.cpp -- prints which arithmetic the packed fills and the
// recomputing walk choose for a scoring and a shape, from the host predicates
// themselves (ta_layout.h, ta_planner.cpp; no HIP).  tests/test_frame_cases.py
// compares the output with the classified table of tests/frame_cases.py.
// Lines on stdin, one answer line each:
//   mode ma mi gap n m         the predicates at an n x m pair
//   mode ma mi gap cap         the largest square L <= cap each predicate admits (0: none)
//   m mode ma mi gap n cap     the largest m <= cap each predicate admits beside n rows
//   p mode ma mi gap cigar flags n m [n m ...]   what build_plan makes of these pairs
// and of the affine family (affine_fits_int16, build_affine_plan):
//   a mode ma mi open ext n m      the predicate and the pass count at an n x m pair
//   e mode ma mi open ext cap      the largest square L <= cap it admits (0: none)
//   w mode ma mi open ext n cap    the widest m <= cap it admits beside n rows
//   t mode ma mi open ext m cap    the tallest n <= cap it admits beside m columns
//   q mode ma mi open ext cigar flags n m [n m ...]   what build_affine_plan makes of these pairs
#include <cstdint>
#include <cstdio>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ta_layout.h"
#include "ta_planner.h"

namespace {

// the recomputing walk's sweep kind (ta_walk_ck.hip: TAB windows need both gains
// (s - gap) in [-128, 127]; global / semi walks always take them)
bool tab_ok(int mode, int ma, int mi, int gap) {
    const int ua = ma - gap + 128, ub = mi - gap + 128;
    return mode != ta::kLocal || ((uint32_t)ua < 256u && (uint32_t)ub < 256u);
}

struct Pred {
    const char* name;
    std::function<bool(int, int, int, int, uint32_t, uint32_t)> f;
};

const Pred kPreds[] = {
    {"fits_int16", [](int mode, int ma, int mi, int g, uint32_t n, uint32_t m) { return ta::fits_int16(mode, n, m, ma, mi, g); }},
    {"flex_local_fits", [](int, int ma, int mi, int g, uint32_t n, uint32_t m) { return ta::flex_local_fits(n, m, ma, mi, g); }},
    {"flex_ck_fits", [](int mode, int ma, int mi, int g, uint32_t n, uint32_t m) { return ta::flex_ck_fits(mode, n, m, ma, mi, g); }},
    {"max3_z", [](int, int ma, int mi, int g, uint32_t n, uint32_t m) { return ta::local_max3_offset(n, m, ma, mi, g, false) >= 0; }},
    {"max3_eq", [](int, int ma, int mi, int g, uint32_t n, uint32_t m) { return ta::local_max3_offset(n, m, ma, mi, g, true) >= 0; }},
};

// the affine family's lines (v: the numbers after the kind letter); false: malformed
bool affine_line(char kind, const std::vector<long>& v) {
    if (v.size() < 6) return false;
    const int mode = (int)v[0], ma = (int)v[1], mi = (int)v[2], O = (int)v[3], X = (int)v[4];
    auto fits = [&](long n, long m) { return ta::affine_fits_int16(mode, (uint32_t)n, (uint32_t)m, ma, mi, O, X); };
    if (kind == 'a' && v.size() == 7) {
        std::printf("aff_at fits=%d passes=%u\n", (int)fits(v[5], v[6]), ta::n_passes((uint32_t)v[5]));
    } else if (kind == 'e' && v.size() == 6) {
        long L = v[5];
        while (L > 0 && !fits(L, L)) --L;
        std::printf("aff_square edge=%ld\n", L);
    } else if (kind == 'w' && v.size() == 7) {
        long m = v[6];
        while (m > 0 && !fits(v[5], m)) --m;
        std::printf("aff_wide edge=%ld\n", m);
    } else if (kind == 't' && v.size() == 7) {
        long n = v[6];
        while (n > 0 && !fits(n, v[5])) --n;
        std::printf("aff_tall edge=%ld passes=%u\n", n, ta::n_passes((uint32_t)n));
    } else if (kind == 'q' && v.size() >= 9 && v.size() % 2 == 1) {
        std::vector<uint32_t> ql, tl;
        for (size_t k = 7; k < v.size(); k += 2) {
            ql.push_back((uint32_t)v[k]);
            tl.push_back((uint32_t)v[k + 1]);
        }
        ta::AffinePlan pl;
        ta::build_affine_plan(pl, (uint32_t)ql.size(), ql.data(), tl.data(), mode, ma, mi, O, X, v[5] != 0, 1ull << 30,
                              (uint32_t)v[6]);
        std::printf("aff_plan couples=%zu singles=%zu dual_pairs=%zu chunks=%zu\n", pl.duals.size() / 2, pl.singles.size(),
                    pl.duals.size(), pl.chunks.size());
    } else {
        return false;
    }
    return true;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        const char kind = std::string("mpaewtq").find(line[0]) != std::string::npos ? line[0] : ' ';
        std::istringstream in(kind == ' ' ? line : line.substr(1));
        std::vector<long> v;
        for (long x; in >> x;) v.push_back(x);
        if (!in.eof() || v.size() < 5) {
            std::fprintf(stderr, "frame_probe: cannot read line: %s\n", line.c_str());
            return 2;
        }
        const int mode = (int)v[0], ma = (int)v[1], mi = (int)v[2], gap = (int)v[3];
        if (std::string("aewtq").find(kind) != std::string::npos) {
            if (!affine_line(kind, v)) {
                std::fprintf(stderr, "frame_probe: cannot read line: %s\n", line.c_str());
                return 2;
            }
            continue;
        }
        if (kind == 'p' && v.size() >= 8 && v.size() % 2 == 0) {
            std::vector<uint32_t> ql, tl;
            for (size_t k = 6; k < v.size(); k += 2) {
                ql.push_back((uint32_t)v[k]);
                tl.push_back((uint32_t)v[k + 1]);
            }
            ta::Plan pl;
            ta::build_plan(pl, (uint32_t)ql.size(), ql.data(), tl.data(), mode, ma, mi, gap, v[4] != 0, 1ull << 30,
                           (uint32_t)v[5]);
            // the recomputing walk decodes order[2k] and order[2k + 1] side by side in one 8-lane
            // group (ta_walk_ck.hip), each in its own frame: 0 equal-gain, 1 two-max, 2 the
            // flexible fill's H; count the groups whose two pairs differ
            std::vector<int> frame(ql.size(), 0);
            for (size_t p = 0; p < ql.size(); ++p)
                frame[p] = mode == ta::kLocal && ta::local_max3_offset(ql[p], tl[p], ma, mi, gap, true) < 0;
            for (uint32_t p : pl.flexes) frame[p] = 2;
            int mixed[3] = {0, 0, 0};  // eq | max2, eq | flex, max2 | flex
            for (size_t k = 0; k + 1 < pl.order.size(); k += 2) {
                const int a = frame[pl.order[k]], b = frame[pl.order[k + 1]];
                if (a != b) ++mixed[a + b - 1];
            }
            std::printf("plan ck=%d blk=%d walk=%d dual_pairs=%u flex_pairs=%zu singles=%zu chunks=%zu mixed_eq_max2=%d "
                        "mixed_eq_flex=%d mixed_max2_flex=%d\n", (int)pl.ck, (int)pl.blk, pl.walk_group, pl.n_dual_pairs,
                        pl.flexes.size(), pl.singles.size(), pl.chunks.size(), mixed[0], mixed[1], mixed[2]);
        } else if (kind == 'm' && v.size() == 6) {
            std::printf("edge_m mode=%d ma=%d mi=%d gap=%d n=%ld cap=%ld", mode, ma, mi, gap, v[4], v[5]);
            for (const Pred& p : kPreds) {
                long m = v[5];
                while (m > 0 && !p.f(mode, ma, mi, gap, (uint32_t)v[4], (uint32_t)m)) --m;
                std::printf(" %s=%ld", p.name, m);
            }
            std::printf("\n");
        } else if (kind == ' ' && v.size() == 6) {
            const uint32_t n = (uint32_t)v[4], m = (uint32_t)v[5];
            std::printf("at mode=%d ma=%d mi=%d gap=%d n=%u m=%u fits_int16=%d flex_fits=%d flex_local_fits=%d "
                        "flex_ck_fits=%d local_eq_gains=%d off_z=%d off_eq=%d tab_ok=%d\n",
                        mode, ma, mi, gap, n, m, (int)ta::fits_int16(mode, n, m, ma, mi, gap),
                        (int)ta::flex_fits(mode, ma, mi, gap), (int)ta::flex_local_fits(n, m, ma, mi, gap),
                        (int)ta::flex_ck_fits(mode, n, m, ma, mi, gap), (int)ta::local_eq_gains(ma, mi),
                        ta::local_max3_offset(n, m, ma, mi, gap, false), ta::local_max3_offset(n, m, ma, mi, gap, true),
                        (int)tab_ok(mode, ma, mi, gap));
        } else if (kind == ' ' && v.size() == 5) {
            std::printf("edge mode=%d ma=%d mi=%d gap=%d cap=%ld", mode, ma, mi, gap, v[4]);
            for (const Pred& p : kPreds) {
                long L = v[4];
                while (L > 0 && !p.f(mode, ma, mi, gap, (uint32_t)L, (uint32_t)L)) --L;
                std::printf(" %s=%ld", p.name, L);
            }
            std::printf("\n");
        } else {
            std::fprintf(stderr, "frame_probe: cannot read line: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
