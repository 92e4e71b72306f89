// bioinfo1_amd/csrc/tm_stitch.h -- the mapper's host stitcher (--extend-ends,
// include/team_mapper_c.h): one read's CIGAR from its three pieces.  No HIP
// here: a CPU program tests it (tests/cpp/anchored_stitch_check.cpp).
//
// The left end is aligned backwards from the window (both sequences reversed),
// so its runs come in reverse order; the middle and the right end follow as
// they are.  Adjacent runs of one op are merged across the junctions, and a
// piece that is the empty op string ("1\0") contributes nothing; three empty
// pieces give "1\0".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

namespace tmap {

using CigarRuns = std::vector<std::pair<uint64_t, char>>;

// Appends the runs of a run-length CIGAR text to `runs`; false on a malformed
// text (a count of 0, a run without a count, trailing digits).
inline bool cigar_runs(const char* text, size_t len, CigarRuns& runs) {
    if (len == 2 && text[0] == '1' && text[1] == '\0') return true;
    uint64_t c = 0;
    bool digits = false;
    for (size_t k = 0; k < len; ++k) {
        const char ch = text[k];
        if (ch >= '0' && ch <= '9') {
            c = c * 10 + (uint64_t)(ch - '0');
            digits = true;
        } else {
            if (!digits || c == 0) return false;
            runs.push_back({c, ch});
            c = 0;
            digits = false;
        }
    }
    return !digits;
}

// out = the stitched CIGAR of (left reversed, mid, right); false if a piece is malformed.
inline bool stitch_cigar(const char* left, size_t n_left, const char* mid, size_t n_mid, const char* right,
                         size_t n_right, std::string& out) {
    CigarRuns l, runs;
    if (!cigar_runs(left, n_left, l)) return false;
    runs.assign(l.rbegin(), l.rend());
    if (!cigar_runs(mid, n_mid, runs) || !cigar_runs(right, n_right, runs)) return false;
    out.clear();
    for (size_t k = 0; k < runs.size();) {
        uint64_t c = runs[k].first;
        size_t e = k + 1;
        while (e < runs.size() && runs[e].second == runs[k].second) c += runs[e++].first;
        out += std::to_string(c);
        out += runs[k].second;
        k = e;
    }
    if (runs.empty()) out.assign("1\0", 2);
    return true;
}

}  // namespace tmap
