// tests/cpp/band_probe.cpp -- the banded extension's geometry (ta_layout.h
// band_*) against brute force, on the CPU (tests/test_banded_ref.py).
// stdin: lines "n m w"; stdout per line: "n m w cells swept dwords" when every
// check holds, else "n m w FAIL <what>".
//
// Checks, cell by cell over the whole (n x m) matrix with the definition's
// predicate lo <= j - i <= hi:
//   * every in-band interior cell lies in the column range c0 .. c1 of the
//     pass that holds its row, and of no other pass's rows (passes split rows);
//   * c0 and c1 are tight: each holds an in-band cell of a row of its pass;
//   * band_cells is the number of in-band interior cells, band_swept_cells the
//     sum of the passes' rectangles;
//   * the passes' code regions follow one another without overlap, each holds
//     the last step a lane stores (columns + lanes in use - 1 steps), and the
//     pair's size is their sum.
#include <cstdint>
#include <cstdio>
#include <string>

#include "ta_layout.h"

using namespace ta;

static std::string check(uint32_t n, uint32_t m, uint32_t w, uint64_t* cells_out, uint64_t* swept_out,
                         uint64_t* dwords_out) {
    const long long d = (long long)m - (long long)n;
    const long long lo = (d < 0 ? d : 0) - (long long)w, hi = (d > 0 ? d : 0) + (long long)w;
    if (w <= (n > m ? n : m) && (band_lo(n, m, w) != lo || band_hi(n, m, w) != hi)) return "lo/hi";
    const uint32_t passes = n_passes(n);
    uint64_t cells = 0, swept = 0, off = 0;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t row_base = p * kPassRows;
        const uint32_t nrows = n - row_base < (uint32_t)kPassRows ? n - row_base : (uint32_t)kPassRows;
        const uint32_t c0 = band_c0(n, m, w, p), c1 = band_c1(n, m, w, p);
        if (c0 < 1 || c1 > m || c0 > c1) return "empty or out-of-matrix column range";
        bool at_c0 = false, at_c1 = false;
        for (uint32_t i = row_base + 1; i <= row_base + nrows; ++i)
            for (uint32_t j = 1; j <= m; ++j) {
                const long long dd = (long long)j - (long long)i;
                if (dd < lo || dd > hi) continue;
                ++cells;
                if (j < c0 || j > c1) return "in-band cell outside its pass's columns";
                at_c0 |= j == c0;
                at_c1 |= j == c1;
            }
        if (!at_c0 || !at_c1) return "column range not tight";
        swept += (uint64_t)(c1 - c0 + 1) * nrows;
        if (band_pass_offset(n, m, w, p) != off) return "pass offset";
        const uint32_t nl = (nrows + kRows - 1) / kRows;
        const uint32_t steps = band_pass_steps(n, m, w, p);
        if ((c1 - c0 + 1) + nl - 1 > steps) return "a stored step beyond the pass's region";
        off += (uint64_t)steps * kWave;
    }
    if (band_ptr_dwords(n, m, w) != (n && m ? off : 0)) return "pair size";
    if (band_cells(n, m, w) != cells) return "band_cells";
    if (band_swept_cells(n, m, w) != swept) return "band_swept_cells";
    if (swept < cells) return "swept < cells";
    *cells_out = cells;
    *swept_out = swept;
    *dwords_out = off;
    return "";
}

int main() {
    uint32_t n, m, w;
    while (std::scanf("%u %u %u", &n, &m, &w) == 3) {
        uint64_t cells = 0, swept = 0, dwords = 0;
        const std::string err = check(n, m, w, &cells, &swept, &dwords);
        if (err.empty())
            std::printf("%u %u %u %llu %llu %llu\n", n, m, w, (unsigned long long)cells, (unsigned long long)swept,
                        (unsigned long long)dwords);
        else
            std::printf("%u %u %u FAIL %s\n", n, m, w, err.c_str());
    }
    return 0;
}
