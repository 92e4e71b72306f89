/*
 * tests/annotate_dp.c -- TEST INFRASTRUCTURE ONLY (compiled by tests/annotate_ref.py).
 *
 * Score and goal cell of one pair, written for the annotate tests: two rolling
 * rows of the affine recurrences the project defines (a gap of length L costs
 * open + L * extend, a '-' byte makes its gap step free; open == 0 is
 * team::Align's linear gap), MATCH > INSERT > DELETE on ties, and the goal by
 * the reference's rule: global (n, m); local the first strict maximum in
 * row-major order starting from INT_MIN, clamped cells included; semi-global the
 * last column from row 0 down, then the last row from column 0, both strict.
 */
#include <limits.h>
#include <stdlib.h>

#define NEG (-(1 << 29))

int annotate_goal(const char* q, unsigned n, const char* t, unsigned m, int type, int match, int mismatch, int open,
                  int extend, int* score, unsigned* goal_i, unsigned* goal_j) {
    const int global = type == 0, local = type == 1;
    int* h = (int*)malloc(((size_t)m + 1) * sizeof(int)); /* H of the row above, then of this row */
    int* f = (int*)malloc(((size_t)m + 1) * sizeof(int)); /* F by column */
    if (!h || !f) {
        free(h), free(f);
        return 1;
    }
    int best = INT_MIN;
    unsigned gi = 0, gj = 0;
    h[0] = 0;
    for (unsigned j = 1; j <= m; ++j) {
        h[j] = global ? open + (int)j * extend : 0;
        f[j] = NEG;
    }
    if (type == 2 && h[m] > best) { /* last column, row 0 */
        best = h[m];
        gi = 0;
        gj = m;
    }
    for (unsigned i = 1; i <= n; ++i) {
        const char qc = q[i - 1];
        const int oq = qc == '-' ? 0 : open + extend, eq = qc == '-' ? 0 : extend;
        int diag = h[0];
        h[0] = global ? open + (int)i * extend : 0;
        int e = NEG;
        for (unsigned j = 1; j <= m; ++j) {
            const char tc = t[j - 1];
            const int ot = tc == '-' ? 0 : open + extend, et = tc == '-' ? 0 : extend;
            const int e_open = h[j - 1] + ot, e_ext = e + et;
            e = e_ext > e_open ? e_ext : e_open;
            const int f_open = h[j] + oq, f_ext = f[j] + eq;
            f[j] = f_ext > f_open ? f_ext : f_open;
            int v = diag + (qc == tc ? match : mismatch);
            if (e > v) v = e;
            if (f[j] > v) v = f[j];
            if (local) {
                if (v < 0) v = 0;
                if (v > best) {
                    best = v;
                    gi = i;
                    gj = j;
                }
            }
            diag = h[j];
            h[j] = v;
        }
        if (type == 2 && h[m] > best) { /* last column, row i */
            best = h[m];
            gi = i;
            gj = m;
        }
    }
    if (global) {
        gi = n;
        gj = m;
        best = h[m];
    } else if (type == 2) {
        for (unsigned j = 0; j <= m; ++j) /* last row */
            if (h[j] > best) {
                best = h[j];
                gi = n;
                gj = j;
            }
    } else if (best == INT_MIN) { /* local without a cell: H(0, 0) */
        best = 0;
    }
    *score = best;
    *goal_i = gi;
    *goal_j = gj;
    free(h), free(f);
    return 0;
}
