"""The packed affine fill (ta_affine.hip aff_dual_pass) at the edges of its range
predicate and at every last-lane row count: plain data (no GPU import).

tests/test_affine_frame_cases.py pins every entry on the CPU against
affine_fits_int16 and build_affine_plan themselves (tests/cpp/frame_probe.cpp);
tests/test_affine_frame_gpu.py runs the same entries on the GPU against the
affine oracle.  The numbers are pinned here and never computed from the code
under test in a GPU test: a change to the predicate has to move this table.

An edge is keyed by (mode, (match, mismatch, open, extend), aspect):
  "square"    the largest L with an L x L pair admitted
  "wide17"    the widest m beside n = 17 rows (one full lane and a 1-row lane)
  "wide1030"  the widest m beside n = 1,030 rows (a two-pass query)
  "tall64"    the tallest n beside m = 64 columns (many passes)
and holds (n, m, kind).  kind "tight": the stored values S = V - ma j + X (j - i)
of the definition come within 1,000 of the predicate's +-32,000 at this shape
(`reach` below, closed forms only: |S| >= 31,000); "loose": the predicate binds
through a corner no input reaches (the product of the upper score bound and the
bias), or through the 16-bit column of the semi-global goal; kept for the routing.
"""
GLOBAL, SEMI = 0, 2

WIDE_N, TWO_PASS_N, TALL_M = 17, 1030, 64
# The semi-global fills report the column of row n's best in 16 bits: no couple past it
COLUMN_CAP = 65535

T, L = "tight", "loose"
EDGES = {
    (GLOBAL, (5, -4, -6, -3), "square"): (2904, 2904, T),
    (SEMI, (5, -4, -6, -3), "square"): (3993, 3993, T),
    (GLOBAL, (10, -4, -8, -6), "square"): (1450, 1450, T),
    (SEMI, (10, -4, -8, -6), "square"): (1995, 1995, T),
    (GLOBAL, (10, -4, -8, -6), "wide1030"): (1030, 1450, T),
    (SEMI, (10, -4, -8, -6), "wide1030"): (1030, 1995, T),
    (GLOBAL, (10, -4, -8, -6), "tall64"): (5216, 64, L),
    (SEMI, (10, -4, -8, -6), "tall64"): (5216, 64, T),
    (GLOBAL, (64, -64, -64, -64), "square"): (163, 163, T),
    (SEMI, (64, -64, -64, -64), "square"): (245, 245, T),
    (GLOBAL, (1, -1, -1, -200), "square"): (78, 78, T),
    (SEMI, (1, -1, -1, -200), "square"): (141, 141, T),
    (GLOBAL, (1, -1, -1, -200), "wide17"): (17, 78, T),
    (SEMI, (1, -1, -1, -200), "wide17"): (17, 157, T),
    (GLOBAL, (3, -2, -150, -10), "square"): (1363, 1363, T),
    (SEMI, (3, -2, -150, -10), "square"): (2423, 2423, T),
    (GLOBAL, (-7, 8, -3, -1), "square"): (2129, 2129, T),
    (SEMI, (-7, 8, -3, -1), "square"): (2129, 2129, T),
    (GLOBAL, (-7, 8, -3, -1), "wide1030"): (1030, 3757, L),
    (SEMI, (-7, 8, -3, -1), "wide1030"): (1030, 3757, L),
    (GLOBAL, (2, -1, 3, 2), "square"): (3189, 3189, L),
    (SEMI, (2, -1, 3, 2), "square"): (3189, 3189, L),
    (GLOBAL, (1, -1, -2, -1), "wide17"): (17, 10658, T),
    (SEMI, (1, -1, -2, -1), "wide17"): (17, 15988, T),
    (GLOBAL, (1, -1, -2, -1), "tall64"): (31915, 64, L),
    (SEMI, (1, -1, -2, -1), "tall64"): (31915, 64, T),
    # match == extend: the bias -ma j + X (j - i) does not depend on j and the value bound
    # admits any m; the semi-global column cap is the edge
    (SEMI, (0, -1, -2, 0), "wide17"): (17, COLUMN_CAP, L),
    (SEMI, (-1, -2, -2, -1), "wide17"): (17, COLUMN_CAP, L),
    (SEMI, (-2, -3, -5, -2), "wide17"): (17, COLUMN_CAP, L),
}
# Edges pinned on the CPU only: (value, the probe's cap).  The headline scoring's squares
# are too large for a quick test; (64, -64, -64, -64) admits no m beside 1,030 rows; in
# global mode (no goal column) match == extend admits any m.
CPU_EDGES = {
    (GLOBAL, (1, -1, -2, -1), "square"): (10658, 20000),
    (SEMI, (1, -1, -2, -1), "square"): (15988, 20000),
    (GLOBAL, (64, -64, -64, -64), "wide1030"): (0, 20000),
    (SEMI, (64, -64, -64, -64), "wide1030"): (0, 20000),
    (GLOBAL, (0, -1, -2, 0), "wide17"): (200000, 200000),
}
EDGE_KEYS = sorted(EDGES)
PAIRS_PER_SHAPE = 6  # even: the affine planner does not couple a pair with itself


def edge_id(key):
    mode, sc, aspect = key
    return "%s_%d_%d_%d_%d_%s" % ("semi" if mode == SEMI else "global", *sc, aspect)


def past_shape(key):
    """The shape one past the edge: one more column, one more row for the tall aspect, and
    both for a square (the edge is the largest L x L: where the rows bind, as column 0 does
    for semi (1, -1, -1, -200), L x (L + 1) is still admitted)."""
    n, m, _ = EDGES[key]
    return {"tall64": (n + 1, m), "square": (n + 1, m + 1)}.get(key[2], (n, m + 1))


def edge_batches(mode, sc, aspect):
    """(shapes within the edge, shapes past it): the edge shape and the shape one row
    shorter, then the shape one past the edge; PAIRS_PER_SHAPE pairs each."""
    n, m, _ = EDGES[(mode, sc, aspect)]
    k = PAIRS_PER_SHAPE
    return [(n, m)] * k + [(n - 1, m)] * k, [past_shape((mode, sc, aspect))] * k


def reach_all(mode, sc, n, m):
    """The stored values S = V - ma j + X (j - i) that an n x m pair provably holds,
    from the definition's closed forms alone (not the predicate, not the kernel):
      row 0:     H(0, j) = O + X j (global) or 0 (semi), j = 1..m, and F(0, j) = H - K
      column 0:  H(i, 0) = O + X i (global) or 0 (semi), i = 1..n + 15 (the last lane's
                 padding rows), and E(i, 0) = H - K;  K = |O| + |X| + 2
      diagonal:  H(i, i) = max(ma, mi) i for i <= min(n, m) when that is >= 0 and O, X <= 0:
                 no path scores above hs per diagonal step, and the diagonal of an identical
                 (ma >= mi) or an all-mismatch (mi > ma) pair attains it
      row n:     semi keeps H(n, j) - X n packed: an identical pair has H(n, n) = ma n when
                 n <= m and ma >= max(mi, 0), O, X <= 0; and every pair has
                 H(n, 1) >= min(0, O + X) when X <= 0 (a gap of one from the 0 boundary)
    Returns [(S, what)]: the values and where they lie."""
    ma, mi, O, X = sc
    K = abs(O) + abs(X) + 2
    out = []
    for j in (1, m):
        h = O + X * j if mode == GLOBAL else 0
        s = h - ma * j + X * j
        out += [(s, "row 0"), (s - K, "row 0 F")]
    for i in (1, n + 15):
        h = O + X * i if mode == GLOBAL else 0
        s = h - X * i
        out += [(s, "column 0"), (s - K, "column 0 E")]
    hs = max(ma, mi)
    if hs >= 0 and O <= 0 and X <= 0:
        i = min(n, m)
        out.append((hs * i - ma * i, "diagonal"))
    if mode == SEMI:
        if n <= m and ma >= max(mi, 0) and O <= 0 and X <= 0:
            out.append((ma * n - X * n, "row n"))
        if X <= 0:
            out.append((min(0, O + X) - X * n, "row n"))
    return out


def reach(mode, sc, n, m):
    """(S, what) of largest magnitude among reach_all's."""
    return max(reach_all(mode, sc, n, m), key=lambda v: abs(v[0]))


TIGHT_REACH = 31000

# ---- the semi-global pass, compiled once per valid-row count of the last lane (NV = 1..15
# and 16): every n mod 16 as a one-pass query (one full lane and the short one) and as the
# last pass of a two-pass query; 2 pairs per shape
NV_SHAPES = [(n, 40) for n in range(33, 49)] + [(n, 96) for n in range(1025, 1041)]
NV_PAIRS = 2

# ---- the semi-global goal in row n at a column past 65,535: (affine scoring, its linear
# twin or None, n, m).  4 pairs per case; the query occurs once in the target, ending at
# LONG_ENDS[pair]
LONG_COLUMNS = [
    ((0, -1, -2, 0), (0, -1, 0), 17, 66100),
    ((-1, -2, -2, -1), None, 17, 66100),
]
LONG_ENDS = (65990, 300, 300, 65990)
# In LONG_COLUMNS nothing scores above 0, so H(0, m) = 0 -- found first, in column m --
# is the goal and row n's column is never read.  With a positive mismatch the one best end
# does lie in row n: A^n against A^m with C^n at the occurrence scores n * mismatch there
# and less everywhere else (every other end misses a mismatch or pays a gap).  match ==
# extend (linear: match == gap) again, so the value bound admits any m.
LONG_ROW_GOALS = [
    ((0, 1, -2, 0), None, 17, 66100),
    ((-1, 1, -2, -1), (-1, 1, -1), 17, 66100),
]
