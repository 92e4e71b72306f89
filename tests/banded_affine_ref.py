"""Pure-Python definition of the banded affine extension
(include/team_align_c.h): the checker of ta_banded_affine_plan_* and
ta_align_batch_banded_affine.

For a pair of lengths n (query) and m (target) and its band w:

* The band is the banded extension's (banded_ref.band_limits): cell (i, j)
  exists iff lo <= j - i <= hi; boundary cells obey the same rule.
* The recurrence is oracle/affine_oracle.c's Gotoh H/E/F with out-of-band
  cells not existing.  E(i, j) = max(H(i, j-1) + go_t, E(i, j-1) + ge_t) when
  (i, j-1) is in band, else -inf, E-ext = (2nd > 1st); F likewise over
  (i-1, j).  MATCH is always a candidate of an in-band interior cell; INSERT
  wins iff E > diag, DELETE iff F > max(diag, E), both strict.  '-' bytes make
  their gap step free (open and extend); the local clamp keeps the source.
* Boundaries: H(i, 0) and H(0, j) are open + L * extend (global) or 0, where
  in band; E(i, 0) = F(0, j) = -inf.
* Goals are the banded extension's; the three-state walk, the reversal, the
  semi-global trailing run, the RLE and "1\\0" are the affine oracle's.
* Degenerate pairs (n == 0 or m == 0): the affine closed forms.
* Range: (n + m + 2) * max(|match|, |mismatch|, |open| + |extend|) < 2^26.

Only in-band cells are touched: per query row one list of at most
hi - lo + 1 cells, a plain per-cell loop.
"""
from __future__ import annotations

from banded_ref import GLOBAL, LOCAL, SEMI, Result, band_limits, need_w, parse_cigar, path_diagonals, rle  # noqa: F401

NONE = -(1 << 40)  # a cell (or an E / F) that does not exist: far below any sum of < 2^26 steps


def in_range(n: int, m: int, match: int, mismatch: int, gap_open: int, gap_extend: int) -> bool:
    return (n + m + 2) * max(abs(match), abs(mismatch), abs(gap_open) + abs(gap_extend)) < (1 << 26)


def align_full(q: bytes, t: bytes, type: int, match: int, mismatch: int, gap_open: int, gap_extend: int, w: int,
               want_cigar: bool = True) -> Result:
    if type not in (GLOBAL, LOCAL, SEMI):
        raise ValueError("Unknown AlignmentType provided.")
    q, t = bytes(q), bytes(t)
    n, m = len(q), len(t)
    if not in_range(n, m, match, mismatch, gap_open, gap_extend):
        raise ValueError("out of the banded affine extension's range")
    lo, hi = band_limits(n, m, int(w))
    if n == 0 or m == 0:  # the affine closed forms; the whole boundary is in band by construction
        if type == GLOBAL:
            L = n if n else m
            gi, gj, score = n, m, (gap_open + L * gap_extend if L else 0)
        elif type == LOCAL:
            gi = gj = score = 0
        else:
            gi, gj, score = 0, (m if n == 0 else 0), 0
        cig = None
        if want_cigar:
            cig = rle("" if type == LOCAL else "I" * m + "D" * n)
        return Result(score, cig, 1 if type == LOCAL else 0, gi, gj)

    glob, local = type == GLOBAL, type == LOCAL
    OX, X = gap_open + gap_extend, gap_extend
    dash = ord("-")
    got = [0 if c == dash else OX for c in t]  # horizontal step into column j: index j - 1
    get = [0 if c == dash else X for c in t]

    def edge(L):
        return gap_open + L * gap_extend if glob and L else 0

    # per row i: a (its first in-band column) and the lists H, F, code over columns a .. b
    # code: bits 0..1 source (0 M, 1 I, 2 D), 2 E-ext, 3 F-ext
    b0 = min(m, hi)
    A = [0]
    Hs = [[edge(j) for j in range(b0 + 1)]]
    Fs = [[NONE] * (b0 + 1)]
    Cs = [[0] * (b0 + 1)]
    best, gi, gj = None, 0, 0
    for i in range(1, n + 1):
        a, b = max(0, i + lo), min(m, i + hi)
        pa, pH, pF = A[i - 1], Hs[i - 1], Fs[i - 1]
        pb = pa + len(pH) - 1
        qc = q[i - 1]
        goq, geq = (0, 0) if qc == dash else (OX, X)
        H = [0] * (b - a + 1)
        F = [NONE] * (b - a + 1)
        C = [0] * (b - a + 1)
        h_left, e_left, have_left = NONE, NONE, False  # the cell (i, j - 1), where in band
        if a == 0:
            H[0] = edge(i)
            h_left, e_left, have_left = H[0], NONE, True  # E(i, 0) = -inf
        for j in range(max(a, 1), b + 1):
            code = 0
            if have_left:
                eo, ee = h_left + got[j - 1], e_left + get[j - 1]
                if ee > eo:
                    e, code = ee, 4
                else:
                    e = eo
            else:
                e = NONE
            if pa <= j <= pb:
                fo, fe = pH[j - pa] + goq, pF[j - pa] + geq
                if fe > fo:
                    f = fe
                    code |= 8
                else:
                    f = fo
            else:
                f = NONE
            h = pH[j - 1 - pa] + (match if qc == t[j - 1] else mismatch)  # same diagonal: always in band
            if e > h:
                h = e
                code |= 1
            if f > h:
                h = f
                code = (code & ~3) | 2
            if local:
                if h < 0:
                    h = 0
                if best is None or h > best:  # first strict maximum, row-major
                    best, gi, gj = h, i, j
            k = j - a
            H[k], F[k], C[k] = h, f, code
            h_left, e_left, have_left = h, e, True
        A.append(a)
        Hs.append(H)
        Fs.append(F)
        Cs.append(C)

    def cell(i, j):
        a = A[i]
        return Hs[i][j - a] if a <= j < a + len(Hs[i]) else None

    if glob:
        gi, gj, tb = n, m, 0
    elif local:
        tb = gj + 1
    else:
        best, gi, gj = None, 0, 0
        for i in range(0, n + 1):  # column m, i ascending
            v = cell(i, m)
            if v is not None and (best is None or v > best):
                best, gi, gj = v, i, m
        for j in range(0, m + 1):  # then row n
            v = cell(n, j)
            if v is not None and (best is None or v > best):
                best, gi, gj = v, n, j
        tb = 0
    score = cell(gi, gj)
    cig = None
    if want_cigar:
        ops = []
        i, j, state = gi, gj, 0  # 0 H, 1 E, 2 F
        while True:
            if state == 0:
                if local and (i == 0 or j == 0 or cell(i, j) <= 0):
                    break
                if not local and i == 0:
                    ops.extend("I" * j)
                    break
                if not local and j == 0:
                    ops.extend("D" * i)
                    break
                src = Cs[i][j - A[i]] & 3
                if src == 0:
                    ops.append("M")
                    i -= 1
                    j -= 1
                else:
                    state = src
            elif state == 1:
                ext = (Cs[i][j - A[i]] >> 2) & 1
                ops.append("I")
                j -= 1
                state = 1 if ext else 0
            else:
                ext = (Cs[i][j - A[i]] >> 3) & 1
                ops.append("D")
                i -= 1
                state = 2 if ext else 0
            assert cell(i, j) is not None, "the walk left the band"
        ops.reverse()
        if type == SEMI and (gj != m or gi != n):
            if gi == n:
                ops.extend("I" * (m - gj))
            elif gj == m:
                ops.extend("D" * (n - gi))
        cig = rle("".join(ops))
    return Result(score, cig, tb, gi, gj)


def align(q: bytes, t: bytes, type: int, match: int, mismatch: int, gap_open: int, gap_extend: int, w: int,
          want_cigar: bool = True):
    """(score, cigar bytes or None, target_begin), as Oracle.align_affine returns them."""
    return align_full(q, t, type, match, mismatch, gap_open, gap_extend, w, want_cigar).triple()
