"""Pure-Python definition of the banded extension (include/team_align_c.h):
the checker of ta_banded_plan_* and ta_align_batch_banded.

For a pair of lengths n (query) and m (target) and its band w:

* The band.  Cell (i, j), 0 <= i <= n, 0 <= j <= m, is in band iff
  lo <= j - i <= hi with lo = min(0, m - n) - w and hi = max(0, m - n) + w.
  (0, 0) and (n, m) are always in band; w >= max(n, m) puts every cell in
  band; boundary cells (row 0, column 0) obey the same rule.
* The recurrence is team::Align's as oracle/align_oracle.c restates it, with
  out-of-band cells not existing: MATCH is always a candidate of an in-band
  interior cell, INSERT (left) and DELETE (up) only when their predecessor is
  in band.  Strict '>' in the order M, I, D; '-' bytes make their gap step
  free; the local clamp keeps the parent.
* Goals.  Global (n, m).  Local: first strict row-major maximum over in-band
  interior cells, target_begin = gj + 1.  Semi-global: column m with i
  ascending, then row n, in-band cells only, strict '>'; the trailing I / D
  run to (n, m) as in the reference.  Traceback, reversal, RLE and "1\\0" are
  the reference's.
* Degenerate pairs (n == 0 or m == 0): the unbanded closed forms.
* Range: (n + m + 2) * max(|match|, |mismatch|, |gap|) < 2^26, so plain
  integers (int64 here) are exact.

Only in-band cells are touched: one numpy row of at most hi - lo + 1 cells
per query row.  A row's INSERT chain h[j] = max(x[j], h[j-1] + g[j]) is the
running maximum of x[j] - G[j] (G the prefix sums of the gap steps g).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

GLOBAL, LOCAL, SEMI = 0, 1, 2
M_, I_, D_ = 0, 1, 2
NONE = -(1 << 40)  # the cost of a cell that does not exist (far below any sum of < 2^26 steps)


def band_limits(n: int, m: int, w: int):
    return min(0, m - n) - w, max(0, m - n) + w


def in_range(n: int, m: int, match: int, mismatch: int, gap: int) -> bool:
    return (n + m + 2) * max(abs(match), abs(mismatch), abs(gap)) < (1 << 26)


def rle(ops: str) -> bytes:
    """team_alignment.cpp:145-160; the empty op string gives "1" + NUL."""
    if not ops:
        return b"1\0"
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append(f"{e - k}{ops[k]}")
        k = e
    return "".join(out).encode()


def parse_cigar(cigar: bytes):
    """[(count, op)] of a run-length CIGAR ("1\\0": no ops)."""
    if cigar == b"1\0":
        return []
    runs, c = [], 0
    for ch in cigar.decode():
        if ch.isdigit():
            c = c * 10 + int(ch)
        else:
            runs.append((c, ch))
            c = 0
    return runs


@dataclass
class Result:
    score: int
    cigar: bytes | None
    target_begin: int
    gi: int
    gj: int

    def triple(self):
        return self.score, self.cigar, self.target_begin


def align_full(q: bytes, t: bytes, type: int, match: int, mismatch: int, gap: int, w: int,
               want_cigar: bool = True) -> Result:
    if type not in (GLOBAL, LOCAL, SEMI):
        raise ValueError("Unknown AlignmentType provided.")
    n, m = len(q), len(t)
    if not in_range(n, m, match, mismatch, gap):
        raise ValueError("out of the banded extension's range")
    lo, hi = band_limits(n, m, int(w))
    if n == 0 or m == 0:
        # today's closed forms; the whole boundary is in band by construction
        if type == GLOBAL:
            gi, gj, score = n, m, (n if n else m) * gap
        elif type == LOCAL:
            gi = gj = score = 0
        else:
            gi, gj, score = 0, (m if n == 0 else 0), 0
        tb = 1 if type == LOCAL else 0
        cig = None
        if want_cigar:
            ops = "" if type == LOCAL else "I" * m + "D" * n
            cig = rle(ops)
        return Result(score, cig, tb, gi, gj)

    init = gap if type == GLOBAL else 0
    qa = np.frombuffer(bytes(q), np.uint8)
    ta = np.frombuffer(bytes(t), np.uint8)
    gt = np.where(ta == ord("-"), 0, gap).astype(np.int64)  # indel(t[j-1]) at index j-1
    # rows[i] = (a, cost[a..b], parent[a..b]): the in-band columns of row i
    b0 = min(m, hi)
    rows = [(0, np.arange(b0 + 1, dtype=np.int64) * init, np.full(b0 + 1, I_, np.uint8))]  # :89-92
    best, gi, gj = None, 0, 0  # local argmax
    for i in range(1, n + 1):
        a, b = max(0, i + lo), min(m, i + hi)
        pa, pc, _ = rows[i - 1]
        pb = pa + len(pc) - 1
        cost = np.empty(b - a + 1, np.int64)
        par = np.empty(b - a + 1, np.uint8)
        j0 = max(a, 1)  # interior columns j0 .. b (never empty: every row holds an in-band interior cell)
        if a == 0:
            cost[0] = i * init  # :83-86
            par[0] = D_
        cols = np.arange(j0, b + 1)
        # up (i-1, j) and diag (i-1, j-1) where they exist
        up = np.full(len(cols), NONE, np.int64)
        s, e = max(j0, pa), min(b, pb)
        if s <= e:
            up[s - j0:e - j0 + 1] = pc[s - pa:e - pa + 1]
        diag = pc[cols - 1 - pa]  # same diagonal: always in band
        o0 = diag + np.where(ta[cols - 1] == qa[i - 1], match, mismatch)
        o2 = up + (0 if qa[i - 1] == ord("-") else gap)
        x = np.maximum(o0, o2)
        if type == LOCAL:
            x = np.maximum(x, 0)
        g = gt[cols - 1]
        G = np.cumsum(g)
        seed = cost[0] if a == 0 else NONE  # the cell left of column j0
        run = np.maximum.accumulate(np.concatenate(([seed], x - G)))
        h = run[1:] + G
        left = np.concatenate(([seed], h[:-1])) + g  # o1
        c = o0.copy()
        p = np.zeros(len(cols), np.uint8)
        mi = left > c  # strict '>', :108-113
        c = np.where(mi, left, c)
        p[mi] = I_
        md = o2 > c
        c = np.where(md, o2, c)
        p[md] = D_
        if type == LOCAL:
            c = np.maximum(c, 0)  # :185, parent kept
        assert np.array_equal(c, h)
        cost[j0 - a:] = h
        par[j0 - a:] = p
        rows.append((a, cost, par))
        if type == LOCAL:
            k = int(np.argmax(h))  # the row's first maximum
            if best is None or h[k] > best:  # :186-192 first strict max, row-major
                best, gi, gj = int(h[k]), i, j0 + k

    def cell(i, j):
        a, c, _ = rows[i]
        return int(c[j - a]) if a <= j < a + len(c) else None

    if type == GLOBAL:
        gi, gj, tb = n, m, 0
    elif type == LOCAL:
        tb = gj + 1
    else:
        best, gi, gj = None, 0, 0
        for i in range(0, n + 1):  # :265-270
            v = cell(i, m)
            if v is not None and (best is None or v > best):
                best, gi, gj = v, i, m
        for j in range(0, m + 1):  # :271-278
            v = cell(n, j)
            if v is not None and (best is None or v > best):
                best, gi, gj = v, n, j
        tb = 0
    score = cell(gi, gj)
    cig = None
    if want_cigar:
        ops = []
        i, j = gi, gj

        def parent(i, j):
            a, _, p = rows[i]
            return int(p[j - a])

        if type == LOCAL:
            while cell(i, j) > 0:  # :201-217
                d = parent(i, j)
                if d == M_:
                    ops.append("M"); i -= 1; j -= 1
                elif d == I_:
                    ops.append("I"); j -= 1
                else:
                    ops.append("D"); i -= 1
        else:
            while i > 0 or j > 0:  # :123-138 / :286-302
                d = parent(i, j)
                if i > 0 and j > 0 and d == M_:
                    ops.append("M"); i -= 1; j -= 1
                elif j > 0 and d == I_:
                    ops.append("I"); j -= 1
                elif i > 0 and d == D_:
                    ops.append("D"); i -= 1
                else:
                    raise ValueError("Unknown error in determining cigar string.")
        ops.reverse()
        if type == SEMI and (gj != m or gi != n):  # :306-315
            if gi == n:
                ops.extend("I" * (m - gj))
            elif gj == m:
                ops.extend("D" * (n - gi))
        cig = rle("".join(ops))
    return Result(score, cig, tb, gi, gj)


def align(q: bytes, t: bytes, type: int, match: int, mismatch: int, gap: int, w: int, want_cigar: bool = True):
    """(score, cigar bytes or None, target_begin), as Oracle.align returns them."""
    return align_full(q, t, type, match, mismatch, gap, w, want_cigar).triple()


def path_diagonals(cigar: bytes, n: int, m: int, type: int, gi: int, gj: int):
    """(dmin, dmax) of j - i over the cells the walk of this CIGAR visits: the
    ops from the start cell -- (0, 0), or for a local alignment the goal cell
    minus the consumption -- up to the goal cell (gi, gj); a semi-global
    CIGAR's run appended after the goal is not part of the walk."""
    runs = parse_cigar(cigar)
    if type == LOCAL:
        ci = sum(c for c, op in runs if op in "MD")
        cj = sum(c for c, op in runs if op in "MI")
        i, j = gi - ci, gj - cj
    else:
        i, j = 0, 0
    dmin = dmax = j - i
    for c, op in runs:
        if type == SEMI and (i, j) == (gi, gj):
            break
        if op == "I":
            if type == SEMI and i == gi == n and j + c > gj:  # the run merged with the appended tail
                c = gj - j
            j += c
            dmax = max(dmax, j - i)
        elif op == "D":
            if type == SEMI and j == gj == m and i + c > gi:
                c = gi - i
            i += c
            dmin = min(dmin, j - i)
        else:
            i += c
            j += c
    return dmin, dmax


def need_w(cigar: bytes, n: int, m: int, type: int, gi: int, gj: int) -> int:
    """The smallest band that holds every cell the walk of this CIGAR visits."""
    dmin, dmax = path_diagonals(cigar, n, m, type, gi, gj)
    return max(0, min(0, m - n) - dmin, dmax - max(0, m - n))
