"""Pure-Python definition of anchored (free-end) alignment
(include/team_align_c.h): the checker of ta_anchored_plan_* and
ta_align_batch_anchored.

For a pair of lengths n (query) and m (target) and its band w:

* The band is the banded extension's (banded_ref.band_limits): cell (i, j)
  exists iff lo <= j - i <= hi; boundary cells obey the same rule.
* Boundaries are global's, where in band: H(i, 0) = i * gap, H(0, j) = j * gap
  whatever the bytes; affine: open + L * extend, 0 at (0, 0), E(i, 0) =
  F(0, j) = -inf.
* The interior recurrence is banded_ref's global one (strict '>' in the order
  M, I, D, free gap steps at '-' bytes, no clamp); the affine form is
  banded_affine_ref's global H/E/F.
* Goal: (0, 0) with score 0 unless some in-band interior cell has H > 0; then
  the first strict row-major maximum over in-band interior cells (the scan
  starts from best = 0 at (0, 0)).  Boundary cells other than (0, 0) are
  never goals.  score = H(goal) >= 0.
* Walk: the global walk from (gi, gj) to (0, 0) (row 0: I x j, column 0:
  D x i; affine: three states, starting in H).  Reversal, RLE and "1\\0" are
  the reference's.
* Degenerate pairs (n == 0 or m == 0): goal (0, 0), score 0, "1\\0".
* Range: the banded families' rule.

The linear form touches one numpy row of in-band cells per query row (as
banded_ref does); the affine form is a plain per-cell loop.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import banded_affine_ref
import banded_ref
from banded_ref import band_limits, rle

M_, I_, D_ = 0, 1, 2
NONE = -(1 << 40)


@dataclass
class Result:
    score: int
    cigar: bytes | None
    gi: int
    gj: int

    def quad(self):
        return self.score, self.cigar, self.gi, self.gj


def align_full(q: bytes, t: bytes, match: int, mismatch: int, gap: int, w: int, gap_open: int | None = None,
               want_cigar: bool = True) -> Result:
    """gap_open=None: the linear form; gap_open=o: the affine form with gap_extend = gap."""
    q, t = bytes(q), bytes(t)
    n, m = len(q), len(t)
    if gap_open is None:
        if not banded_ref.in_range(n, m, match, mismatch, gap):
            raise ValueError("out of the anchored family's range")
    elif not banded_affine_ref.in_range(n, m, match, mismatch, gap_open, gap):
        raise ValueError("out of the anchored family's range")
    if n == 0 or m == 0:
        return Result(0, rle("") if want_cigar else None, 0, 0)
    if gap_open is None:
        return _linear(q, t, match, mismatch, gap, int(w), want_cigar)
    return _affine(q, t, match, mismatch, gap_open, gap, int(w), want_cigar)


def _linear(q, t, match, mismatch, gap, w, want_cigar):
    n, m = len(q), len(t)
    lo, hi = band_limits(n, m, w)
    qa = np.frombuffer(q, np.uint8)
    ta = np.frombuffer(t, np.uint8)
    gt = np.where(ta == ord("-"), 0, gap).astype(np.int64)
    b0 = min(m, hi)
    rows = [(0, np.arange(b0 + 1, dtype=np.int64) * gap, np.full(b0 + 1, I_, np.uint8))]
    best, gi, gj = 0, 0, 0
    for i in range(1, n + 1):
        a, b = max(0, i + lo), min(m, i + hi)
        pa, pc, _ = rows[i - 1]
        pb = pa + len(pc) - 1
        cost = np.empty(b - a + 1, np.int64)
        par = np.empty(b - a + 1, np.uint8)
        j0 = max(a, 1)
        if a == 0:
            cost[0] = i * gap
            par[0] = D_
        cols = np.arange(j0, b + 1)
        up = np.full(len(cols), NONE, np.int64)
        s, e = max(j0, pa), min(b, pb)
        if s <= e:
            up[s - j0:e - j0 + 1] = pc[s - pa:e - pa + 1]
        diag = pc[cols - 1 - pa]  # same diagonal: always in band
        o0 = diag + np.where(ta[cols - 1] == qa[i - 1], match, mismatch)
        o2 = up + (0 if qa[i - 1] == ord("-") else gap)
        x = np.maximum(o0, o2)
        g = gt[cols - 1]
        G = np.cumsum(g)
        seed = cost[0] if a == 0 else NONE
        run = np.maximum.accumulate(np.concatenate(([seed], x - G)))
        h = run[1:] + G
        left = np.concatenate(([seed], h[:-1])) + g
        c = o0.copy()
        p = np.zeros(len(cols), np.uint8)
        mi = left > c  # strict '>' in the order M, I, D
        c = np.where(mi, left, c)
        p[mi] = I_
        md = o2 > c
        c = np.where(md, o2, c)
        p[md] = D_
        assert np.array_equal(c, h)
        cost[j0 - a:] = h
        par[j0 - a:] = p
        rows.append((a, cost, par))
        k = int(np.argmax(h))  # the row's first maximum
        if h[k] > best:  # first strict maximum, row-major, from best = 0 at (0, 0)
            best, gi, gj = int(h[k]), i, j0 + k
    cig = None
    if want_cigar:
        ops = []
        i, j = gi, gj
        while i > 0 or j > 0:
            a, _, par = rows[i]
            d = int(par[j - a])
            if i > 0 and j > 0 and d == M_:
                ops.append("M"); i -= 1; j -= 1
            elif j > 0 and d == I_:
                ops.append("I"); j -= 1
            elif i > 0 and d == D_:
                ops.append("D"); i -= 1
            else:
                raise ValueError("Unknown error in determining cigar string.")
        ops.reverse()
        cig = rle("".join(ops))
    return Result(best, cig, gi, gj)


def _affine(q, t, match, mismatch, gap_open, gap_extend, w, want_cigar):
    n, m = len(q), len(t)
    lo, hi = band_limits(n, m, w)
    OX, X = gap_open + gap_extend, gap_extend
    dash = ord("-")
    got = [0 if c == dash else OX for c in t]
    get = [0 if c == dash else X for c in t]

    def edge(L):
        return gap_open + L * gap_extend if L else 0

    b0 = min(m, hi)
    A = [0]
    Hs = [[edge(j) for j in range(b0 + 1)]]
    Fs = [[NONE] * (b0 + 1)]
    Cs = [[0] * (b0 + 1)]  # bits 0..1 source (0 M, 1 I, 2 D), 2 E-ext, 3 F-ext
    best, gi, gj = 0, 0, 0
    for i in range(1, n + 1):
        a, b = max(0, i + lo), min(m, i + hi)
        pa, pH, pF = A[i - 1], Hs[i - 1], Fs[i - 1]
        pb = pa + len(pH) - 1
        qc = q[i - 1]
        goq, geq = (0, 0) if qc == dash else (OX, X)
        H = [0] * (b - a + 1)
        F = [NONE] * (b - a + 1)
        Cd = [0] * (b - a + 1)
        h_left, e_left, have_left = NONE, NONE, False
        if a == 0:
            H[0] = edge(i)
            h_left, e_left, have_left = H[0], NONE, True
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
            h = pH[j - 1 - pa] + (match if qc == t[j - 1] else mismatch)
            if e > h:
                h = e
                code |= 1
            if f > h:
                h = f
                code = (code & ~3) | 2
            if h > best:
                best, gi, gj = h, i, j
            k = j - a
            H[k], F[k], Cd[k] = h, f, code
            h_left, e_left, have_left = h, e, True
        A.append(a)
        Hs.append(H)
        Fs.append(F)
        Cs.append(Cd)
    cig = None
    if want_cigar:
        ops = []
        i, j, state = gi, gj, 0
        while True:
            if state == 0:
                if i == 0:
                    ops.extend("I" * j)
                    break
                if j == 0:
                    ops.extend("D" * i)
                    break
                src = Cs[i][j - A[i]] & 3
                if src == 0:
                    ops.append("M"); i -= 1; j -= 1
                else:
                    state = src
            elif state == 1:
                ext = (Cs[i][j - A[i]] >> 2) & 1
                ops.append("I"); j -= 1
                state = 1 if ext else 0
            else:
                ext = (Cs[i][j - A[i]] >> 3) & 1
                ops.append("D"); i -= 1
                state = 2 if ext else 0
            assert A[i] <= j < A[i] + len(Hs[i]), "the walk left the band"
        ops.reverse()
        cig = rle("".join(ops))
    return Result(best, cig, gi, gj)


def align(q: bytes, t: bytes, match: int, mismatch: int, gap: int, w: int, gap_open: int | None = None,
          want_cigar: bool = True):
    """(score, cigar bytes or None, query_end, target_end)."""
    return align_full(q, t, match, mismatch, gap, w, gap_open, want_cigar).quad()


def consumed(cigar: bytes):
    """(query bytes, target bytes) a CIGAR consumes."""
    runs = banded_ref.parse_cigar(cigar)
    return sum(c for c, op in runs if op in "MD"), sum(c for c, op in runs if op in "MI")


def need_w(cigar: bytes, n: int, m: int) -> int:
    """The smallest band of the (n, m) pair that holds every cell of this CIGAR's walk from (0, 0)."""
    gi, gj = consumed(cigar)
    dmin, dmax = banded_ref.path_diagonals(cigar, n, m, banded_ref.GLOBAL, gi, gj)
    return max(0, min(0, m - n) - dmin, dmax - max(0, m - n))


def stitch(left: bytes, mid: bytes, right: bytes) -> bytes:
    """The mapper's stitched CIGAR: the left piece's runs in reverse order, the
    middle, the right; adjacent runs of one op merged; "1\\0" pieces contribute
    nothing; an empty result is "1\\0"."""
    runs = list(reversed(banded_ref.parse_cigar(left))) + banded_ref.parse_cigar(mid) + banded_ref.parse_cigar(right)
    out = []
    for c, op in runs:
        if out and out[-1][1] == op:
            out[-1][0] += c
        else:
            out.append([c, op])
    return "".join(f"{c}{op}" for c, op in out).encode() if out else b"1\0"
