"""Pure-Python definition of z-drop on anchored alignment
(include/team_align_c.h): the checker of ta_anchored_plan_create_zdrop,
ta_anchored_plan_swept_steps and ta_align_batch_anchored_zdrop.

Cell values are anchored alignment's (anchored_ref.py): same band, boundaries,
recurrence, tie order and '-' bytes, in both gap families.  Nothing is pruned.
The drop only decides which cells EXIST for the goal scan, and it is tied to
the order in which the fill sweeps them:

* Step index.  An in-band interior cell (i, j) lies in pass p = (i-1) div 1024
  and is computed at step
      tau(i, j) = j - c0(p) + ((i-1) mod 1024) div 16
  of that pass (c0(p): the pass's first swept column, ta_layout.h band_c0).
  Its segment is (p, tau div DROP_STEPS), DROP_STEPS = 64.  Pass p has
  ceil(steps_p / 64) segments, steps_p = c1 - c0 + 1 + nl_p - 1 (nl_p: the
  16-row stripes of the pass).
* Scan.  Segments in order (pass, then segment), B = 0 at the start:
    S = max(-1, every H of the segment's in-band interior cells, i <= n)
        (an empty segment: -1)
    if B >= Z and S < B - Z: the pair DROPS.  This segment's cells still
        exist; every later segment's cells, and those of later passes, do not.
    else B = max(B, S)
  (With S >= -1 the guard B >= Z follows from S < B - Z; it is kept because
  it says what is meant: nothing drops before the best has reached Z.)
* Goal: (0, 0) with score 0 unless an existing cell has H > 0, else the first
  strict row-major maximum over the existing cells.
* Walk, CIGAR, "1\\0", degenerate pairs, range: anchored alignment's.
* swept_steps: the fill steps the pair executed -- the whole passes before the
  drop plus min(64 (s + 1), steps_p) in the dropping pass (p, s); the sum of
  steps_p when nothing drops; 0 for a degenerate pair.
* Z: 0 <= Z <= INT32_MAX; zdrop=None (the C ABI's zdrop < 0) is off: plain
  anchored alignment, every step swept.

At 1/-1/-1 random DNA drifts upward inside a band and nothing drops; a scoring
with negative drift (2/-4/-4) is what makes a dead end fall.

fill() computes the cell values once; scan() and result() apply any number of
Z values to them.  `rules` breaks one rule at a time for the tests that show
the directed cases pin each of them.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import banded_affine_ref
import banded_ref
from banded_ref import band_limits, rle

M_, I_, D_ = 0, 1, 2
NONE = -(1 << 40)
ROWS, WAVE, PASS_ROWS = 16, 64, 1024
DROP_STEPS = 64
INT32_MAX = (1 << 31) - 1

# The rules a mutant reference breaks (tests/test_anchored_zdrop_ref.py).
RULES = {
    "keep_dropping_segment": True,  # the dropping segment's cells still exist
    "floor": -1,                    # S is at least this
    "guard_strict": False,          # True: B > Z instead of B >= Z
    "tau_pass": True,               # tau counts from the pass's own c0 and stripe
}


def clamp(n, m, w):
    return min(int(w), max(n, m))


def n_passes(n):
    return (n + PASS_ROWS - 1) // PASS_ROWS


def pass_geometry(n, m, w, p):
    """(c0, c1, nl, steps) of pass p, as ta_layout.h band_c0 / band_c1 / band_drop_steps."""
    lo, hi = band_limits(n, m, clamp(n, m, w))
    base = p * PASS_ROWS
    nrows = min(PASS_ROWS, n - base)
    c0 = max(1, base + 1 + lo)
    c1 = min(m, base + nrows + hi)
    nl = (nrows + ROWS - 1) // ROWS
    return c0, c1, nl, c1 - c0 + 1 + nl - 1


def total_steps(n, m, w):
    if n == 0 or m == 0:
        return 0
    return sum(pass_geometry(n, m, w, p)[3] for p in range(n_passes(n)))


def tau(n, m, w, i, j, rules=RULES):
    if not rules["tau_pass"]:  # broken: as if the pair were one pass
        return j - pass_geometry(n, m, w, 0)[0] + (i - 1) // ROWS
    p = (i - 1) // PASS_ROWS
    return j - pass_geometry(n, m, w, p)[0] + ((i - 1) % PASS_ROWS) // ROWS


@dataclass
class Fill:
    n: int
    m: int
    w: int
    affine: bool
    A: list = field(default_factory=list)      # first column of row i (0: the boundary column)
    H: list = field(default_factory=list)      # int64 array per row, columns A[i] ..
    code: list = field(default_factory=list)   # linear: parent per cell; affine: bits 0..1 source, 2 E-ext, 3 F-ext


@dataclass
class Scan:
    drop: tuple | None   # (pass, segment) of the dropping segment
    swept_steps: int
    score: int
    gi: int
    gj: int
    B: int               # the running best when the scan ended


@dataclass
class Result:
    score: int
    cigar: bytes | None
    gi: int
    gj: int
    swept_steps: int
    drop: tuple | None

    def quad(self):
        return self.score, self.cigar, self.gi, self.gj


def fill(q: bytes, t: bytes, match: int, mismatch: int, gap: int, w: int, gap_open: int | None = None) -> Fill:
    """The cell values of anchored alignment.  gap_open=None: linear; else affine with gap_extend = gap."""
    q, t = bytes(q), bytes(t)
    n, m = len(q), len(t)
    if gap_open is None:
        if not banded_ref.in_range(n, m, match, mismatch, gap):
            raise ValueError("out of the anchored family's range")
    elif not banded_affine_ref.in_range(n, m, match, mismatch, gap_open, gap):
        raise ValueError("out of the anchored family's range")
    f = Fill(n, m, int(w), gap_open is not None)
    if n == 0 or m == 0:
        return f
    if gap_open is None:
        _linear(f, q, t, match, mismatch, gap)
    else:
        _affine(f, q, t, match, mismatch, gap_open, gap)
    return f


def _linear(f, q, t, match, mismatch, gap):
    n, m = f.n, f.m
    lo, hi = band_limits(n, m, f.w)
    qa = np.frombuffer(q, np.uint8)
    ta = np.frombuffer(t, np.uint8)
    gt = np.where(ta == ord("-"), 0, gap).astype(np.int64)
    b0 = min(m, hi)
    f.A.append(0)
    f.H.append(np.arange(b0 + 1, dtype=np.int64) * gap)
    f.code.append(np.full(b0 + 1, I_, np.uint8))
    for i in range(1, n + 1):
        a, b = max(0, i + lo), min(m, i + hi)
        pa, pc = f.A[i - 1], f.H[i - 1]
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
        f.A.append(a)
        f.H.append(cost)
        f.code.append(par)


def _affine(f, q, t, match, mismatch, gap_open, gap_extend):
    n, m = f.n, f.m
    lo, hi = band_limits(n, m, f.w)
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
    Cs = [[0] * (b0 + 1)]
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
                    fv = fe
                    code |= 8
                else:
                    fv = fo
            else:
                fv = NONE
            h = pH[j - 1 - pa] + (match if qc == t[j - 1] else mismatch)
            if e > h:
                h = e
                code |= 1
            if fv > h:
                h = fv
                code = (code & ~3) | 2
            k = j - a
            H[k], F[k], Cd[k] = h, fv, code
            h_left, e_left, have_left = h, e, True
        A.append(a)
        Hs.append(H)
        Fs.append(F)
        Cs.append(Cd)
    f.A = A
    f.H = [np.asarray(h, np.int64) for h in Hs]
    f.code = Cs


def _row_segments(f, i, rules):
    """(first interior column, H of the row's interior cells, their segment numbers)."""
    a = f.A[i]
    j0 = max(a, 1)
    h = f.H[i][j0 - a:]
    cols = np.arange(j0, j0 + len(h))
    if rules["tau_pass"]:
        c0 = pass_geometry(f.n, f.m, f.w, (i - 1) // PASS_ROWS)[0]
        tt = cols - c0 + ((i - 1) % PASS_ROWS) // ROWS
    else:
        tt = cols - pass_geometry(f.n, f.m, f.w, 0)[0] + (i - 1) // ROWS
    return j0, h, tt // DROP_STEPS


def scan(f: Fill, zdrop: int | None, rules=RULES) -> Scan:
    n, m, w = f.n, f.m, f.w
    if zdrop is not None and not 0 <= zdrop <= INT32_MAX:
        raise ValueError("zdrop out of [0, INT32_MAX]")
    if n == 0 or m == 0:
        return Scan(None, 0, 0, 0, 0, 0)
    passes = n_passes(n)
    geo = [pass_geometry(n, m, w, p) for p in range(passes)]
    rows = [None] + [_row_segments(f, i, rules) for i in range(1, n + 1)]
    drop = None
    B = 0
    if zdrop is not None:
        for p in range(passes):
            nseg = (geo[p][3] + DROP_STEPS - 1) // DROP_STEPS
            # (a broken tau can number segments past the pass's own: they are scanned all the same)
            top = max([nseg - 1] + [int(rows[i][2].max()) for i in range(p * PASS_ROWS + 1,
                                                                          min(n, (p + 1) * PASS_ROWS) + 1)])
            S = np.full(top + 1, NONE, np.int64)
            for i in range(p * PASS_ROWS + 1, min(n, (p + 1) * PASS_ROWS) + 1):
                _, h, seg = rows[i]
                np.maximum.at(S, seg, h)
            for s in range(top + 1):
                sv = max(rules["floor"], int(S[s])) if rules["floor"] is not None else int(S[s])
                ok = B > zdrop if rules["guard_strict"] else B >= zdrop
                if ok and sv < B - zdrop:
                    drop = (p, s)
                    break
                B = max(B, sv)
            if drop:
                break
    if drop is None:
        swept = sum(g[3] for g in geo)
        last = (passes, 0)
    else:
        p, s = drop
        keep = rules["keep_dropping_segment"]  # (broken: neither its cells nor its steps count)
        swept = sum(g[3] for g in geo[:p]) + min(DROP_STEPS * (s + 1 if keep else s), geo[p][3])
        last = (p, s) if keep else (p, s - 1)
    best, gi, gj = 0, 0, 0
    for i in range(1, n + 1):
        p = (i - 1) // PASS_ROWS
        if p > last[0]:
            break
        j0, h, seg = rows[i]
        if p == last[0]:
            live = seg <= last[1]
            if not live.any():
                continue
            h = np.where(live, h, NONE)
        k = int(np.argmax(h))  # the row's first maximum
        if h[k] > best:
            best, gi, gj = int(h[k]), i, j0 + k
    return Scan(drop, swept, best, gi, gj, B)


def walk(f: Fill, gi: int, gj: int) -> bytes:
    ops = []
    i, j = gi, gj
    if not f.affine:
        while i > 0 or j > 0:
            d = int(f.code[i][j - f.A[i]])
            if i > 0 and j > 0 and d == M_:
                ops.append("M"); i -= 1; j -= 1
            elif j > 0 and d == I_:
                ops.append("I"); j -= 1
            elif i > 0 and d == D_:
                ops.append("D"); i -= 1
            else:
                raise ValueError("Unknown error in determining cigar string.")
    else:
        state = 0
        while True:
            if state == 0:
                if i == 0:
                    ops.extend("I" * j)
                    break
                if j == 0:
                    ops.extend("D" * i)
                    break
                src = f.code[i][j - f.A[i]] & 3
                if src == 0:
                    ops.append("M"); i -= 1; j -= 1
                else:
                    state = src
            elif state == 1:
                ext = (f.code[i][j - f.A[i]] >> 2) & 1
                ops.append("I"); j -= 1
                state = 1 if ext else 0
            else:
                ext = (f.code[i][j - f.A[i]] >> 3) & 1
                ops.append("D"); i -= 1
                state = 2 if ext else 0
            assert f.A[i] <= j < f.A[i] + len(f.H[i]), "the walk left the band"
    ops.reverse()
    return rle("".join(ops))


def result(f: Fill, zdrop: int | None, want_cigar: bool = True, rules=RULES) -> Result:
    s = scan(f, zdrop, rules)
    if f.n == 0 or f.m == 0:
        return Result(0, rle("") if want_cigar else None, 0, 0, 0, None)
    return Result(s.score, walk(f, s.gi, s.gj) if want_cigar else None, s.gi, s.gj, s.swept_steps, s.drop)


def align_full(q: bytes, t: bytes, match: int, mismatch: int, gap: int, w: int, gap_open: int | None = None,
               zdrop: int | None = None, want_cigar: bool = True, rules=RULES) -> Result:
    return result(fill(q, t, match, mismatch, gap, w, gap_open), zdrop, want_cigar, rules)


def align(q: bytes, t: bytes, match: int, mismatch: int, gap: int, w: int, gap_open: int | None = None,
          zdrop: int | None = None, want_cigar: bool = True):
    """(score, cigar bytes or None, query_end, target_end), as anchored_ref.align."""
    return align_full(q, t, match, mismatch, gap, w, gap_open, zdrop, want_cigar).quad()
