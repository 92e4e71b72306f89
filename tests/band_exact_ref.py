"""Exact banded alignment in pure Python: the rule of include/team_align_c.h
("Exact banded alignment") restated, and the two-round driver over the banded
checkers (tests/banded_ref.py, tests/banded_affine_ref.py).

Linear gaps read gap_open = 0, gap_extend = gap.  w is the pair's band clamped
to max(n, m), as the plans keep it."""
from __future__ import annotations

import banded_affine_ref as BAR
import banded_ref as BR

GLOBAL, LOCAL, SEMI = 0, 1, 2


def clamp(n: int, m: int, w: int) -> int:
    return min(w, max(n, m))


def default_start(n: int, m: int) -> int:
    """The host entries' start band when the caller gives none (a choice)."""
    return max(64, -(-min(n, m) // 16))


def full(n: int, m: int, w: int) -> bool:
    return n == 0 or m == 0 or w >= min(n, m)


def certifiable(gap_open: int, gap_extend: int) -> bool:
    return gap_open <= 0 and gap_extend <= 0


def count_dashes(q: bytes, t: bytes) -> int:
    return q.count(b"-") + t.count(b"-")


def bound(type: int, n: int, m: int, w: int, match: int, mismatch: int, gap_open: int, gap_extend: int,
          dashes: int) -> int:
    """U(w), for w < min(n, m)."""
    k = min(n, m) - w - 1
    u = max(match, mismatch, 0) * k
    if type == GLOBAL:
        u += gap_extend * max(0, abs(m - n) + 2 * (w + 1) - dashes)
        if dashes == 0:
            u += 2 * gap_open
    return u


def certified(type, n, m, w, match, mismatch, gap_open, gap_extend, dashes, score) -> bool:
    if full(n, m, w):
        return True
    if not certifiable(gap_open, gap_extend):
        return False
    return score > bound(type, n, m, w, match, mismatch, gap_open, gap_extend, dashes)


def needed(type, n, m, w, match, mismatch, gap_open, gap_extend, dashes, score) -> int:
    """The smallest w' > w with U(w') < score, else min(n, m): a plain loop."""
    if certifiable(gap_open, gap_extend):
        for v in range(w + 1, min(n, m)):
            if bound(type, n, m, v, match, mismatch, gap_open, gap_extend, dashes) < score:
                return v
    return min(n, m)


def certify(q: bytes, t: bytes, type, match, mismatch, gap_open, gap_extend, w, score):
    """(exact, band_needed) as ta_banded[_affine]_plan_certify writes them."""
    n, m = len(q), len(t)
    w = clamp(n, m, w)
    d = count_dashes(q, t)
    if certified(type, n, m, w, match, mismatch, gap_open, gap_extend, d, score):
        return 1, w
    return 0, needed(type, n, m, w, match, mismatch, gap_open, gap_extend, d, score)


def banded(q, t, type, match, mismatch, gap_open, gap_extend, w):
    """The banded checker of the gap family: gap_open None = linear."""
    if gap_open is None:
        return BR.align(q, t, type, match, mismatch, gap_extend, w)
    return BAR.align(q, t, type, match, mismatch, gap_open, gap_extend, w)


def plan(q: bytes, t: bytes, type, match, mismatch, gap_open, gap_extend, w0, score0):
    """(rounds, band_used) of the two-round entry from the first round's score
    alone.  gap_open None = linear."""
    go = 0 if gap_open is None else gap_open
    ok, w = certify(q, t, type, match, mismatch, go, gap_extend, w0, score0)
    return (1 if ok else 2), w


def align_exact(q: bytes, t: bytes, type, match, mismatch, gap_open, gap_extend, w0=None):
    """((score, cigar, target_begin), band_used, rounds).  gap_open None = linear."""
    n, m = len(q), len(t)
    w0 = clamp(n, m, default_start(n, m) if w0 is None else w0)
    first = banded(q, t, type, match, mismatch, gap_open, gap_extend, w0)
    rounds, w = plan(q, t, type, match, mismatch, gap_open, gap_extend, w0, first[0])
    if rounds == 1:
        return first, w, 1
    return banded(q, t, type, match, mismatch, gap_open, gap_extend, w), w, 2
