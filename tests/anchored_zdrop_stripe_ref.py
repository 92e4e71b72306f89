"""Pure-Python definition of the row-stripe z-drop rule on anchored alignment
(include/team_align_c.h, TA_ZDROP_STRIPE): the checker of
ta_anchored_plan_create_zdrop_rule and ta_align_batch_anchored_zdrop_rule.

Cell values are anchored alignment's; fill() and walk() are
anchored_zdrop_ref's.  Nothing is pruned.  The rule only decides which cells
EXIST for the goal scan, and it is tied to rows, not to the fill's sweep:

* Stripe g is rows 16 g + 1 .. min(16 g + 16, n), g = 0 .. ceil(n / 16) - 1:
  what one lane of the fill owns.  Every row has an in-band interior cell, so
  no stripe is empty.
* Stripe best: S_g = max(-1, every H of the stripe's in-band interior cells).
* Scan.  Stripes in order, B = 0 at the start:
    if B >= Z and S_g < B - Z: the pair DROPS at stripe g.  Stripe g's rows
        still exist; every later row does not.
    else B = max(B, S_g)
  B carries across pass boundaries.
* Goal: (0, 0) with score 0 unless an existing cell has H > 0, else the first
  strict row-major maximum over the existing cells.  (Never in the dropping
  stripe: S_g < B - Z <= B.)
* swept_steps.  The fill tests the rule after every 64th step of a pass and
  after the pass's last step, on every stripe whose last cell has been computed.
  Stripe g lies in pass p = g div 64 as lane l = g mod 64; its last cell is
  computed at step
      tau_done = min(m, i_last + hi) - c0(p) + l,   i_last = min(n, 16 g + 16).
  A drop at g executes sum_{p' < p} steps_p' + min(steps_p, 64 (tau_done div 64
  + 1)) steps; without a drop sum steps_p; 0 for a degenerate pair.
* Z: 0 <= Z <= INT32_MAX; zdrop=None is off: plain anchored alignment.

`rules` breaks one rule at a time for the tests that show the directed cases
pin each of them.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from anchored_zdrop_ref import (DROP_STEPS, INT32_MAX, NONE, PASS_ROWS, ROWS, WAVE, Fill, Result, clamp, fill,
                                n_passes, pass_geometry, total_steps, walk)
from banded_ref import band_limits

__all__ = ["fill", "walk", "scan", "result", "align", "align_full", "tau_done", "drop_steps", "n_stripes",
           "total_steps", "RULES"]

# The rules a mutant reference breaks (tests/test_anchored_zdrop_stripe_ref.py).
RULES = {
    "carry_B": True,                # B carries across pass boundaries (broken: reset to 0)
    "floor": -1,                    # S is at least this (None: no floor)
    "keep_dropping_stripe": True,   # the dropping stripe's rows still exist
    "goal_by_rows": True,           # the goal sees rows, not what the fill had computed at detection
    "clamp_m": True,                # tau_done clamps i_last + hi at m
}


def n_stripes(n):
    return (n + ROWS - 1) // ROWS


def tau_done(n, m, w, g, rules=RULES):
    """ta_layout.h band_stripe_tau_done."""
    _, hi = band_limits(n, m, clamp(n, m, w))
    i_last = min(n, ROWS * g + ROWS)
    jl = i_last + hi
    if rules["clamp_m"]:
        jl = min(m, jl)
    return jl - pass_geometry(n, m, w, g // WAVE)[0] + g % WAVE


def drop_steps(n, m, w, g, rules=RULES):
    """ta_layout.h band_stripe_swept_steps: the steps executed when the pair drops at stripe g."""
    p = g // WAVE
    before = sum(pass_geometry(n, m, w, pp)[3] for pp in range(p))
    return before + min(pass_geometry(n, m, w, p)[3], DROP_STEPS * (tau_done(n, m, w, g, rules) // DROP_STEPS + 1))


@dataclass
class Scan:
    drop: int | None     # the dropping stripe
    swept_steps: int
    score: int
    gi: int
    gj: int
    B: int               # the running best when the scan ended


def _interior(f: Fill, i):
    a = f.A[i]
    j0 = max(a, 1)
    return j0, f.H[i][j0 - a:]


def scan(f: Fill, zdrop: int | None, rules=RULES) -> Scan:
    n, m, w = f.n, f.m, f.w
    if zdrop is not None and not 0 <= zdrop <= INT32_MAX:
        raise ValueError("zdrop out of [0, INT32_MAX]")
    if n == 0 or m == 0:
        return Scan(None, 0, 0, 0, 0, 0)
    drop = None
    B = 0
    if zdrop is not None:
        for g in range(n_stripes(n)):
            if not rules["carry_B"] and g % WAVE == 0:
                B = 0
            S = max(int(_interior(f, i)[1].max()) for i in range(ROWS * g + 1, min(n, ROWS * g + ROWS) + 1))
            if rules["floor"] is not None:
                S = max(rules["floor"], S)
            if B >= zdrop and S < B - zdrop:
                drop = g
                break
            B = max(B, S)
    if drop is None:
        swept = total_steps(n, m, w)
        last_row = n
        t_detect = None
    else:
        swept = drop_steps(n, m, w, drop, rules)
        last_row = min(n, ROWS * drop + ROWS)
        if not rules["keep_dropping_stripe"]:
            # broken: neither its rows nor its steps count.  (The goal never lies in the dropping stripe, so
            # whether its rows "exist" shows only in the steps: the fill would leave a stripe earlier.)
            last_row = ROWS * drop
            swept = drop_steps(n, m, w, drop - 1, rules) if drop else 0
        t_detect = swept - sum(pass_geometry(n, m, w, pp)[3] for pp in range(drop // WAVE))
    best, gi, gj = 0, 0, 0
    if drop is not None and not rules["goal_by_rows"]:
        # broken: every cell of the dropping pass that the fill had computed when it left counts
        p = drop // WAVE
        c0 = pass_geometry(n, m, w, p)[0]
        for i in range(1, min(n, (p + 1) * PASS_ROWS) + 1):
            j0, h = _interior(f, i)
            if (i - 1) // PASS_ROWS == p:
                tt = np.arange(j0, j0 + len(h)) - c0 + ((i - 1) % PASS_ROWS) // ROWS
                h = np.where(tt < t_detect, h, NONE)
            k = int(np.argmax(h))
            if h[k] > best:
                best, gi, gj = int(h[k]), i, j0 + k
        return Scan(drop, swept, best, gi, gj, B)
    for i in range(1, last_row + 1):
        j0, h = _interior(f, i)
        k = int(np.argmax(h))  # the row's first maximum
        if h[k] > best:
            best, gi, gj = int(h[k]), i, j0 + k
    return Scan(drop, swept, best, gi, gj, B)


def result(f: Fill, zdrop: int | None, want_cigar: bool = True, rules=RULES) -> Result:
    from banded_ref import rle
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
