"""Directed cases of the row-stripe z-drop rule (TA_ZDROP_STRIPE), shared by the
CPU test of the reference (tests/test_anchored_zdrop_stripe_ref.py) and the GPU
tests.

The families are anchored_zdrop_cases.py's: an identical prefix, then all 'A'
against all 'C', so that the end dies at a known cell; 2/-4/-4 unless stated.

Each case names what it pins and carries the outcome the reference must give
for it: `drop` = the dropping stripe or None, and claims the CPU test asserts
ON THE REFERENCE (so a GPU comparison cannot pass vacuously):
  goal=(gi, gj), score=, swept=     the result
  tau_done=                         of the dropping stripe (ta_layout.h band_stripe_tau_done)
  pass_end=True                     the drop is seen only at the test after the pass's last step
  all_swept=True                    swept_steps is the undropped count, the result plain anchored's
  clamped=True                      i_last + hi > m in the dropping stripe
  carried=True                      the drop is in pass >= 1 and needs the B of the passes above
  c0_gt1=True                       the dropping pass starts at a column > 1
  higher=(i, j)                     a cell below the dropping stripe, computed before the fill leaves,
                                    whose H is above the score: the goal must not move there
"""
from __future__ import annotations

from dataclasses import dataclass, field

from anchored_zdrop_cases import INT32_MAX, RANGE_GAP, S244, _dash_pairs, dip_pair, pair, prefix, shift_pair


@dataclass
class Case:
    name: str
    q: bytes
    t: bytes
    w: int
    z: int
    drop: int | None
    scoring: tuple = S244
    gap_open: int | None = None
    claims: dict = field(default_factory=dict)
    az: int | None = None  # the Z of the case's affine twin, where the general mapping would move the drop


def _c(name, qt, w, z, drop, scoring=S244, az=None, **claims):
    return Case(name, qt[0], qt[1], w, z, drop, scoring, None, claims, az)


LINEAR = [
    # The goal (100, 100) lies in stripe 6 (rows 97 .. 112), whose row 112 still holds 200 - 48 = 152 < 160:
    # S_6 = 200.  Stripe 7's best is row 113: 200 - 52 = 148 < 160.
    _c("pass 0, small n: the stripe after the goal's drops", pair(100, 300, 300), 16, 40, 7, goal=(100, 100),
       score=200, tau_done=150, swept=192),
    # tau_done(g) = 17 g + 15 + w in pass 0 while i_last + hi <= m: g = 2 gives 49 + w.  L = 20: the goal is in
    # stripe 1, stripe 2 (rows 33 .. 48) holds nothing above -1.
    _c("tau_done = 63: seen at the first check", pair(20, 300, 300), 14, 3, 2, goal=(20, 20), score=40, tau_done=63,
       swept=64),
    _c("tau_done = 64: seen at the second check", pair(20, 300, 300), 15, 3, 2, goal=(20, 20), score=40, tau_done=64,
       swept=128),
    # 200 x 200, w = 16: 212 steps.  The goal (160, 160) ends stripe 9; stripe 10's best is 316, stripe 11's
    # (rows 177 .. 192) 320 - 68 = 252 < 280.  tau_done(11) = 200 - 1 + 11 = 210 >= 192.
    _c("the drop is seen only at the pass-end test", pair(160, 200, 200), 16, 40, 11, goal=(160, 160), score=320,
       tau_done=210, swept=212, pass_end=True),
    # n = 197: stripe 12 is rows 193 .. 197.  Z = 100: stripe 11's 252 >= 220, stripe 12's 320 - 132 = 188 < 220.
    _c("the dropping stripe is the last, partial one (n mod 16 = 5)", pair(160, 197, 200), 16, 100, 12,
       goal=(160, 160), score=320, all_swept=True),
    _c("the dropping stripe is the pair's last stripe (n mod 16 = 0)", pair(160, 208, 210), 16, 100, 12,
       goal=(160, 160), score=320, all_swept=True),
    # m = 120 < n: hi = 16, and from row 105 on i + hi > m.  The goal (100, 100) is in stripe 6; stripe 7
    # (rows 113 .. 128): 200 - 52 = 148 < 160; its last cell is (128, 120), not (128, 144).
    _c("i_last + hi clamped at m in the dropping stripe", pair(100, 300, 120), 16, 40, 7, goal=(100, 100), score=200,
       tau_done=126, swept=128, clamped=True),
    # The goal (1000, 1000) is in stripe 62; stripe 63 (rows 1009 .. 1024): 2000 - 36 = 1964 >= 1960; stripe 64,
    # lane 0 of pass 1 (rows 1025 .. 1040): 2000 - 100 = 1900 < 1960 -- with the B of pass 0.  Pass 0 has
    # 1050 + 63 = 1113 steps, pass 1 (c0 = 1009) 102 + 4 = 106; tau_done(64) = 1066 - 1009 = 57.
    _c("B carried over the pass boundary: the drop is lane 0 of pass 1", pair(1000, 1100, 1110), 16, 40, 64, az=25,
       goal=(1000, 1000), score=2000, tau_done=57, swept=1113 + 64, carried=True, c0_gt1=True),
    # L = 1016, w = 8: stripe 63 holds the goal's row 1016, stripe 64 2032 - 36 = 1996 >= 1992, stripe 65
    # drops.  Pass 0 has 1032 + 63 = 1095 steps, pass 1 (c0 = 1017) 84 + 4; tau_done(65) = 1064 - 1017 + 1 = 48.
    _c("B carried over the pass boundary: the drop is lane 1 of pass 1", pair(1016, 1100, 1100), 8, 40, 65, az=25,
       goal=(1016, 1016), score=2032, tau_done=48, swept=1095 + 64, carried=True, c0_gt1=True),
    _c("the stretch on the diagonal +20, two passes", shift_pair(1010, 20, 1080, 1120), 16, 40, 64,
       goal=(1010, 1030), carried=True, c0_gt1=True),
    _c("n=2100 L=300: passes 1 and 2 never swept", pair(300, 2100, 2110), 16, 40, 20, goal=(300, 300)),
    _c("Z=0, no positive cell: stripe 0 drops", (b"A" * 300, b"C" * 300), 16, 0, 0, goal=(0, 0), score=0,
       tau_done=31, swept=64),
    # Z = 0: the first stripe whose best is below the running best, here the one after the goal's.
    _c("Z=0 with positive cells", pair(100, 400, 400), 16, 0, 7, goal=(100, 100), score=200),
    _c("Z=INT32_MAX never fires", pair(100, 400, 400), 16, INT32_MAX, None, goal=(100, 100), score=200),
    _c("B < Z throughout: the guard holds", pair(20, 400, 400), 16, 41, None, goal=(20, 20), score=40),
    _c("w=0", pair(150, 290, 290), 0, 40, 10, goal=(150, 150)),
    _c("full band m>n", pair(150, 280, 300), 300, 40, 10, goal=(150, 150)),
    _c("'-' bytes in the query (the QDASH pass)", _dash_pairs()[0], 16, 40, 10),
    _c("'-' bytes in the target", _dash_pairs()[1], 16, 40, 10),
    # (rows 17 .. 32 hold nothing above -1: stripe 1 drops, after every step has been swept)
    _c("range limit 50 x 5, Z=0", (prefix(50), prefix(5)), 8, 0, 1, (1, -1, RANGE_GAP), all_swept=True),
    _c("range limit 50 x 5, Z large", (prefix(50), prefix(5)), 8, 1 << 30, None, (1, -1, RANGE_GAP)),
    # Prefix 96 (B = 192), 16 mismatching bases = the whole of stripe 6 (rows 97 .. 112), whose best is row
    # 97's 188 < 192 - 3: the drop.  tau_done(6) = 128 - 1 + 6 = 133, so the fill leaves after step 191, when
    # lane l has done the columns up to 192 - l: the diagonal cells down to (181, 181).  69 identical bases
    # follow the dip, rows 113 .. 181, and take H from 128 at (112, 112) to 266 at (181, 181) -- the pair's
    # highest H, computed, and not existing.
    _c("the end dies and comes back inside the detection lag", dip_pair(96, 16, 69, 400, 400), 16, 3, 6,
       goal=(96, 96), score=192, tau_done=133, swept=192, higher=(181, 181)),
]

# The same cases with affine gaps: open -3, extend -1 (match 2, mismatch -4).  A dead end falls by 1 per
# step there (one long gap), so the cases at Z = 40 run at Z = 10 and those at Z = 100 at Z = 25, or at the
# case's own `az`, chosen so that the same stripe drops.  Every claim but the score then holds in both gap
# families: the rule looks at rows, and the geometry is the same.
_AFFINE_Z = {40: 10, 100: 25}


def _affine_name(c):
    return c.name + " [affine]"


AFFINE = [Case(_affine_name(c), c.q, c.t, c.w, c.az if c.az is not None else _AFFINE_Z.get(c.z, c.z), c.drop,
               (c.scoring[0], c.scoring[1], -1), -3, {k: v for k, v in c.claims.items() if k != "score"})
          for c in LINEAR if not c.name.startswith("range limit")]
AFFINE += [Case(_affine_name(c), c.q, c.t, c.w, c.z, c.drop, (1, -1, RANGE_GAP // 2), RANGE_GAP // 2, dict(c.claims))
           for c in LINEAR if c.name.startswith("range limit")]
