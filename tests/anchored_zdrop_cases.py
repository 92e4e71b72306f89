"""Directed cases of z-drop on anchored alignment, shared by the CPU test of the
reference (tests/test_anchored_zdrop_ref.py) and the GPU tests.

The family: an identical prefix of length L (over G/T), then a query of all 'A'
against a target of all 'C' -- after the prefix every diagonal step loses, so
the end dies at a known cell.  Scoring 2/-4/-4 unless stated: the drop needs a
negative drift (at 1/-1/-1 nothing drops inside a band).

Each case names what it pins and carries the outcome the reference must give
for it: `drop` = the dropping (pass, segment) or None, and optional extra
claims (`goal`, `score`, `swept`, `goal_tau`, `dip_cell`).  The CPU test asserts
them ON THE REFERENCE, so a GPU comparison cannot pass vacuously.
"""
from __future__ import annotations

from dataclasses import dataclass, field

INT32_MAX = (1 << 31) - 1
S244 = (2, -4, -4)
RANGE_GAP = -1177348  # (50 + 5 + 2) * 1177348 < 2^26 <= (50 + 5 + 2) * 1177349: the pair at the range limit


def prefix(L: int) -> bytes:
    return bytes(b"GT"[((k * 2654435761) >> 7) & 1] for k in range(L))


def pair(L: int, n: int, m: int):
    """Identical prefix L, then all 'A' (query) against all 'C' (target)."""
    p = prefix(L)
    return p + b"A" * (n - L), p + b"C" * (m - L)


def dip_pair(L1: int, dip: int, L2: int, n: int, m: int):
    """Prefix L1, `dip` mismatching bases, L2 identical bases again, then dead."""
    p = prefix(L1 + dip + L2)
    q = p[:L1] + b"A" * dip + p[L1 + dip:] + b"A" * (n - L1 - dip - L2)
    t = p[:L1] + b"C" * dip + p[L1 + dip:] + b"C" * (m - L1 - dip - L2)
    return q, t


def shift_pair(L: int, lead: int, n: int, m: int):
    """The target leads with `lead` 'C's, so the identical stretch runs along the diagonal j - i = lead."""
    p = prefix(L)
    return p + b"A" * (n - L), b"C" * lead + p + b"C" * (m - L - lead)


@dataclass
class Case:
    name: str
    q: bytes
    t: bytes
    w: int
    z: int
    drop: tuple | None
    scoring: tuple = S244
    gap_open: int | None = None
    claims: dict = field(default_factory=dict)  # goal=(gi, gj), score=, swept=, goal_tau=, dip_cell=(i, j)


def _c(name, qt, w, z, drop, scoring=S244, **claims):
    return Case(name, qt[0], qt[1], w, z, drop, scoring, None, claims)


def _dash(b: bytes, at) -> bytes:
    b = bytearray(b)
    for k in at:
        b[k] = ord("-")
    return bytes(b)


def _dash_pairs():
    q, t = pair(150, 600, 610)
    return (_dash(q, (40, 41, 300)), t), (q, _dash(t, (60, 61, 400)))


LINEAR = [
    # the goal cell (L, L) of pass 0 has tau = L - 1 + (L - 1) div 16: 63 at L = 61, 64 at L = 62
    # (a goal can never lie in the dropping segment itself: S >= H(goal) >= B contradicts S < B - Z.  The
    # nearest thing is the goal at the last step before it: L = 61 at Z = 3)
    _c("pass0 L=61: (L,L) is the last step of segment 0, the drop is segment 1", pair(61, 400, 400), 16, 3, (0, 1),
       goal=(61, 61), score=122, swept=128, goal_tau=63),
    _c("pass0 L=62: (L,L) is the first step of segment 1, the drop is segment 2", pair(62, 400, 400), 16, 3, (0, 2),
       goal=(62, 62), score=124, swept=192, goal_tau=64),
    _c("pass0 L=61 Z=40", pair(61, 400, 400), 16, 40, (0, 2), goal=(61, 61), swept=192),
    _c("pass0 L=62 Z=40", pair(62, 400, 400), 16, 40, (0, 2), goal=(62, 62), swept=192),
    # 200 x 200, w = 16: steps = 200 + 13 - 1 = 212, segments 0..3, the last one partial (steps 192..211)
    _c("drop in the last, partial segment of a pass", pair(160, 200, 200), 16, 40, (0, 3), goal=(160, 160), swept=212),
    # one pass / two passes around L ~ 1000
    # n = 1024, m = 1040: 1103 steps, segments 0..17
    _c("n=1024 L=1000: the last segment of pass 0", pair(1000, 1024, 1040), 16, 40, (0, 17), goal=(1000, 1000),
       swept=1103),
    _c("n=1025 L=1000: still the last segment of pass 0, pass 1 never swept", pair(1000, 1025, 1041), 16, 40, (0, 17),
       goal=(1000, 1000), swept=1104),
    # the stretch along j - i = 20 ends at (1010, 1030), tau = 1092: in segment 17 of pass 0, which therefore
    # does not drop; row 1025, all of pass 1, does
    _c("n=1025 L=1010 on the diagonal +20: the first segment of pass 1", shift_pair(1010, 20, 1025, 1065), 16, 40,
       (1, 0), goal=(1010, 1030), swept=1185, goal_tau=1092),
    _c("n=2100 L=300: passes 1 and 2 never swept", pair(300, 2100, 2110), 16, 40, (0, 6), goal=(300, 300), swept=448),
    _c("n=2100 L=1100: the drop is in pass 1", pair(1100, 2100, 2110), 16, 40, (1, 2), goal=(1100, 1100)),
    _c("Z=0, no positive cell: immediate drop", (b"A" * 300, b"C" * 300), 16, 0, (0, 0), goal=(0, 0), score=0,
       swept=64),
    _c("Z=0 with positive cells", pair(100, 400, 400), 16, 0, (0, 2), goal=(100, 100), score=200),
    _c("Z=INT32_MAX never fires", pair(100, 400, 400), 16, INT32_MAX, None, goal=(100, 100), score=200),
    _c("B < Z throughout: the guard holds", pair(20, 400, 400), 16, 41, None, goal=(20, 20), score=40),
    _c("a dip deeper than Z but shorter than a segment does not fire; recovery, then the drop",
       dip_pair(100, 12, 120, 500, 500), 16, 40, (0, 5), goal=(232, 232), score=392, dip_cell=(112, 112)),
    _c("w=0", pair(150, 290, 290), 0, 40, (0, 3), goal=(150, 150)),
    _c("w=16 m<n", pair(150, 300, 280), 16, 40, (0, 3), goal=(150, 150)),
    _c("w=16 m>n", pair(150, 280, 300), 16, 40, (0, 3), goal=(150, 150)),
    _c("full band m<n", pair(150, 300, 280), 300, 40, (0, 3), goal=(150, 150)),
    _c("full band m>n", pair(150, 280, 300), 300, 40, (0, 3), goal=(150, 150)),
    _c("'-' bytes in the query (the QDASH pass)", _dash_pairs()[0], 16, 40, (0, 3)),
    _c("'-' bytes in the target", _dash_pairs()[1], 16, 40, (0, 3)),
    _c("n mod 16 == 0 in the last lane", pair(100, 320, 330), 16, 40, (0, 2), goal=(100, 100)),
    _c("n mod 16 == 1 in the last lane", pair(100, 321, 330), 16, 40, (0, 2), goal=(100, 100)),
    _c("n mod 16 == 15 in the last lane", pair(100, 335, 330), 16, 40, (0, 2), goal=(100, 100)),
    _c("the goal in the last lane's last valid row", pair(321, 321, 330), 16, 40, None, goal=(321, 321)),
    _c("range limit 50 x 5, Z=0", (prefix(50), prefix(5)), 8, 0, None, (1, -1, RANGE_GAP)),
    _c("range limit 50 x 5, Z large", (prefix(50), prefix(5)), 8, 1 << 30, None, (1, -1, RANGE_GAP)),
]

# The same family with affine gaps: open -3, extend -1 (match 2, mismatch -4).  A dead end falls by 1 per
# step there (one long gap), not by 4, so the cases at Z = 40 run at Z = 10, and their names say so.  The
# claims about the goal cell and the dip hold in both gap families and are kept; scores and step counts
# differ and come from AFFINE_EXPECT.
def _affine_name(c):
    return c.name.replace("Z=40", "Z=10") + " [affine]"


def _affine_claims(c):
    return {k: v for k, v in c.claims.items() if k in ("goal", "goal_tau", "dip_cell")}


AFFINE = [Case(_affine_name(c), c.q, c.t, c.w, 10 if c.z == 40 else c.z, None,
               (c.scoring[0], c.scoring[1], -1), -3, _affine_claims(c))
          for c in LINEAR if not c.name.startswith("range limit")]
AFFINE += [Case(_affine_name(c), c.q, c.t, c.w, c.z, None, (1, -1, RANGE_GAP // 2), RANGE_GAP // 2, {})
           for c in LINEAR if c.name.startswith("range limit")]

# The outcome the reference must give for the affine cases: (drop, swept_steps).
AFFINE_EXPECT = {
    'pass0 L=61: (L,L) is the last step of segment 0, the drop is segment 1 [affine]': ((0, 1), 128),
    'pass0 L=62: (L,L) is the first step of segment 1, the drop is segment 2 [affine]': ((0, 2), 192),
    'pass0 L=61 Z=10 [affine]': ((0, 2), 192),
    'pass0 L=62 Z=10 [affine]': ((0, 2), 192),
    'drop in the last, partial segment of a pass [affine]': ((0, 3), 212),
    'n=1024 L=1000: the last segment of pass 0 [affine]': ((0, 17), 1103),
    'n=1025 L=1000: still the last segment of pass 0, pass 1 never swept [affine]': ((0, 17), 1104),
    'n=1025 L=1010 on the diagonal +20: the first segment of pass 1 [affine]': ((1, 0), 1185),
    'n=2100 L=300: passes 1 and 2 never swept [affine]': ((0, 6), 448),
    'n=2100 L=1100: the drop is in pass 1 [affine]': ((1, 2), 1305),
    'Z=0, no positive cell: immediate drop [affine]': ((0, 0), 64),
    'Z=0 with positive cells [affine]': ((0, 2), 192),
    'Z=INT32_MAX never fires [affine]': (None, 424),
    'B < Z throughout: the guard holds [affine]': (None, 424),
    'a dip deeper than Z but shorter than a segment does not fire; recovery, then the drop [affine]': ((0, 4), 320),
    'w=0 [affine]': ((0, 3), 256),
    'w=16 m<n [affine]': ((0, 3), 256),
    'w=16 m>n [affine]': ((0, 3), 256),
    'full band m<n [affine]': ((0, 3), 256),
    'full band m>n [affine]': ((0, 3), 256),
    "'-' bytes in the query (the QDASH pass) [affine]": ((0, 3), 256),
    "'-' bytes in the target [affine]": ((0, 3), 256),
    'n mod 16 == 0 in the last lane [affine]': ((0, 2), 192),
    'n mod 16 == 1 in the last lane [affine]': ((0, 2), 192),
    'n mod 16 == 15 in the last lane [affine]': ((0, 2), 192),
    "the goal in the last lane's last valid row [affine]": (None, 350),
    'range limit 50 x 5, Z=0 [affine]': (None, 8),
    'range limit 50 x 5, Z large [affine]': (None, 8),
}
for _c_ in AFFINE:
    _c_.drop = AFFINE_EXPECT[_c_.name][0]
    _c_.claims["swept"] = AFFINE_EXPECT[_c_.name][1]
