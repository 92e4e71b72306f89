"""Which arithmetic each test case of the packed fills and the recomputing walk
runs: a classified table, plain data (no GPU import).

tests/test_frame_cases.py pins every entry on the CPU against the host
predicates themselves (tests/cpp/frame_probe.cpp: ta_layout.h local_max3_offset
and local_eq_gains, ta_planner.cpp fits_int16 / flex_* / build_plan, and the
walk's tab_ok restated from ta_walk_ck.hip); tests/test_frame_gpu.py runs the
same entries on the GPU against the oracle.  A change to a bound then moves a
case between kernels loudly: this table has to move with it.

Classes of a shape (n x m pairs of one case's mode and scoring):
  fill        "dual": an equal-shape couple runs in the int16 dual fill
              (fits_int16); "int32": it does not
  code_frame  local: the frame of the fills that store codes --
              "max3_z" (z = 1 - 16 match, three-input maxima) or "max2"
  ck_frame    local: the frame of the checkpoint and score-only fills, which the
              recomputing walk decodes per pair -- "max3_eq" (equal gains,
              z = -1, with off and dl) or "max2" (z = 1 - 16 match, off = dl = 0)
and of a case:
  tab         the recomputing walk's sweep: True table windows, False byte compares
              (a local gain match - gap or mismatch - gap outside [-128, 127])
  ck          a TA_PLAN_CK plan of the case's batch takes checkpoints and
              recomputing walks (local: gap <= 0, >= 8 pairs, every pair packed)

Flexible couples (ta_flex.hip) need flex_fits, that is |match|, |mismatch|,
|gap| <= 6: their gains always lie inside local_eq_gains' [-7, 8] and inside
tab_ok's range, and they store H itself, so they have no frame to choose; the
"mix_flex" case runs them beside both frames of the dual fill.

A shape is (n, m, pairs, fill, code_frame, ck_frame).  Every shape has an odd
number of pairs, so one is coupled with itself; within a case no two shapes
share (query passes, n mod 16), so no two left-over pairs make a flexible
couple and `dual_fill_pairs` below is exact.  A shape holds 5 pairs, or 3 (always
3 for local shapes above 1.5 M cells: the CPU oracle's time).
"""
GLOBAL, LOCAL, SEMI = 0, 1, 2

Z, EQ, M2 = "max3_z", "max3_eq", "max2"

CASES = [
    # ---- local: ck_frame = max3_eq, tab = True (the headline scoring); the 1830 x 1830
    # pairs are max2 by shape in the checkpoint frame only, and one of them walks beside a
    # 1000 x 1000 pair of the other frame
    dict(id="headline", mode=LOCAL, sc=(1, -1, -1), tab=True, ck=True, shapes=[
        (1830, 1830, 3, "dual", Z, M2), (1000, 1000, 5, "dual", Z, EQ), (300, 280, 5, "dual", Z, EQ)]),
    # ---- both frames inside one checkpoint plan: 1900 x 1900 is max2 by shape
    dict(id="mix_frames", mode=LOCAL, sc=(1, -1, -1), tab=True, ck=True, shapes=[
        (1900, 1900, 3, "dual", M2, M2), (1000, 1000, 3, "dual", Z, EQ), (300, 280, 3, "dual", Z, EQ)]),
    # ---- ... and beside ragged flexible couples (test_ck_walk_flex's shapes, one pair each)
    dict(id="mix_flex", mode=LOCAL, sc=(1, -1, -1), tab=True, ck=True, shapes=[
        (1900, 1900, 3, "dual", M2, M2), (1000, 1000, 3, "dual", Z, EQ)],
        ragged=[(517, 600), (517, 520), (517, 480), (517, 555), (517, 610), (1030, 990), (1030, 1100), (1030, 940),
                (2100, 700), (2100, 640), (2100, 690), (300, 260), (300, 280), (300, 300), (300, 240)]),
    # ---- ck_frame = max2 by score (a gain outside [-7, 8]), tab = True
    dict(id="score_max2_mismatch", mode=LOCAL, sc=(1, -9, -2), tab=True, ck=True, shapes=[
        (1900, 1900, 3, "dual", M2, M2), (1000, 1000, 5, "dual", Z, M2), (300, 280, 5, "dual", Z, M2)]),
    dict(id="score_max2_match", mode=LOCAL, sc=(10, -4, -6), tab=True, ck=True, shapes=[
        (190, 180, 5, "dual", M2, M2), (130, 130, 5, "dual", Z, M2)]),
    # ---- a shape past fits_int16 beside one within it: no checkpoints (an int32 pair)
    dict(id="past_edge", mode=LOCAL, sc=(10, -4, -6), tab=True, ck=False, shapes=[
        (210, 210, 3, "int32", M2, M2), (190, 180, 5, "dual", M2, M2)]),
    # ---- ck_frame = max2 by shape with gains inside [-7, 8] (beside (1, -1, -1) above)
    dict(id="shape_max2", mode=LOCAL, sc=(2, -3, -1), tab=True, ck=True, shapes=[
        (960, 960, 3, "dual", M2, M2), (900, 900, 3, "dual", Z, EQ), (300, 280, 5, "dual", Z, EQ)]),
    # ---- tab = False: byte-compare sweeps, in both checkpoint frames
    dict(id="tab_false_eq", mode=LOCAL, sc=(1, -1, -200), tab=False, ck=True, shapes=[
        (1082, 1082, 3, "dual", Z, M2), (1000, 1000, 5, "dual", Z, EQ), (300, 280, 5, "dual", Z, EQ)]),
    dict(id="tab_false_max2", mode=LOCAL, sc=(1, -130, -1), tab=False, ck=True, shapes=[
        (1500, 1500, 3, "dual", M2, M2), (1000, 1000, 5, "dual", Z, M2), (300, 280, 5, "dual", Z, M2)]),
    # ---- code_frame = max2 while ck_frame = max3_eq
    dict(id="code_max2_ck_eq", mode=LOCAL, sc=(5, -4, -3), tab=True, ck=True, shapes=[
        (390, 390, 3, "dual", M2, M2), (350, 350, 5, "dual", M2, EQ), (300, 280, 5, "dual", Z, EQ)]),
    # ---- the corners of local_eq_gains
    dict(id="eq_gains_inside", mode=LOCAL, sc=(8, -7, -1), tab=True, ck=True, shapes=[
        (230, 230, 5, "dual", M2, EQ), (180, 180, 5, "dual", Z, EQ)]),
    dict(id="eq_gains_inside_swapped", mode=LOCAL, sc=(-7, 8, -1), tab=True, ck=True, shapes=[
        (125, 125, 5, "dual", M2, EQ), (90, 90, 5, "dual", Z, EQ)]),
    dict(id="eq_gains_match_out", mode=LOCAL, sc=(9, -1, -1), tab=True, ck=True, shapes=[
        (215, 215, 5, "dual", M2, M2), (150, 150, 5, "dual", Z, M2)]),
    dict(id="eq_gains_mismatch_out", mode=LOCAL, sc=(1, -8, -1), tab=True, ck=True, shapes=[
        (1000, 1000, 5, "dual", Z, M2), (300, 280, 5, "dual", Z, M2)]),
    # ---- a non-positive match (every local H is 0)
    dict(id="match_negative", mode=LOCAL, sc=(-2, -3, -1), tab=True, ck=True, shapes=[
        (900, 900, 3, "dual", M2, EQ), (800, 800, 5, "dual", Z, EQ), (300, 280, 5, "dual", Z, EQ)]),
    dict(id="match_zero", mode=LOCAL, sc=(0, -1, -1), tab=True, ck=True, shapes=[
        (1000, 1000, 5, "dual", Z, EQ), (300, 280, 5, "dual", Z, EQ)]),
    # ---- mismatch above match, free gaps
    dict(id="mismatch_above", mode=LOCAL, sc=(3, 4, 0), tab=True, ck=True, shapes=[
        (462, 462, 5, "dual", M2, EQ), (300, 280, 5, "dual", Z, EQ)]),
    # ---- a positive gap: local takes no checkpoints, global and semi do
    dict(id="gap_positive_local", mode=LOCAL, sc=(2, -1, 2), tab=True, ck=False, shapes=[
        (320, 320, 5, "dual", M2, M2), (300, 280, 5, "dual", Z, EQ)]),
    dict(id="gap_positive_global", mode=GLOBAL, sc=(2, -1, 2), tab=True, ck=True, shapes=[
        (1030, 990, 3, "dual", None, None), (300, 280, 5, "dual", None, None)]),
    dict(id="gap_positive_semi", mode=SEMI, sc=(2, -1, 2), tab=True, ck=True, shapes=[
        (1030, 990, 3, "dual", None, None), (300, 280, 5, "dual", None, None)]),
    # ---- large magnitudes in the global / semi frame S = H - ma j + gap (j - i)
    dict(id="wide_global", mode=GLOBAL, sc=(64, -64, -64), tab=True, ck=True, shapes=[
        (160, 160, 5, "dual", None, None), (100, 120, 5, "dual", None, None)]),
    dict(id="wide_gap_global", mode=GLOBAL, sc=(1, -1, -200), tab=True, ck=True, shapes=[
        (70, 70, 5, "dual", None, None), (40, 60, 5, "dual", None, None)]),
    dict(id="wide_semi", mode=SEMI, sc=(10, -4, -6), tab=True, ck=True, shapes=[
        (1900, 1900, 3, "dual", None, None), (1030, 990, 3, "dual", None, None), (300, 280, 5, "dual", None, None)]),
]

# Plan properties of the cases with ragged (flexible) couples, per run: the pairs in
# the dual fill (dual_pairs - flex_pairs; a pair coupled with itself counts twice,
# as in ta_plan_dual_pairs) and in the flexible fill.  The other cases:
# dual_fill_pairs() and no flexible pairs.
RAGGED_PLANS = {
    "mix_flex": {"ck": (14, 12), "codes": (14, 12), "no_ck": (14, 12), "score": (14, 12)},
}

RUNS = ("ck", "codes", "no_ck", "score")  # TA_PLAN_CK, flags 0, TA_PLAN_NO_CK, want_cigar=False


def dual_fill_pairs(case, run):
    """Pairs of a case's batch in the int16 dual fill, as ta_plan_dual_pairs counts them
    (2 per couple, 2 for a pair coupled with itself): the couples of every "dual" shape,
    and its left-over pair where a lone pair takes the dual fill -- n m >= 4096, or any
    size under TA_PLAN_CK (ta_planner.cpp lone_dual)."""
    if case["id"] in RAGGED_PLANS:
        return RAGGED_PLANS[case["id"]][run][0]
    total = 0
    for n, m, cnt, fill, _, _ in case["shapes"]:
        if fill == "dual":
            total += 2 * (cnt // 2) + (2 if cnt % 2 and (n * m >= 4096 or run == "ck") else 0)
    return total


def flex_fill_pairs(case, run):
    return RAGGED_PLANS[case["id"]][run][1] if case["id"] in RAGGED_PLANS else 0


def pair_shapes(case):
    """(n, m) of every pair of the case's batch, in batch order."""
    out = []
    for n, m, cnt, _, _, _ in case["shapes"]:
        out += [(n, m)] * cnt
    return out + list(case.get("ragged", []))


# The largest square L x L that fits_int16 admits, per mode and scoring, for every
# scoring of the table whose L is at most 3000 (test_frame_edge runs L x L, (L - 1) x L
# and (L + 1) x (L + 1)); None: above 3000 in that mode.
SCORINGS = [(1, -1, -1), (2, -3, -1), (5, -4, -3), (1, -9, -2), (10, -4, -6), (8, -7, -1), (9, -1, -1), (1, -8, -1),
            (1, -130, -1), (1, -1, -200), (64, -64, -64), (-2, -3, -1), (0, -1, -1), (3, 4, 0), (2, -1, 2), (-7, 8, -1)]
EDGE_CAP = 3000
EDGES = {
    GLOBAL: {(5, -4, -3): 2905, (10, -4, -6): 1450, (9, -1, -1): 2902, (1, -1, -200): 75, (64, -64, -64): 164,
             (-7, 8, -1): 2128},
    LOCAL: {(1, -1, -1): 1998, (2, -3, -1): 997, (5, -4, -3): 398, (1, -9, -2): 1982, (10, -4, -6): 198,
            (8, -7, -1): 248, (9, -1, -1): 220, (1, -8, -1): 1984, (1, -130, -1): 1740, (1, -1, -200): 1600,
            (64, -64, -64): 29, (-2, -3, -1): 966, (3, 4, 0): 498, (2, -1, 2): 332, (-7, 8, -1): 131},
    SEMI: {(10, -4, -6): 1989, (1, -1, -200): 135, (64, -64, -64): 238, (-7, 8, -1): 2128},
}
# The largest squares of the two local three-input-max frames (0: the frame is never
# taken), for the scorings of the table: (max3_eq, max3_z)
LOCAL_FRAME_EDGES = {
    (1, -1, -1): (1803, 1855), (2, -3, -1): (925, 925), (5, -4, -3): (375, 337), (1, -9, -2): (0, 1824),
    (10, -4, -6): (0, 136), (8, -7, -1): (234, 187), (9, -1, -1): (0, 159), (1, -8, -1): (0, 1828),
    (1, -130, -1): (0, 1369), (1, -1, -200): (1054, 1105), (64, -64, -64): (0, 0), (-2, -3, -1): (15263, 834),
    (0, -1, -1): (15327, 15264), (3, 4, 0): (468, 453), (2, -1, 2): (313, 313), (-7, 8, -1): (234, 95),
}
# One two-pass rectangular edge per mode: n = 1030 rows and the largest m fits_int16 admits
RECT_N = 1030
RECT_EDGES = {GLOBAL: ((10, -4, -6), 1450), LOCAL: ((1, -1, -1), 2062), SEMI: ((10, -4, -6), 1995)}


def edge_batches(mode, sc, rect=False):
    """test_frame_edge's two batches: (shapes within the edge, shapes past it), 6 pairs (8 at the rectangular edge: local checkpoint plans need 8)
    per shape -- an even number, so every pair has a partner of its shape."""
    if rect:
        m = RECT_EDGES[mode][1]
        return [(RECT_N, m)] * 8, [(RECT_N, m + 1)] * 8
    L = EDGES[mode][sc]
    return [(L, L)] * 6 + [(L - 1, L)] * 6, [(L + 1, L + 1)] * 6


def edge_takes_ck(mode, sc):
    """A TA_PLAN_CK plan of the pairs within the edge takes checkpoints (local: gap <= 0)."""
    return mode != LOCAL or sc[2] <= 0
