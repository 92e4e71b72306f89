"""The packed fills and the recomputing walk in every frame they choose from
the scoring and the shape, against the CPU oracle: the classified cases of
tests/frame_cases.py (pinned on the CPU by tests/test_frame_cases.py) and the
largest shapes fits_int16 admits, with inputs that drive H to its bounds.
Bit-exact: scores, target_begin and every CIGAR byte."""
import numpy as np
import pytest

import frame_cases as fc
from bioinfo1_amd import synth
from bioinfo1_amd.align import TA_PLAN_CK, TA_PLAN_NO_CK, Aligner, DevicePlan
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.gpu

RUN_ARGS = {"ck": (True, TA_PLAN_CK), "codes": (True, 0), "no_ck": (True, TA_PLAN_NO_CK), "score": (False, 0)}


@pytest.fixture(scope="module")
def aligner():
    return Aligner(0)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _kinds(rng, n, m, k, seed):
    """Pair k of an n x m shape, the kinds of test_ck_walk: 0 an insertion in the target (a
    block of N that matches nothing: an I run of more than a window's 32 columns), 1 the
    same in the query (a D run), 2 random ACGT, 3 and up related pairs."""
    al = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda c: al[rng.integers(4, size=c)].tobytes()  # noqa: E731
    if k >= 3:
        rb = synth.related_batch(1, n, m, seed=seed + k)
        return rb.query(0), rb.target(0)
    lo = min(n, m)
    core = rnd(lo - 200 if lo > 400 else lo // 2)
    gapb = b"N" * ((40 + 23 * k) if lo > 200 else (33 + 7 * k))
    if k == 0:
        q, t = core, core[: len(core) // 2] + gapb + core[len(core) // 2:]
    elif k == 1:
        q, t = core[: len(core) // 3] + gapb + core[len(core) // 3:], core
    else:
        q, t = rnd(n), rnd(m)
    return (q + rnd(max(0, n - len(q))))[:n], (t + rnd(max(0, m - len(t))))[:m]


def _case_batch(case):
    rng = np.random.default_rng(0xF4A3E + fc.CASES.index(case))
    pairs = []
    for s, (n, m, cnt, _, _, _) in enumerate(case["shapes"]):
        pairs += [_kinds(rng, n, m, k, 0xF4A + 16 * s) for k in range(cnt)]
    for k, (n, m) in enumerate(case.get("ragged", [])):
        pairs.append(_kinds(rng, n, m, k % 3, 0))
    b = synth.from_pairs(pairs)
    assert [(int(n), int(m)) for n, m in zip(b.qlen, b.tlen)] == fc.pair_shapes(case)
    return b


def _check(got, want, cigars, where):
    np.testing.assert_array_equal(got.scores, want.scores, err_msg=str(where))
    np.testing.assert_array_equal(got.target_begins, want.target_begins, err_msg=str(where))
    if cigars:
        for p in range(len(want.scores)):
            assert got.cigar(p) == want.cigar(p), (where, p)


@pytest.mark.parametrize("case", fc.CASES, ids=[c["id"] for c in fc.CASES])
def test_frame_case(aligner, oracle, case):
    """One table case: a batch of its shapes (per shape an odd number of pairs -- a long I
    run, a long D run, random, related --, so one pair is coupled with itself) through
    checkpoints and recomputing walks, codes and lane walks, blocked codes and band walks
    (local) and the score-only fill, each plan in the fill the table says.

    The recomputing walk decodes two pairs side by side, each in its own frame: pairs
    2k and 2k + 1 of the plan's order, which is sorted by cells, couples first.  A shape's
    odd count therefore puts its self-coupled pair beside the next smaller shape's first
    pair -- the cases "headline" and "mix_frames" list a max2 shape right above a max3_eq
    one, "mix_flex" has flexible couples between them in size (test_frame_cases.py
    asserts the adjacency from the planner's order)."""
    mode, sc = case["mode"], case["sc"]
    b = _case_batch(case)
    want = oracle.align_batch(b, mode, *sc, True)
    for run in fc.RUNS:
        if run == "no_ck" and mode != fc.LOCAL:
            continue
        cig, flags = RUN_ARGS[run]
        plan = DevicePlan(aligner, b, mode, *sc, cig, flags=flags)
        try:
            print(f"frame_case {case['id']} {run}: ck={plan.ck} blk={plan.blk} walk={plan.walk} "
                  f"dual_pairs={plan.dual_pairs} flex_pairs={plan.flex_pairs}")
            where = (case["id"], run, plan.ck, plan.blk, plan.walk, plan.dual_pairs, plan.flex_pairs)
            assert plan.dual_pairs - plan.flex_pairs == fc.dual_fill_pairs(case, run), where
            assert plan.flex_pairs == fc.flex_fill_pairs(case, run), where
            if run == "ck":
                assert bool(plan.ck) == case["ck"], where
                if case["ck"]:
                    assert plan.blk and plan.walk == 64, where
            else:
                assert not plan.ck, where
            plan.run()
            got = plan.results()
        finally:
            plan.close()
        _check(got, want, cig, (case["id"], run))


def _edge_pair(rng, n, m, k, seed):
    """Inputs that drive H to its bounds (n <= m): 0 identical, 1 nothing matches (for
    (3, 4, 0) every step a mismatch above match), 2 A^n against (AC)^(m/2), 3 random,
    4 related, 5 identical again (another sequence), then random."""
    al = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda c: al[rng.integers(4, size=c)].tobytes()  # noqa: E731
    if k in (0, 5):
        t = rnd(m)
        return t[:n], t
    if k == 1:
        return b"A" * n, b"C" * m
    if k == 2:
        return b"A" * n, (b"AC" * (m // 2 + 1))[:m]
    if k == 4:
        rb = synth.related_batch(1, n, m, seed=seed)
        return rb.query(0), rb.target(0)
    return rnd(n), rnd(m)


def _edge_run(aligner, oracle, mode, sc, rect):
    rng = np.random.default_rng(0xED6E + 31 * mode + 7 * sc[0] - sc[1] + 3 * sc[2] + rect)
    inside, past = fc.edge_batches(mode, sc, rect)
    for shapes, within in ((inside, True), (past, False)):
        pairs, seen = [], {}
        for n, m in shapes:
            k = seen[(n, m)] = seen.get((n, m), -1) + 1
            pairs.append(_edge_pair(rng, n, m, k, 0xED6 + n))
        b = synth.from_pairs(pairs)
        want = oracle.align_batch(b, mode, *sc, True)
        for flags in (0, TA_PLAN_CK):
            plan = DevicePlan(aligner, b, mode, *sc, True, flags=flags)
            try:
                where = (mode, sc, shapes[0], shapes[-1], flags, plan.ck, plan.walk, plan.dual_pairs, plan.flex_pairs)
                print("frame_edge", where)
                if within:
                    assert plan.dual_pairs == b.n_pairs and plan.flex_pairs == 0, where
                    if flags:
                        assert bool(plan.ck and plan.walk == 64) == fc.edge_takes_ck(mode, sc), where
                else:  # past the edge: no pair in the dual fill
                    assert plan.dual_pairs == plan.flex_pairs, where
                plan.run()
                got = plan.results()
            finally:
                plan.close()
            _check(got, want, True, where)


EDGE_KEYS = [(mode, sc) for mode in (0, 1, 2) for sc in fc.EDGES[mode]]


@pytest.mark.parametrize("mode,sc", EDGE_KEYS,
                         ids=["%s_%d_%d_%d" % (("global", "local", "semi")[mode], *sc) for mode, sc in EDGE_KEYS])
def test_frame_edge(aligner, oracle, mode, sc):
    """The largest square L fits_int16 admits for the mode and scoring (pinned in
    frame_cases.EDGES, never computed from the code under test here): L x L and
    (L - 1) x L pairs run in the dual fill, (L + 1) x (L + 1) pairs leave it and are
    exact in the int32 (or flexible) fill; identical, disjoint, periodic, random and
    related inputs; codes and lane walks, and checkpoints and recomputing walks."""
    _edge_run(aligner, oracle, mode, sc, False)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["global", "local", "semi"])
def test_frame_edge_two_pass(aligner, oracle, mode):
    """The same at a two-pass rectangular edge: 1030 rows and the largest m admitted."""
    _edge_run(aligner, oracle, mode, fc.RECT_EDGES[mode][0], True)
