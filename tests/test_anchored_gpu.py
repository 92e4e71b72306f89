"""Anchored (free-end) alignment on the GPU (ta_anchored_plan_*,
ta_align_batch_anchored) against its definition in tests/anchored_ref.py:
exact parity at the shapes where the kernels take another path (linear and
affine), goals in an upper pass while lower passes still run, '-' bytes, the
full band against the reference engine, the affine kernels at gap_open == 0,
chunks, annotate, the host entries and the errors."""
import anchored_ref as AR
import annotate_ref as R
import numpy as np
import pytest
from test_banded_gpu import BANDS, edge_batch

from bioinfo1_amd import align as A
from bioinfo1_amd import synth
from bioinfo1_amd.align import Aligner, DevicePlan
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.gpu

SCORINGS = [(1, -1, -1), (2, -3, -2)]
GAP_OPEN = -3


@pytest.fixture(scope="module")
def aligner():
    return Aligner(0)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def run_anchored(aligner, batch, sc, band, gap_open=0, want_cigar=True, budget=0, flags=0, annotate=False):
    """-> (BatchResult with the ends, annotation or None, chunks, pair_chunks, (band cells, swept cells, workspace))."""
    plan = DevicePlan.anchored(aligner, batch, *sc, band, gap_open=gap_open, want_cigar=want_cigar,
                               workspace_budget=budget, flags=flags)
    try:
        plan.run()
        if annotate:
            plan.annotate(eqx=True)
        res = plan.results()
        res.query_ends, res.target_ends = plan.ends()
        ann = plan.annotation() if annotate else None
        return res, ann, plan.chunks, plan.pair_chunks(), (plan.band_cells, plan.swept_cells, plan.workspace_bytes)
    finally:
        plan.close()


def quad(res, p):
    return int(res.scores[p]), res.cigar(p), int(res.query_ends[p]), int(res.target_ends[p])


def same_as(res, want, tag):
    np.testing.assert_array_equal(res.scores, want.scores, err_msg=str(tag))
    np.testing.assert_array_equal(res.query_ends, want.query_ends, err_msg=str(tag))
    np.testing.assert_array_equal(res.target_ends, want.target_ends, err_msg=str(tag))
    assert not res.target_begins.any(), tag
    if res.arena is not None and want.arena is not None:
        for p, (a, b) in enumerate(zip(res.cigars(), want.cigars())):
            assert a == b, (tag, p, a, b)


_defs = {}


def definition(batch, bands, sc, gap_open, key):
    """The definition's results for a batch, computed once per (key, scoring, gap model)."""
    k = (key, sc, gap_open)
    if k not in _defs:
        _defs[k] = [AR.align_full(batch.query(p), batch.target(p), *sc, int(bands[p]),
                                  gap_open=gap_open if gap_open else None) for p in range(batch.n_pairs)]
    return _defs[k]


def check_against_definition(aligner, batch, bands, sc, gap_open, key):
    want = definition(batch, bands, sc, gap_open, key)
    res, _, _, _, (cells, swept, _) = run_anchored(aligner, batch, sc, bands, gap_open)
    for p in range(batch.n_pairs):
        assert quad(res, p) == want[p].quad(), (key, sc, gap_open, p, int(batch.qlen[p]), int(batch.tlen[p]),
                                                int(bands[p]), quad(res, p), want[p].quad())
    assert not res.target_begins.any()
    assert swept >= cells > 0
    nocig, _, _, _, _ = run_anchored(aligner, batch, sc, bands, gap_open, want_cigar=False)
    assert nocig.arena is None
    same_as(nocig, res, (key, "score only"))
    return res, want


# ---- 1. exact parity with the definition where the kernels can go wrong
@pytest.mark.parametrize("gap_open", [0, GAP_OPEN])
@pytest.mark.parametrize("sc", SCORINGS)
def test_parity_at_the_edges(aligner, sc, gap_open):
    batch, bands = edge_batch()
    res, want = check_against_definition(aligner, batch, bands, sc, gap_open, "edges")
    P = batch.n_pairs - 3  # the three degenerate pairs come last
    for p in range(P, batch.n_pairs):
        assert quad(res, p) == (0, b"1\0", 0, 0), p
    # the full band (the device's, pinned to the definition and the reference below): what the band changed
    full, _, _, _, _ = run_anchored(aligner, batch, sc, np.maximum(batch.qlen, batch.tlen), gap_open)
    inside = sum(0 < w.gi < int(batch.qlen[p]) and 0 < w.gj < int(batch.tlen[p]) for p, w in enumerate(want[:P]))
    origin = sum((w.gi, w.gj) == (0, 0) for w in want[:P])
    changed = sum(quad(res, p) != quad(full, p) for p in range(P))
    print("edges", sc, gap_open, "inside", inside, "at (0, 0)", origin, "changed by the band", changed)
    assert (res.scores <= full.scores).all() and (res.scores >= 0).all()  # A4 (P2), A5
    assert inside >= 8 and origin >= 1 and changed >= 5


# Scoring at the range limit: (n + m + 2) * |gap| just below 2^26.  The padding rows of the last
# lane's stripe (below row n, computed like any row) then fall below -2^26; they must not reach the
# argmax key.  Every pair is a plan of its own, so that the limit is the pair's.
@pytest.mark.parametrize("gap_open", [0, 1])  # (1: the gap step split between open and extend)
@pytest.mark.parametrize("nm", [(50, 5), (5, 50), (49, 16), (17, 1), (1, 17), (1030, 9)])
def test_parity_at_the_range_limit(aligner, nm, gap_open):
    n, m = nm
    step = ((1 << 26) - 1) // (n + m + 2)
    b = synth.related_batch(1, n, m, seed=0x11A17 + 64 * n + m, rate=0.05)
    q, t = b.query(0), b.target(0)
    go, gap = (-(step // 2), -(step - step // 2)) if gap_open else (0, -step)
    for w in (max(n, m), 3, 0):
        want = AR.align_full(q, t, 1, -1, gap, w, gap_open=go if gap_open else None)
        res, _, _, _, _ = run_anchored(aligner, b, (1, -1, gap), w, go)
        assert quad(res, 0) == want.quad(), (nm, gap_open, w, quad(res, 0), want.quad())
        nocig, _, _, _, _ = run_anchored(aligner, b, (1, -1, gap), w, go, want_cigar=False)
        same_as(nocig, res, (nm, gap_open, w))
    with pytest.raises(ValueError, match="range"):  # one more and the pair is refused
        DevicePlan.anchored(aligner, b, 1, -1, -(((1 << 26) - 1) // (n + m + 2) + 1), 3)


# ---- 2. the goal in an upper pass while lower passes still run
CORES = (1, 15, 16, 17, 700, 1023, 1024, 1025, 1500, 2049)
TAILS = ((600, 600), (0, 300), (300, 0), (40, 700))


def tails_batch():
    pairs, k = [], 0
    for core in CORES:
        for tq, tt in TAILS:
            c = synth.related_batch(1, core, core, seed=0x7A11 + k, rate=0.05)
            u = synth.uniform_batch(1, tq, tt, seed=0x7A11 + 1000 + k)
            pairs.append((c.query(0) + u.query(0), c.target(0) + u.target(0)))
            k += 1
    return synth.from_pairs(pairs)


@pytest.mark.parametrize("sc", SCORINGS)
def test_tails_leave_the_goal_in_an_upper_pass(aligner, sc):
    batch = tails_batch()
    assert batch.n_pairs == 40
    w64 = np.full(batch.n_pairs, 64, np.uint32)
    _, want = check_against_definition(aligner, batch, w64, sc, 0, "tails, w = 64")
    inside = sum(0 < w.gi < int(batch.qlen[p]) and 0 < w.gj < int(batch.tlen[p]) for p, w in enumerate(want))
    upper = sum(w.gi > 0 and (w.gi - 1) // 1024 < (int(batch.qlen[p]) - 1) // 1024 for p, w in enumerate(want))
    print("tails", sc, "goals strictly inside", inside, "in a pass above the last", upper)
    assert inside >= 20 and upper >= 1
    full = np.maximum(batch.qlen, batch.tlen).astype(np.uint32)
    check_against_definition(aligner, batch, full, sc, 0, "tails, full band")


def test_tails_with_affine_gaps(aligner):
    batch = tails_batch()
    # the pairs with equal tails (n == m: the band's cells stay few enough for the per-cell definition)
    idx = [k for k in range(batch.n_pairs) if TAILS[k % len(TAILS)] == (600, 600)]
    sub = synth.from_pairs([(batch.query(k), batch.target(k)) for k in idx])
    check_against_definition(aligner, sub, np.full(sub.n_pairs, 64, np.uint32), (2, -3, -2), GAP_OPEN, "tails, affine")


# ---- 3. '-' bytes
@pytest.mark.parametrize("gap_open", [0, GAP_OPEN])
def test_parity_with_dash_bytes(aligner, gap_open):
    batch = synth.ragged_batch(60, 0, 140, alphabet=b"AC-GT")
    bands = np.array([BANDS[p % len(BANDS)] for p in range(batch.n_pairs)], np.uint32)
    check_against_definition(aligner, batch, bands, (1, -1, -1), gap_open, "dash")


# ---- 4. the full band against the reference engine (A1)
def test_full_band_is_the_global_alignment_of_the_prefixes(aligner, oracle):
    b = synth.related_batch(64, 300, 280)
    for sc in SCORINGS:
        res, _, _, _, (cells, swept, _) = run_anchored(aligner, b, sc, 300)
        assert cells == 64 * 300 * 280 == swept
        assert (res.query_ends > 0).all() and (res.target_ends > 0).all()
        pre = synth.from_pairs([(b.query(p)[:int(res.query_ends[p])], b.target(p)[:int(res.target_ends[p])])
                                for p in range(b.n_pairs)])
        want = oracle.align_batch(pre, 0, *sc, True)
        np.testing.assert_array_equal(res.scores, want.scores)
        assert res.cigars() == want.cigars()
        # and no later end scores higher: the global score of the whole pair is not above it
        whole = oracle.align_batch(b, 0, *sc, False)
        assert (res.scores >= whole.scores).all() and (res.scores >= 0).all()


# ---- 5. A3 on the device: the affine kernels at gap_open == 0
@pytest.mark.parametrize("sc", SCORINGS)
def test_affine_kernels_at_gap_open_0_equal_the_linear_plan(aligner, sc):
    batch, bands = edge_batch()
    lin, _, _, _, (_, _, ws) = run_anchored(aligner, batch, sc, bands)
    aff, _, _, _, (_, _, ws_aff) = run_anchored(aligner, batch, sc, bands, flags=A.TA_ANCHORED_AFFINE_KERNELS)
    same_as(aff, lin, ("A3", sc))
    assert ws_aff > ws  # 8-byte code entries, not 4: the other kernels ran
    nocig, _, _, _, _ = run_anchored(aligner, batch, sc, bands, flags=A.TA_ANCHORED_AFFINE_KERNELS, want_cigar=False)
    same_as(nocig, lin, ("A3, score only", sc))


# ---- 6. chunks
@pytest.mark.parametrize("gap_open", [0, GAP_OPEN])
def test_chunks(aligner, gap_open):
    b, sc = synth.related_batch(48, 3000, 2900), (1, -1, -1)
    one, _, chunks, _, (_, _, ws) = run_anchored(aligner, b, sc, 64, gap_open)
    assert chunks == 1
    many, _, nch, of_pair, (_, _, ws_c) = run_anchored(aligner, b, sc, 64, gap_open, budget=max(ws // 4, 1))
    assert nch >= 3 and ws_c < ws
    same_as(many, one, ("chunks", gap_open))
    assert sorted(set(int(c) for c in of_pair)) == list(range(nch))
    for p in (0, 17, 47):  # and the results are the definition's
        want = AR.align_full(b.query(p), b.target(p), *sc, 64, gap_open=gap_open if gap_open else None)
        assert quad(one, p) == want.quad(), (gap_open, p)


def test_fill_and_traceback_per_chunk(aligner):
    b, sc = synth.related_batch(24, 1500, 1400), (2, -3, -2)
    whole, _, _, _, (_, _, ws) = run_anchored(aligner, b, sc, 32)
    plan = DevicePlan.anchored(aligner, b, *sc, 32, workspace_budget=max(ws // 3, 1))
    try:
        assert plan.chunks >= 2
        for c in range(plan.chunks):
            plan.run_fill(c)
            plan.run_traceback(c)
        res = plan.results()
        res.query_ends, res.target_ends = plan.ends()
    finally:
        plan.close()
    same_as(res, whole, "per chunk")


# ---- 7. annotate
@pytest.mark.parametrize("gap_open", [0, GAP_OPEN])
def test_annotate(aligner, gap_open):
    sc = (2, -3, -2)
    b = synth.ragged_batch(80, 0, 200, seed=0xA22, alphabet=b"AC-GT")
    bands = np.array([BANDS[(3 * p) % len(BANDS)] for p in range(b.n_pairs)], np.uint32)
    res, ann, _, _, _ = run_anchored(aligner, b, sc, bands, gap_open, annotate=True)
    moved = 0
    for p in range(b.n_pairs):
        q, t = b.query(p), b.target(p)
        want = AR.align_full(q, t, *sc, int(bands[p]), gap_open=gap_open if gap_open else None)
        assert quad(res, p) == want.quad(), (gap_open, p)
        # the records of the global alignment of the prefixes with this CIGAR
        info, eqx = R.expected(q[:want.gi], t[:want.gj], R.GLOBAL, want.cigar, want.gi, want.gj)
        got = {f: int(ann.info[f][p]) for f in R.FIELDS}
        assert got == info, (gap_open, p, want.cigar, got, info)
        assert ann.eqx(p) == eqx, (gap_open, p)
        assert got["n_free"] == 0 and got["query_begin"] == 0 and got["target_begin"] == 0
        assert R.score_from_info(info, sc, gap_open or None) == want.score or b"-" in q + t, (gap_open, p)
        moved += want.gi > 0
    assert moved >= 10


# ---- 8. the host batch, the one-pair call, the errors
@pytest.mark.parametrize("gap_open", [0, GAP_OPEN])
def test_host_batch_equals_the_plan(aligner, gap_open):
    b = synth.ragged_batch(120, 0, 260, seed=0x4057, alphabet=b"AC-GT")
    bands = np.array([BANDS[p % len(BANDS)] for p in range(b.n_pairs)], np.uint32)
    plan, _, _, _, _ = run_anchored(aligner, b, (1, -1, -1), bands, gap_open)
    host = aligner.align_batch_anchored(b, 1, -1, -1, bands, gap_open=gap_open)
    same_as(host, plan, ("host", gap_open))
    assert host.cigars() == plan.cigars()
    nocig = aligner.align_batch_anchored(b, 1, -1, -1, bands, gap_open=gap_open, want_cigar=False)
    same_as(nocig, plan, ("host, score only", gap_open))
    assert nocig.arena is None
    one = aligner.align_batch_anchored(b, 1, -1, -1, 16, gap_open=gap_open)  # an int: every pair
    same16, _, _, _, _ = run_anchored(aligner, b, (1, -1, -1), 16, gap_open)
    same_as(one, same16, ("host, one band", gap_open))
    for p in (3, 50, 119):  # the one-pair call agrees with both
        got = A.align_anchored(b.query(p), b.target(p), 1, -1, -1, int(bands[p]), gap_open=gap_open)
        assert got == quad(plan, p) == quad(host, p), (gap_open, p)
        s, cig, qe, te = A.align_anchored(b.query(p), b.target(p), 1, -1, -1, int(bands[p]), gap_open=gap_open,
                                          want_cigar=False)
        assert (s, cig, qe, te) == (got[0], None, got[2], got[3])
    empty = aligner.align_batch_anchored(synth.from_pairs([]), 1, -1, -1, 4)
    assert len(empty.scores) == 0


def test_errors(aligner):
    b = synth.ragged_batch(4, 1, 40, seed=5)
    with pytest.raises(ValueError, match="range"):  # (40 + 40 + 2) * 2^20 >= 2^26
        aligner.align_batch_anchored(b, 1 << 20, -1, -1, 8)
    with pytest.raises(ValueError, match="range"):
        DevicePlan.anchored(aligner, b, 1, -(1 << 20), -1, 8)
    with pytest.raises(ValueError, match="range"):  # |open| + |extend| counts as one step
        A.align_anchored(b"ACGT", b"ACGT", 1, -1, -(1 << 24), 2, gap_open=-(1 << 24))
    with pytest.raises(ValueError, match="range"):
        DevicePlan.anchored(aligner, b, 1, -1, -(1 << 19), 8, gap_open=-(1 << 19))
    with pytest.raises(ValueError):
        DevicePlan.anchored(aligner, b, 1, -1, -1, np.zeros(3, np.uint32))  # one band per pair
    with pytest.raises(ValueError):
        aligner.align_batch_anchored(b, 1, -1, -1, np.zeros(5, np.uint32))
    for flags in (2, 4, 1 << 31, 3):
        with pytest.raises(A.DeviceError, match="flag"):  # TA_ERR_ARG: unknown flag bits
            DevicePlan.anchored(aligner, b, 1, -1, -1, 8, flags=flags)
    plan = DevicePlan.anchored(aligner, b, 1, -1, -1, 8)
    try:
        plan.run()
        with pytest.raises(AttributeError, match="certif"):
            plan.certify()
        with pytest.raises(AttributeError, match="certif"):
            plan.certify_async()
    finally:
        plan.close()
    # the existing entries keep rejecting the internal mode number
    with pytest.raises(ValueError, match="Unknown AlignmentType"):
        aligner.align_batch_banded(b, 3, 1, -1, -1, 8)
    with pytest.raises(ValueError, match="Unknown AlignmentType"):
        aligner.align_batch_banded_affine(b, 3, 1, -1, -3, -1, 8)
    banded = DevicePlan(aligner, b, 0, 1, -1, -1, True, band=8)
    try:
        with pytest.raises(AttributeError, match="anchored"):
            banded.ends()
    finally:
        banded.close()
