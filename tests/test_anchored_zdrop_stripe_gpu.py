"""The row-stripe z-drop rule on the GPU (ta_anchored_plan_create_zdrop_rule,
ta_align_batch_anchored_zdrop_rule with TA_ZDROP_STRIPE) against its definition
in tests/anchored_zdrop_stripe_ref.py: score, ends, CIGAR bytes and swept_steps
-- the exact number of fill steps each pair executed -- on the directed cases
(tests/anchored_zdrop_stripe_cases.py) and on seeded batches of dying ends, in
both gap families, with CIGAR and score-only; the band-caveat pair, which the
stripe plan must leave whole where the segment plan clips it; the host batch,
ends / annotate / swept_steps after the fills alone, chunks, the affine kernels
at gap_open == 0, and the errors."""
import ctypes as C

import anchored_zdrop_ref as ZR
import anchored_zdrop_stripe_cases as SC
import anchored_zdrop_stripe_ref as SR
import annotate_ref as R
import numpy as np
import pytest

from bioinfo1_amd import align as A
from bioinfo1_amd import synth
from bioinfo1_amd.align import Aligner, DevicePlan

pytestmark = pytest.mark.gpu

S244 = (2, -4, -4)
GAP_OPEN = -3


@pytest.fixture(scope="module")
def aligner():
    return Aligner(0)


def run_plan(aligner, batch, sc, band, z, gap_open=0, want_cigar=True, budget=0, flags=0, rule="stripe"):
    """-> (BatchResult with ends and swept_steps, chunks, workspace bytes)."""
    plan = DevicePlan.anchored(aligner, batch, *sc, band, gap_open=gap_open, want_cigar=want_cigar,
                               workspace_budget=budget, flags=flags, zdrop=z, zdrop_rule=rule)
    try:
        plan.run()
        res = plan.results()
        res.query_ends, res.target_ends = plan.ends()
        res.swept_steps = plan.swept_steps() if z is not None else None
        return res, plan.chunks, plan.workspace_bytes
    finally:
        plan.close()


def five(res, p):
    return (int(res.scores[p]), res.cigar(p), int(res.query_ends[p]), int(res.target_ends[p]),
            None if res.swept_steps is None else int(res.swept_steps[p]))


def same_as(res, want, tag):
    np.testing.assert_array_equal(res.scores, want.scores, err_msg=str(tag))
    np.testing.assert_array_equal(res.query_ends, want.query_ends, err_msg=str(tag))
    np.testing.assert_array_equal(res.target_ends, want.target_ends, err_msg=str(tag))
    if res.swept_steps is not None and want.swept_steps is not None:
        np.testing.assert_array_equal(res.swept_steps, want.swept_steps, err_msg=str(tag))
    if res.arena is not None and want.arena is not None:
        for p, (a, b) in enumerate(zip(res.cigars(), want.cigars())):
            assert a == b, (tag, p, a, b)


# ---- 1. the directed cases: one plan per case list, every pair with its own band; Z differs between the
# cases, so the cases are grouped by Z
@pytest.mark.parametrize("want_cigar", [True, False], ids=["cigar", "score-only"])
@pytest.mark.parametrize("cases", [SC.LINEAR, SC.AFFINE], ids=["linear", "affine"])
def test_directed_cases(aligner, cases, want_cigar):
    drops = 0
    by_z = {}
    for c in cases:
        by_z.setdefault((c.z, c.scoring, c.gap_open), []).append(c)
    for (z, scoring, gap_open), group in by_z.items():
        batch = synth.from_pairs([(c.q, c.t) for c in group])
        bands = np.array([c.w for c in group], np.uint32)
        res, _, _ = run_plan(aligner, batch, scoring, bands, z, 0 if gap_open is None else gap_open, want_cigar)
        for p, c in enumerate(group):
            want = SR.align_full(c.q, c.t, *c.scoring, c.w, c.gap_open, c.z)
            assert want.drop == c.drop, c.name  # (pinned on the CPU by tests/test_anchored_zdrop_stripe_ref.py)
            exp = (want.score, want.cigar if want_cigar else None, want.gi, want.gj, want.swept_steps)
            assert five(res, p) == exp, (c.name, five(res, p), exp)
            drops += c.drop is not None
    assert drops >= 15


# ---- 2. seeded batches of dying ends
FUZZ = [(S244, 40), (S244, 10), ((2, -3, -2), 0)]
FUZZ_SEEDS = [0x2E40, 0x2E41, 0x2E42]
BANDS = (0, 5, 16, 33, 64)
_fuzz = {}


def fuzz_batch(k):
    """14 pairs: 11 of 40-700 rows and 3 of 1,030-1,400, bands 0 / 5 / 16 / 33 / 64 in turn, a related
    prefix of random length then unrelated bases; '-' bytes in some."""
    if k in _fuzz:
        return _fuzz[k]
    rng = np.random.default_rng(FUZZ_SEEDS[k])
    pairs, bands = [], []
    for x in range(14):
        n = int(rng.integers(1030, 1401)) if x < 3 else int(rng.integers(40, 701))
        m = max(1, n + int(rng.integers(-20, 21)))
        lim = min(n, m)
        L = lim if x % 5 == 4 else int(rng.integers(0, lim + 1))  # (every 5th related to the end)
        c = synth.related_batch(1, max(L, 1), max(L, 1), seed=FUZZ_SEEDS[k] * 64 + x, rate=0.05)
        u = synth.uniform_batch(1, max(n - L, 1), max(m - L, 1), seed=FUZZ_SEEDS[k] * 64 + 32 + x)
        q = bytearray(c.query(0)[:L] + u.query(0)[:n - L])
        t = bytearray(c.target(0)[:L] + u.target(0)[:m - L])
        if x % 3 == 1:
            q[7] = t[11] = ord("-")
            q[len(q) // 2] = ord("-")
        pairs.append((bytes(q), bytes(t)))
        bands.append(BANDS[x % 5])
    _fuzz[k] = (synth.from_pairs(pairs), np.array(bands, np.uint32), {})
    return _fuzz[k]


def fuzz_fills(k, gap_open):
    """The definition's cell values of batch k, computed once per gap family."""
    batch, bands, cache = fuzz_batch(k)
    sc = FUZZ[k][0]
    if gap_open not in cache:
        gap = sc[2] if not gap_open else -1
        cache[gap_open] = [SR.fill(batch.query(p), batch.target(p), sc[0], sc[1], gap, int(bands[p]),
                                   gap_open=gap_open if gap_open else None) for p in range(batch.n_pairs)]
    return cache[gap_open]


def fuzz_sc(k, gap_open):
    sc = FUZZ[k][0]
    return sc if not gap_open else (sc[0], sc[1], -1)


@pytest.mark.parametrize("gap_open", [0, GAP_OPEN], ids=["linear", "affine"])
@pytest.mark.parametrize("k", range(len(FUZZ)))
def test_fuzz_batches(aligner, k, gap_open):
    batch, bands, _ = fuzz_batch(k)
    sc, z = fuzz_sc(k, gap_open), FUZZ[k][1]
    fills = fuzz_fills(k, gap_open)
    want = [SR.result(f, z) for f in fills]
    dropped = sum(w.drop is not None for w in want)
    print("fuzz", k, sc, "Z", z, "gap_open", gap_open, "drops", dropped, "of", len(want),
          "steps", sum(w.swept_steps for w in want), "of", sum(SR.total_steps(f.n, f.m, f.w) for f in fills))
    assert 4 * dropped >= len(want), (k, gap_open, dropped)
    res, _, _ = run_plan(aligner, batch, sc, bands, z, gap_open)
    for p, w in enumerate(want):
        exp = (w.score, w.cigar, w.gi, w.gj, w.swept_steps)
        assert five(res, p) == exp, (k, gap_open, p, int(batch.qlen[p]), int(batch.tlen[p]), int(bands[p]),
                                     five(res, p), exp, w.drop)
    nocig, _, _ = run_plan(aligner, batch, sc, bands, z, gap_open, want_cigar=False)
    assert nocig.arena is None
    same_as(nocig, res, ("score only", k, gap_open))


# ---- 3. the band caveat: a live two-pass end stays whole under the stripe rule
def caveat_pair(w, n=2000):
    """The band-caveat pair of tests/test_anchored_zdrop_ref.py: every 10th base substituted, m = n + w."""
    q = synth.uniform_batch(1, n, 1, seed=0x2D61).query(0)
    sub = bytearray(q)
    for k in range(4, n, 10):
        sub[k] = {65: 67, 67: 71, 71: 84, 84: 65}[sub[k]]
    return q, bytes(sub) + synth.uniform_batch(1, 1, w, seed=5).target(0)


@pytest.mark.parametrize("gap_open", [0, GAP_OPEN], ids=["linear", "affine"])
def test_the_caveat_pair_is_whole_under_the_stripe_rule_and_clipped_under_the_segment_rule(aligner, gap_open):
    ws = (64, 128)
    pairs = [caveat_pair(w) for w in ws]
    batch, bands = synth.from_pairs(pairs), np.array(ws, np.uint32)
    sc = S244 if not gap_open else (2, -4, -1)
    plain = aligner.align_batch_anchored(batch, *sc, bands, gap_open=gap_open)
    assert [int(e) for e in plain.query_ends] == [2000, 2000]
    if not gap_open:
        assert [int(s) for s in plain.scores] == [2800, 2800]
    total = [SR.total_steps(2000, 2000 + w, w) for w in ws]
    fills = [ZR.fill(q, t, *sc, w, gap_open if gap_open else None) for (q, t), w in zip(pairs, ws)]
    for z in (0, 40, 100):
        for want_cigar in (True, False):
            stripe, _, _ = run_plan(aligner, batch, sc, bands, z, gap_open, want_cigar)
            same_as(stripe, plain, ("stripe", z, want_cigar))
            assert [int(s) for s in stripe.swept_steps] == total
        seg, _, _ = run_plan(aligner, batch, sc, bands, z, gap_open, rule="segment")
        ref = [ZR.result(f, z) for f in fills]
        assert [five(seg, p) for p in range(2)] == [(r.score, r.cigar, r.gi, r.gj, r.swept_steps) for r in ref]
        if not gap_open or z < 100:  # (affine ends fall by 1 a step: at Z = 100, w = 64 the tail segment holds)
            assert [int(e) for e in seg.query_ends] == [1024, 1024], z  # clipped at the pass boundary
            assert all(int(a) < int(b) for a, b in zip(seg.scores, plain.scores))
    host = aligner.align_batch_anchored(batch, *sc, bands, gap_open=gap_open, zdrop=40, zdrop_rule="stripe")
    same_as(host, plain, "host")
    assert host.cigars() == plain.cigars() and [int(s) for s in host.swept_steps] == total


# ---- 4. the host batch, and ends / annotate / swept_steps
@pytest.mark.parametrize("gap_open", [0, GAP_OPEN], ids=["linear", "affine"])
def test_host_batch_equals_the_plan(aligner, gap_open):
    batch, bands, _ = fuzz_batch(1)
    sc, z = fuzz_sc(1, gap_open), FUZZ[1][1]
    plan, _, _ = run_plan(aligner, batch, sc, bands, z, gap_open)
    host = aligner.align_batch_anchored(batch, *sc, bands, gap_open=gap_open, zdrop=z, zdrop_rule="stripe")
    same_as(host, plan, ("host", gap_open))
    assert host.cigars() == plan.cigars()
    nocig = aligner.align_batch_anchored(batch, *sc, bands, gap_open=gap_open, want_cigar=False, zdrop=z,
                                         zdrop_rule="stripe")
    same_as(nocig, plan, ("host, score only", gap_open))
    assert nocig.arena is None
    for p in (0, 5, 13):  # the one-pair call
        got = A.align_anchored(batch.query(p), batch.target(p), *sc, int(bands[p]), gap_open=gap_open, zdrop=z,
                               zdrop_rule="stripe")
        assert got == five(plan, p)[:4], (gap_open, p)
    # z-drop off: the rule is not looked at, the results are plain anchored's
    off = aligner.align_batch_anchored(batch, *sc, bands, gap_open=gap_open, zdrop_rule="stripe")
    plain = aligner.align_batch_anchored(batch, *sc, bands, gap_open=gap_open)
    same_as(off, plain, "off")
    assert off.swept_steps is None and off.cigars() == plain.cigars()
    # the default rule is the segment rule, through either entry
    seg = aligner.align_batch_anchored(batch, *sc, bands, gap_open=gap_open, zdrop=z)
    seg2 = aligner.align_batch_anchored(batch, *sc, bands, gap_open=gap_open, zdrop=z, zdrop_rule="segment")
    same_as(seg2, seg, "segment")
    empty = aligner.align_batch_anchored(synth.from_pairs([]), *sc, 4, zdrop=z, zdrop_rule="stripe")
    assert len(empty.scores) == 0 and len(empty.swept_steps) == 0
    deg = aligner.align_batch_anchored(synth.from_pairs([(b"", b"ACGT"), (b"ACGT", b""), (b"", b"")]), *sc, 4,
                                       gap_open=gap_open, zdrop=z, zdrop_rule="stripe")
    assert [five(deg, p) for p in range(3)] == [(0, b"1\0", 0, 0, 0)] * 3


@pytest.mark.parametrize("gap_open", [0, GAP_OPEN], ids=["linear", "affine"])
@pytest.mark.parametrize("want_cigar", [True, False], ids=["cigar", "score-only"])
def test_ends_and_swept_steps_after_the_fills_alone(aligner, gap_open, want_cigar):
    batch, bands, _ = fuzz_batch(0)
    sc, z = fuzz_sc(0, gap_open), FUZZ[0][1]
    want = [SR.result(f, z) for f in fuzz_fills(0, gap_open)]
    plan = DevicePlan.anchored(aligner, batch, *sc, bands, gap_open=gap_open, want_cigar=want_cigar, zdrop=z,
                               zdrop_rule="stripe")
    try:
        for c in range(plan.chunks):
            plan.run_fill(c)
        steps = plan.swept_steps()
        qe, te = plan.ends()
        plan.check()
        assert [int(s) for s in steps] == [w.swept_steps for w in want]
        assert [(int(a), int(b)) for a, b in zip(qe, te)] == [(w.gi, w.gj) for w in want]
        assert plan.pair_chunks().max() < plan.chunks
    finally:
        plan.close()


@pytest.mark.parametrize("gap_open", [0, GAP_OPEN], ids=["linear", "affine"])
def test_annotate(aligner, gap_open):
    batch, bands, _ = fuzz_batch(2)
    sc, z = fuzz_sc(2, gap_open), FUZZ[2][1]
    want = [SR.result(f, z) for f in fuzz_fills(2, gap_open)]
    plan = DevicePlan.anchored(aligner, batch, *sc, bands, gap_open=gap_open, zdrop=z, zdrop_rule="stripe")
    try:
        plan.run()
        plan.annotate(eqx=True)
        ann = plan.annotation()
    finally:
        plan.close()
    moved = 0
    for p, w in enumerate(want):
        q, t = batch.query(p), batch.target(p)
        info, eqx = R.expected(q[:w.gi], t[:w.gj], R.GLOBAL, w.cigar, w.gi, w.gj)
        got = {f: int(ann.info[f][p]) for f in R.FIELDS}
        assert got == info, (gap_open, p, w.cigar, got, info)
        assert ann.eqx(p) == eqx, (gap_open, p)
        moved += w.gi > 0
    assert moved >= 6


# ---- 5. chunks
@pytest.mark.parametrize("gap_open", [0, GAP_OPEN], ids=["linear", "affine"])
def test_multi_chunk_plans_give_the_same_results(aligner, gap_open):
    batch, bands, _ = fuzz_batch(0)
    sc, z = fuzz_sc(0, gap_open), FUZZ[0][1]
    one, chunks, ws = run_plan(aligner, batch, sc, bands, z, gap_open)
    assert chunks == 1
    seg, _, ws_seg = run_plan(aligner, batch, sc, bands, z, gap_open, rule="segment")
    assert ws == ws_seg  # planned as the segment rule's plan
    many, nch, ws_c = run_plan(aligner, batch, sc, bands, z, gap_open, budget=max(ws // 4, 1))
    assert nch >= 3 and ws_c < ws
    same_as(many, one, ("chunks", gap_open))
    want = [SR.result(f, z) for f in fuzz_fills(0, gap_open)]
    assert [five(many, p) for p in range(batch.n_pairs)] == [(w.score, w.cigar, w.gi, w.gj, w.swept_steps) for w in want]


# ---- 6. the affine kernels at gap_open == 0
def test_affine_kernels_at_gap_open_0_equal_the_linear_plan(aligner):
    for k in (0, 2):
        batch, bands, _ = fuzz_batch(k)
        sc, z = FUZZ[k]
        lin, _, ws = run_plan(aligner, batch, sc, bands, z)
        aff, _, ws_aff = run_plan(aligner, batch, sc, bands, z, flags=A.TA_ANCHORED_AFFINE_KERNELS)
        same_as(aff, lin, ("gap_open 0", k))
        assert ws_aff > ws  # 8-byte code entries: the other kernels ran
        assert sum(int(s) for s in lin.swept_steps) < sum(
            SR.total_steps(int(batch.qlen[p]), int(batch.tlen[p]), int(bands[p])) for p in range(batch.n_pairs))
        nocig, _, _ = run_plan(aligner, batch, sc, bands, z, flags=A.TA_ANCHORED_AFFINE_KERNELS, want_cigar=False)
        same_as(nocig, lin, ("gap_open 0, score only", k))


# ---- 7. the errors
def test_errors(aligner):
    b = synth.from_pairs([(b"ACGTACGT", b"ACGTACGT"), (b"ACGT", b"ACTT")])
    plan = DevicePlan.anchored(aligner, b, *S244, 4, zdrop=5, zdrop_rule="stripe")
    try:
        plan.run()
        with pytest.raises(AttributeError, match="certif"):
            plan.certify()
        assert [int(s) for s in plan.swept_steps()] == [8, 4]
    finally:
        plan.close()
    off = DevicePlan.anchored(aligner, b, *S244, 4, zdrop_rule="stripe")  # z-drop off, whatever the rule
    try:
        off.run()
        with pytest.raises(AttributeError, match="z-drop"):
            off.swept_steps()
    finally:
        off.close()
    for rule in ("Stripe", "rows", 1, None):
        with pytest.raises(ValueError, match="zdrop_rule"):
            DevicePlan.anchored(aligner, b, *S244, 4, zdrop=5, zdrop_rule=rule)
        with pytest.raises(ValueError, match="zdrop_rule"):
            aligner.align_batch_anchored(b, *S244, 4, zdrop=5, zdrop_rule=rule)
    with pytest.raises(ValueError, match="zdrop"):
        DevicePlan.anchored(aligner, b, *S244, 4, zdrop=-1, zdrop_rule="stripe")
    with pytest.raises(ValueError, match="range"):
        aligner.align_batch_anchored(b, 1 << 23, -1, -1, 4, zdrop=3, zdrop_rule="stripe")
    # the C entries: a rule outside {0, 1} is TA_ERR_ARG, with z-drop on or off; unknown flag bits stay refused
    L = A.lib()
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    band = np.full(2, 4, np.uint32)
    for rule in (2, -1, 7):
        for z in (5, -1):
            h = C.c_void_p()
            r = L.ta_anchored_plan_create_zdrop_rule(aligner.handle, 2, u32(b.qlen), u32(b.tlen), u32(band), 2, -4, 0, -4,
                                                     1, 0, 0, z, rule, C.byref(h))
            assert r == A.TA_ERR_ARG and not h.value, (rule, z)
    h = C.c_void_p()
    assert L.ta_anchored_plan_create_zdrop_rule(aligner.handle, 2, u32(b.qlen), u32(b.tlen), u32(band), 2, -4, 0, -4, 1,
                                                0, 2, 5, A.TA_ZDROP_STRIPE, C.byref(h)) == A.TA_ERR_ARG
    sc = np.zeros(2, np.int32)
    r = L.ta_align_batch_anchored_zdrop_rule(
        aligner.handle, 2, b.qbytes.ctypes.data, b.qoff.ctypes.data_as(C.POINTER(C.c_uint64)), u32(b.qlen),
        b.tbytes.ctypes.data, b.toff.ctypes.data_as(C.POINTER(C.c_uint64)), u32(b.tlen), u32(band), 2, -4, 0, -4, 0,
        sc.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, 0, None, None, 5, 2, None)
    assert r == A.TA_ERR_ARG
