"""The affine edge table (tests/affine_frame_cases.py) against the host code
that routes pairs into the packed affine fill (tests/cpp/frame_probe.cpp:
ta_planner.cpp affine_fits_int16 and build_affine_plan), on the CPU: every
pinned edge is admitted and the shape one past it refused, the batches of
tests/test_affine_frame_gpu.py plan as couples within the edge and as singles
past it, and the entries marked tight really reach the int16 bound by the
definition's closed forms.  Also the linear twin of the 16-bit goal column
(fits_int16) and, with the oracle, where the goals of the last-lane sweep and
of the long-column cases lie."""
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import affine_frame_cases as ac
import affine_frame_inputs as ai

CS = os.path.join(ROOT, "bioinfo1_amd", "csrc")
ASPECT_LINE = {"square": lambda n, m: ("e",), "wide17": lambda n, m: ("w", n), "wide1030": lambda n, m: ("w", n),
               "tall64": lambda n, m: ("t", m)}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("affine_frame_probe") / "frame_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", CS, os.path.join(ROOT, "tests", "cpp", "frame_probe.cpp"),
                           os.path.join(CS, "ta_planner.cpp"), "-o", exe])

    def ask(lines):
        r = subprocess.run([exe], input="".join(" ".join(str(x) for x in ln) + "\n" for ln in lines),
                           capture_output=True, text=True, timeout=120, check=True)
        out = [{k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])} for ln in r.stdout.splitlines()]
        assert len(out) == len(lines), r.stdout
        return out

    return ask


@pytest.fixture(scope="module")
def oracle():
    from oracle.pyoracle import Oracle

    return Oracle()


def _edge_line(key, cap):
    mode, sc, aspect = key
    n, m = (ac.EDGES[key][:2] if key in ac.EDGES else
            {"square": (0, 0), "wide17": (ac.WIDE_N, 0), "wide1030": (ac.TWO_PASS_N, 0), "tall64": (0, ac.TALL_M)}[aspect])
    head = ASPECT_LINE[aspect](n, m)
    return (head[0], mode, *sc, *head[1:], cap)


def test_table_is_well_formed():
    assert ac.PAIRS_PER_SHAPE % 2 == 0 and ac.NV_PAIRS % 2 == 0
    for key, (n, m, kind) in ac.EDGES.items():
        mode, sc, aspect = key
        assert mode in (ac.GLOBAL, ac.SEMI) and kind in (ac.T, ac.L), key
        assert {"square": n == m, "wide17": n == ac.WIDE_N, "wide1030": n == ac.TWO_PASS_N,
                "tall64": m == ac.TALL_M}[aspect], key
        assert n * m <= 16_000_000, key  # (the oracle's time: 18 pairs a case)
    # every n mod 16, as a one-pass query and as the last pass of a two-pass query
    assert {(n > 1024, n % 16) for n, _ in ac.NV_SHAPES} == {(p, r) for p in (False, True) for r in range(16)}
    assert all((n <= 1024 and n > 16) or 1024 < n <= 2048 for n, _ in ac.NV_SHAPES)
    assert len(ac.LONG_ENDS) == 4 and sorted(ac.LONG_ENDS) == [300, 300, 65990, 65990]
    for _, _, n, m in ac.LONG_COLUMNS + ac.LONG_ROW_GOALS:
        assert n == 17 and max(ac.LONG_ENDS) + 17 < m and m > ac.COLUMN_CAP + 17


def test_edges(probe):
    """Every pinned edge is the largest shape of its aspect the predicate admits (the
    probe searches down from well above it), the shape itself and the shape one row
    shorter are admitted, the shape one past it is refused, and no admitted shape has
    64 passes or more."""
    keys = list(ac.EDGE_KEYS)
    caps = [max(20000, 3 * max(ac.EDGES[k][:2])) for k in keys]
    got = probe([_edge_line(k, c) for k, c in zip(keys, caps)])
    for key, g in zip(keys, got):
        n, m, _ = ac.EDGES[key]
        assert g["edge"] == {"square": n, "wide17": m, "wide1030": m, "tall64": n}[key[2]], (key, g)
    at, want = [], []
    for key in keys:
        mode, sc, _ = key
        n, m, _ = ac.EDGES[key]
        for (a, b), w in (((n, m), 1), ((n - 1, m), 1), (ac.past_shape(key), 0)):
            at.append(("a", mode, *sc, a, b))
            want.append(w)
    for a, g, w in zip(at, probe(at), want):
        assert g["fits"] == w, (a, g)
        assert not w or g["passes"] < 64, (a, g)
    cpu = list(ac.CPU_EDGES)
    for key, g in zip(cpu, probe([_edge_line(k, ac.CPU_EDGES[k][1]) for k in cpu])):
        assert g["edge"] == ac.CPU_EDGES[key][0], (key, g)
    # the tallest admitted shape of the table: 32 passes
    g, = probe([("t", ac.SEMI, 1, -1, -2, -1, ac.TALL_M, 70000)])
    assert (g["edge"], g["passes"]) == (31915, 32), g


def test_edge_plans(probe):
    """test_affine_edge's batches: all couples within the edge, no couple past it, with
    and without a CIGAR; TA_PLAN_INT32_ONLY (flags 1) makes every pair a single."""
    asks = []
    for key in ac.EDGE_KEYS:
        mode, sc, aspect = key
        for shapes in ac.edge_batches(mode, sc, aspect):
            flat = [x for nm in shapes for x in nm]
            asks += [("q", mode, *sc, 1, 0, *flat), ("q", mode, *sc, 0, 0, *flat), ("q", mode, *sc, 1, 1, *flat)]
    got = iter(probe(asks))
    for key in ac.EDGE_KEYS:
        inside, past = ac.edge_batches(*key)
        assert len(inside) == 2 * ac.PAIRS_PER_SHAPE and len(past) == ac.PAIRS_PER_SHAPE
        for shapes, within in ((inside, True), (past, False)):
            for cig in (1, 0):
                g = next(got)
                if within:
                    assert g["dual_pairs"] == len(shapes) and g["singles"] == 0, (key, cig, g)
                else:
                    assert g["dual_pairs"] == 0 and g["singles"] == len(shapes), (key, cig, g)
            g = next(got)
            assert g["dual_pairs"] == 0 and g["singles"] == len(shapes), (key, "int32", g)


def test_edges_reach_the_bound():
    """The condition on the table: by the closed forms of the definition (row 0, column 0
    with its padding rows and the -K stand-ins, the diagonal, semi row n), every entry
    marked tight holds a stored value within 1,000 of the predicate's bound, at the edge
    shape; the loose ones do not (they stay for the routing only)."""
    for key in ac.EDGE_KEYS:
        mode, sc, _ = key
        n, m, kind = ac.EDGES[key]
        s, what = ac.reach(mode, sc, n, m)
        print("affine_edge_reach %-36s %5d x %-5d %-5s S = %6d (%s)" % (ac.edge_id(key), n, m, kind, s, what))
        assert abs(s) <= 32000, key  # (the closed forms lie inside the predicate's bound)
        assert (abs(s) >= ac.TIGHT_REACH) == (kind == ac.T), (key, s, what)
    tight = [k for k in ac.EDGE_KEYS if ac.EDGES[k][2] == ac.T]
    assert {k[0] for k in tight} == {ac.GLOBAL, ac.SEMI}
    assert {k[2] for k in tight} == {"square", "wide17", "wide1030", "tall64"}
    # both ends of the range, and the row-n values that semi keeps packed (the tall entries)
    assert {ac.reach(k[0], k[1], *ac.EDGES[k][:2])[0] > 0 for k in tight} == {True, False}
    for k in tight:
        if k[0] == ac.SEMI and k[2] == "tall64":
            rown = max(s for s, what in ac.reach_all(k[0], k[1], *ac.EDGES[k][:2]) if what == "row n")
            print("affine_edge_reach %-36s row n S = %6d" % (ac.edge_id(k), rown))
            assert rown >= ac.TIGHT_REACH, k


def test_goal_column_cap(probe):
    """The semi-global packed fills carry the column of row n's best in 16 bits: no semi
    couple with m > 65,535 in either family, whatever the scoring (global couples have no
    goal column and are not capped: CPU_EDGES, test_edges)."""
    cap = ac.COLUMN_CAP
    asks, want = [], []
    for sc, lin, n, m in ac.LONG_COLUMNS + ac.LONG_ROW_GOALS:
        for mm, w in ((cap, 1), (cap + 1, 0), (m, 0)):
            asks.append(("a", ac.SEMI, *sc, n, mm))
            want.append(("fits", w))
            if lin is not None:
                asks.append((ac.SEMI, *lin, n, mm))
                want.append(("fits_int16", w))
    for a, g, (k, w) in zip(asks, probe(asks), want):
        assert g[k] == w, (a, g)
    # the long-column batches: no packed couple of equal shapes in either family
    for sc, lin, n, m in ac.LONG_COLUMNS + ac.LONG_ROW_GOALS:
        g, = probe([("q", ac.SEMI, *sc, 1, 0, *([n, m] * 4))])
        assert g["dual_pairs"] == 0 and g["singles"] == 4, (sc, g)
        if lin is not None:
            g, = probe([("p", ac.SEMI, *lin, 1, 0, *([n, m] * 4))])
            assert g["dual_pairs"] == g["flex_pairs"], (lin, g)  # (flexible couples keep the column in 32 bits)


def test_nv_sweep_plans(probe):
    """The last-lane sweep's batches plan as couples only, in both families."""
    flat = [x for nm in ac.NV_SHAPES for x in nm * ac.NV_PAIRS]
    P = len(ac.NV_SHAPES) * ac.NV_PAIRS
    for cig in (1, 0):
        g, = probe([("q", ac.SEMI, *ai.NV_AFFINE_SC, cig, 0, *flat)])
        assert g["dual_pairs"] == P and g["singles"] == 0, g
        for mode in (1, 2):
            g, = probe([("p", mode, *ai.NV_LINEAR_SC, cig, 0, *flat)])
            assert g["dual_pairs"] == P and g["flex_pairs"] == 0 and g["singles"] == 0, (mode, g)


def _goals(res, batch):
    """Per pair of a semi-global oracle result, 'row' (the goal lies in row n at a column
    below m: the CIGAR ends in an I run that the goal rule appended), 'col' (column m at a
    row below n: a trailing D run) or 'corner'."""
    out = []
    for p in range(batch.n_pairs):
        c = res.cigar(p)
        out.append("row" if c.endswith(b"I") else "col" if c.endswith(b"D") else "corner")
    return out


@pytest.mark.parametrize("alpha", sorted(ai.NV_ALPHABETS))
def test_nv_sweep_goals(oracle, alpha):
    """On the CPU first: by the oracle's goal cell, at least a quarter of the sweep's pairs
    end in row n at an interior column and at least a quarter in column m, per alphabet --
    for the affine and for the linear scoring."""
    b = ai.nv_batch(alpha)
    for name, want in (("affine", oracle.align_affine_batch(b, ac.SEMI, *ai.NV_AFFINE_SC, True)),
                       ("linear", oracle.align_batch(b, ac.SEMI, *ai.NV_LINEAR_SC, True))):
        g = _goals(want, b)
        print(f"nv_sweep_goals {alpha} {name}: row n {g.count('row')}, column m {g.count('col')}, of {len(g)}")
        assert 4 * g.count("row") >= len(g) and 4 * g.count("col") >= len(g), (alpha, name, g)


def test_long_column_goals(oracle):
    """Where the oracle puts the goals of the long-column cases.  LONG_COLUMNS (match ==
    extend <= 0, nothing scores above 0): H(0, m) = 0 is found first in column m and row n
    never beats it strictly -- the goal is (0, m), no column is reported.  LONG_ROW_GOALS
    (a positive mismatch): the goal is row n at the occurrence's end, past 65,535 in two
    pairs of four."""
    for sc, lin, n, m in ac.LONG_COLUMNS:
        b = ai.long_batch(sc, n, m)
        want = oracle.align_affine_batch(b, ac.SEMI, *sc, True)
        assert [want.cigar(p) for p in range(4)] == [b"%dI%dD" % (m, n)] * 4 and not want.scores.any(), sc
        if lin is not None:
            wl = oracle.align_batch(b, ac.SEMI, *lin, True)
            assert not wl.scores.any(), lin
    for sc, lin, n, m in ac.LONG_ROW_GOALS:
        b = ai.long_batch(sc, n, m)
        res = [oracle.align_affine_batch(b, ac.SEMI, *sc, True)]
        if lin is not None:
            res.append(oracle.align_batch(b, ac.SEMI, *lin, True))
        for want in res:
            np.testing.assert_array_equal(want.scores, [n * sc[1]] * 4)
            for p, end in enumerate(ac.LONG_ENDS):
                assert want.cigar(p) == b"%dI%dM%dI" % (end - n, n, m - end), (sc, p, want.cigar(p)[:40])
