"""The classified case table (tests/frame_cases.py) against the host predicates
that choose the packed fills' and the recomputing walk's arithmetic
(tests/cpp/frame_probe.cpp: ta_layout.h, ta_planner.cpp), on the CPU: every
shape's class, every pinned edge, the plan each case's batch gets, and that the
table covers every class the kernels have."""
import os
import subprocess

import pytest
from conftest import ROOT

import frame_cases as fc

CS = os.path.join(ROOT, "bioinfo1_amd", "csrc")
RUN_ARGS = {"ck": (1, 512), "codes": (1, 0), "no_ck": (1, 256), "score": (0, 0)}  # (want_cigar, TA_PLAN_* flags)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_probe") / "frame_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", CS, os.path.join(ROOT, "tests", "cpp", "frame_probe.cpp"),
                           os.path.join(CS, "ta_planner.cpp"), "-o", exe])

    def ask(lines):
        r = subprocess.run([exe], input="".join(" ".join(str(x) for x in ln) + "\n" for ln in lines),
                           capture_output=True, text=True, timeout=120, check=True)
        out = []
        for ln in r.stdout.splitlines():
            out.append({k: int(v) for k, v in (f.split("=") for f in ln.split()[1:])})
        assert len(out) == len(lines), r.stdout
        return out

    return ask


def _mag(sc):
    return max(1, *(abs(x) for x in sc))


def test_table_is_well_formed():
    ids = [c["id"] for c in fc.CASES]
    assert len(set(ids)) == len(ids)
    for c in fc.CASES:
        shapes = fc.pair_shapes(c)
        assert len(shapes) <= 40, c["id"]
        keys = set()
        for n, m, cnt, fill, code, ck in c["shapes"]:
            assert cnt >= 3 and cnt % 2 == 1, (c["id"], n, m)
            assert fill in ("dual", "int32")
            if c["mode"] == fc.LOCAL:
                assert code in (fc.Z, fc.M2) and ck in (fc.EQ, fc.M2), (c["id"], n, m)
                assert cnt <= 4 or n * m <= 1500000, (c["id"], n, m)  # (the oracle's time)
            else:
                assert code is None and ck is None
            key = ((n + 1023) // 1024, n % 16)
            assert key not in keys, (c["id"], n, m)  # left-over pairs never make a flexible couple
            keys.add(key)
        if c["mode"] == fc.LOCAL and c["ck"]:
            assert len(shapes) >= 8 and c["sc"][2] <= 0, c["id"]


def test_shape_classes(probe):
    """Every shape of the table runs in the kernel variant the table says."""
    asks, want = [], []
    for c in fc.CASES:
        for n, m, _, fill, code, ck in c["shapes"]:
            asks.append((c["mode"], *c["sc"], n, m))
            want.append((c, n, m, fill, code, ck))
        for n, m in c.get("ragged", []):
            asks.append((c["mode"], *c["sc"], n, m))
            want.append((c, n, m, "flex", None, None))
    for got, (c, n, m, fill, code, ck) in zip(probe(asks), want):
        where = (c["id"], n, m, got)
        assert bool(got["tab_ok"]) == c["tab"], where
        assert bool(got["flex_fits"]) == (_mag(c["sc"]) <= 6), where
        ma, mi = c["sc"][0], c["sc"][1]
        assert bool(got["local_eq_gains"]) == (-7 <= ma <= 8 and -7 <= mi <= 8), where
        if fill == "flex":  # a ragged pair: the flexible fill and its checkpoints take it
            assert got["flex_fits"] and got["flex_ck_fits"] and (c["mode"] != fc.LOCAL or got["flex_local_fits"]), where
            continue
        assert ("dual" if got["fits_int16"] else "int32") == fill, where
        if c["mode"] == fc.LOCAL:
            assert (fc.Z if got["off_z"] >= 0 else fc.M2) == code, where
            assert (fc.EQ if got["off_eq"] >= 0 else fc.M2) == ck, where
            assert got["off_z"] <= 0x7BFF and got["off_eq"] <= 0x7BFF, where


def test_case_plans(probe):
    """The plan of every case's batch, per run of test_frame_gpu.py: checkpoints where the
    table says so, and as many pairs in the dual and flexible fills as the classes give."""
    asks, want = [], []
    for c in fc.CASES:
        flat = [x for nm in fc.pair_shapes(c) for x in nm]
        for run in fc.RUNS:
            cig, flags = RUN_ARGS[run]
            asks.append(("p", c["mode"], *c["sc"], cig, flags, *flat))
            want.append((c, run))
    for got, (c, run) in zip(probe(asks), want):
        where = (c["id"], run, got)
        assert got["dual_pairs"] - got["flex_pairs"] == fc.dual_fill_pairs(c, run), where
        assert got["flex_pairs"] == fc.flex_fill_pairs(c, run), where
        if run == "ck":
            assert bool(got["ck"] and got["blk"] and got["walk"] == 64) == c["ck"], where
            assert bool(got["ck"]) == c["ck"], where
        else:
            assert not got["ck"], where
        if run == "no_ck" and c["mode"] == fc.LOCAL and all(s[3] == "dual" for s in c["shapes"]) \
                and "ragged" not in c:
            assert got["blk"] and got["walk"] == (64 if c["sc"][2] <= 0 else 0), where  # blocked codes, band walks
        if run == "codes":
            assert not got["blk"], where
        # the walk decodes the pairs order[2k], order[2k + 1] of the plan's cost-sorted order side
        # by side: a shape's odd count leaves its self-coupled pair beside the next shape's first
        assert got["chunks"] == 1, where
        if run == "ck" and c["id"] in ("headline", "mix_frames"):
            assert got["mixed_eq_max2"] >= 1, where
        if run == "ck" and c["id"] == "mix_flex":
            assert got["mixed_eq_flex"] >= 1 and got["mixed_max2_flex"] >= 1, where


def test_edge_plans(probe):
    """test_frame_edge's batches: every pair within the edge in the dual fill (and in a
    checkpoint plan under TA_PLAN_CK where the mode and gap allow), none past it."""
    keys = [(mode, sc, False) for mode in (0, 1, 2) for sc in fc.EDGES[mode]]
    keys += [(mode, fc.RECT_EDGES[mode][0], True) for mode in (0, 1, 2)]
    asks = []
    for mode, sc, rect in keys:
        for shapes in fc.edge_batches(mode, sc, rect):
            for flags in (0, 512):
                asks.append(("p", mode, *sc, 1, flags, *[x for nm in shapes for x in nm]))
    got = iter(probe(asks))
    for mode, sc, rect in keys:
        inside, past = fc.edge_batches(mode, sc, rect)
        for flags in (0, 512):
            g = next(got)
            assert g["dual_pairs"] == len(inside) and g["flex_pairs"] == 0 and g["singles"] == 0, (mode, sc, rect, g)
            if flags:
                assert bool(g["ck"] and g["walk"] == 64) == fc.edge_takes_ck(mode, sc), (mode, sc, rect, g)
        for flags in (0, 512):
            g = next(got)
            assert g["dual_pairs"] == g["flex_pairs"], (mode, sc, rect, g)


def _dual_shapes(sc, mode=fc.LOCAL):
    for c in fc.CASES:
        if c["sc"] == sc and c["mode"] == mode:
            for s in c["shapes"]:
                if s[3] == "dual":
                    yield c, s


def test_required_classes_are_covered():
    """The table holds a dual-fill case of every class the local kernels have."""
    def any_shape(sc, pred, mode=fc.LOCAL):
        return any(pred(c, s) for c, s in _dual_shapes(sc, mode))

    eq_in = lambda sc: -7 <= sc[0] <= 8 and -7 <= sc[1] <= 8  # noqa: E731
    # ck_frame = max3_eq, tab = True: the headline scoring
    assert any_shape((1, -1, -1), lambda c, s: s[5] == fc.EQ and c["tab"] and c["ck"])
    # ck_frame = max2 by score, tab = True
    for sc in ((1, -9, -2), (10, -4, -6)):
        assert not eq_in(sc) and any_shape(sc, lambda c, s: s[5] == fc.M2 and c["tab"] and c["ck"]), sc
    # ck_frame = max2 by shape with gains inside [-7, 8]: the headline at 1900 x 1900 and one more scoring
    assert any_shape((1, -1, -1), lambda c, s: s[:2] == (1900, 1900) and s[5] == fc.M2 and c["ck"])
    assert any(eq_in(c["sc"]) and c["sc"] != (1, -1, -1) and c["ck"] and c["tab"] and s[3] == "dual" and s[5] == fc.M2
               for c in fc.CASES if c["mode"] == fc.LOCAL for s in c["shapes"])
    # tab = False in both checkpoint frames
    assert any_shape((1, -1, -200), lambda c, s: s[5] == fc.EQ and not c["tab"] and c["ck"])
    assert any_shape((1, -130, -1), lambda c, s: s[5] == fc.M2 and not c["tab"] and c["ck"])
    # code_frame = max2 while ck_frame = max3_eq
    assert any_shape((5, -4, -3), lambda c, s: s[4] == fc.M2 and s[5] == fc.EQ and 330 <= s[0] <= 370)
    # the corners of local_eq_gains
    assert any_shape((8, -7, -1), lambda c, s: s[5] == fc.EQ and c["ck"])
    assert any_shape((9, -1, -1), lambda c, s: s[5] == fc.M2 and c["ck"])
    assert any_shape((1, -8, -1), lambda c, s: s[5] == fc.M2 and c["ck"])
    # a non-positive match, mismatch above match
    for sc in ((-2, -3, -1), (0, -1, -1), (3, 4, 0)):
        assert any_shape(sc, lambda c, s: c["ck"]), sc
    # a positive gap: local takes no checkpoints, global and semi do
    assert any_shape((2, -1, 2), lambda c, s: not c["ck"])
    assert any_shape((2, -1, 2), lambda c, s: c["ck"], fc.GLOBAL) and any_shape((2, -1, 2), lambda c, s: c["ck"], fc.SEMI)
    # both frames inside one checkpoint plan, and one of them beside flexible couples
    for cid in ("mix_frames", "mix_flex"):
        c = next(c for c in fc.CASES if c["id"] == cid)
        assert c["ck"] and {s[5] for s in c["shapes"]} == {fc.EQ, fc.M2}, cid
    assert next(c for c in fc.CASES if c["id"] == "mix_flex")["ragged"]
    # a pair past fits_int16
    assert any(s[3] == "int32" for c in fc.CASES for s in c["shapes"])
    # every scoring of the table is one the edge tables speak of
    assert {c["sc"] for c in fc.CASES} <= set(fc.SCORINGS)


def test_edges(probe):
    """The pinned edges: the largest admitted squares of fits_int16 per mode (those up to
    EDGE_CAP exactly, L x L and (L - 1) x L in, (L + 1) x (L + 1) out), of the two local
    frames, and the two-pass rectangular edges."""
    asks = [(mode, *sc, 20000) for mode in (0, 1, 2) for sc in fc.SCORINGS]
    got = probe(asks)
    at, at_want = [], []
    for (mode, *sc, _), g in zip(asks, got):
        sc = tuple(sc)
        L = g["fits_int16"]
        assert fc.EDGES[mode].get(sc) == (L if L <= fc.EDGE_CAP else None), (mode, sc, L)
        if mode == fc.LOCAL:
            assert fc.LOCAL_FRAME_EDGES[sc] == (g["max3_eq"], g["max3_z"]), (sc, g)
        if L <= fc.EDGE_CAP:
            for n, m, fits in ((L, L, 1), (L - 1, L, 1), (L + 1, L + 1, 0)):
                at.append((mode, *sc, n, m))
                at_want.append(fits)
    for mode, (sc, m) in fc.RECT_EDGES.items():
        g, = probe([("m", mode, *sc, fc.RECT_N, 20000)])
        assert g["fits_int16"] == m, (mode, sc, g)
        at += [(mode, *sc, fc.RECT_N, m), (mode, *sc, fc.RECT_N, m + 1)]
        at_want += [1, 0]
    for a, g, w in zip(at, probe(at), at_want):
        assert g["fits_int16"] == w, (a, g)
    assert set(fc.LOCAL_FRAME_EDGES) == set(fc.SCORINGS)
