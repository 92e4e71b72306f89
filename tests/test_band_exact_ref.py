"""Exact banded alignment on the CPU: the rule of include/team_align_c.h as
tests/band_exact_ref.py restates it, checked with the project's own banded
checkers (tests/banded_ref.py, tests/banded_affine_ref.py) -- every result
certified at its first band, and every second round at the needed band, is the
full-band result; the bindings; and ta_layout.h's band_exact_* functions under
ASan + UBSan (tests/cpp/band_exact_check.cpp, a program of its own)."""
import os
import random
import subprocess

import band_exact_ref as BX
import pytest
from conftest import ROOT

from bioinfo1_amd import align as A
from bioinfo1_amd import mapper as M

CS = os.path.join(ROOT, "bioinfo1_amd", "csrc")
SEED = 0xBA2D
N_PAIRS = 150
W0 = (0, 2, 7, 19)
# (match, mismatch, gap): gap = 0, hs = 0, hs < 0 and mismatch > 0 among them
SCORINGS = [(1, -1, -1), (2, -3, -2), (1, -1, 0), (0, -1, -1), (-1, -2, -1), (2, 1, -2), (3, -2, -4)]
GAP_OPEN = (0, -1, -3, -6)
FLOOR = 100  # per (mode, gap family): certified first rounds, and second rounds below min(n, m)


def related_pairs(seed: int, count: int):
    """Related pairs of 1-200 bp: the target is the query with 0-40 % of its
    bases substituted, inserted or deleted; a third of the pairs get a random
    prefix and / or suffix on either side; a quarter hold '-' bytes."""
    rng = random.Random(seed)
    pairs = []
    for k in range(count):
        n = rng.randint(1, 200) if k % 5 else rng.randint(1, 24)
        q = [rng.choice(b"ACGT") for _ in range(n)]
        rate = rng.choice((0.0, 0.02, 0.05, 0.1, 0.2, 0.4))
        t = []
        for c in q:
            u = rng.random()
            if u < rate / 3:
                t.append(rng.choice(b"ACGT"))
            elif u < 2 * rate / 3:
                t += [c, rng.choice(b"ACGT")]
            elif u >= rate:
                t.append(c)
        if k % 3 == 0:
            extra = [rng.choice(b"ACGT") for _ in range(rng.randint(1, 30))]
            side = rng.randrange(4)
            q, t = ((extra + q, t), (q + extra, t), (q, extra + t), (q, t + extra))[side]
        if k % 4 == 0:
            for s in (q, t):
                for _ in range(rng.randint(0, 4)):
                    if s:
                        s[rng.randrange(len(s))] = ord("-")
        q, t = q[:200], (t or [rng.choice(b"ACGT")])[:200]
        pairs.append((bytes(q), bytes(t)))
    return pairs


def test_certified_and_second_rounds_equal_the_full_band():
    pairs = related_pairs(SEED, N_PAIRS)
    assert all(1 <= len(q) <= 200 and 1 <= len(t) <= 200 for q, t in pairs)
    assert sum(b"-" in q + t for q, t in pairs) >= N_PAIRS // 8
    count = {}
    for k, (q, t) in enumerate(pairs):
        n, m = len(q), len(t)
        ma, mi, gap = SCORINGS[k % len(SCORINGS)]
        for mode in (0, 1, 2):
            for go in (None, GAP_OPEN[(k // len(SCORINGS)) % len(GAP_OPEN)]):
                sc = (ma, mi, go, gap)
                full = BX.banded(q, t, mode, *sc, max(n, m))
                assert BX.banded(q, t, mode, *sc, min(n, m)) == full, (k, mode, sc)  # the full-band clause
                c = count.setdefault((mode, go is None), [0, 0, 0])
                again = {}
                for w0 in W0:
                    first = BX.banded(q, t, mode, *sc, w0)
                    rounds, w = BX.plan(q, t, mode, *sc, w0, first[0])
                    if rounds == 1:
                        assert first == full, (k, mode, sc, w0)
                        c[0] += w < min(n, m)
                    else:
                        assert w > w0
                        if w not in again:
                            again[w] = BX.banded(q, t, mode, *sc, w)
                        assert again[w] == full, (k, mode, sc, w0, w)
                        # the second round is itself certified (two rounds always suffice)
                        assert BX.plan(q, t, mode, *sc, w, again[w][0])[0] == 1
                        c[1] += w < min(n, m)
                        c[2] += w == min(n, m)
    print(count)
    assert len(count) == 6
    for key, (cert, narrow, _) in count.items():
        assert cert >= FLOOR and narrow >= FLOOR, (key, cert, narrow)


def test_positive_gap_is_uncertifiable_and_goes_to_the_full_band():
    q, t = b"ACGTACGTACGTACGTACGT", b"ACGTACGAACGTACGTACGTAC"
    n, m = len(q), len(t)
    for mode in (0, 1, 2):
        for go, ge in ((None, 1), (0, 2), (1, -1), (-1, 1)):
            assert not BX.certifiable(go or 0, ge)
            res, w, rounds = BX.align_exact(q, t, mode, 1, -1, go, ge, 3)
            assert (w, rounds) == (min(n, m), 2)
            assert res == BX.banded(q, t, mode, 1, -1, go, ge, max(n, m))
            assert BX.certify(q, t, mode, 1, -1, go or 0, ge, 3, 10 ** 6) == (0, min(n, m))
            # at the full band it is exact whatever the scoring
            assert BX.certify(q, t, mode, 1, -1, go or 0, ge, min(n, m), -5) == (1, min(n, m))
    assert BX.certify(b"", b"ACGT", 0, 1, -1, 0, -1, 0, -4) == (1, 0)  # a degenerate pair
    assert BX.default_start(100, 3000) == 64 and BX.default_start(32768, 32768) == 2048
    assert BX.default_start(1025, 1025) == 65


# ---- the bindings
def test_abi_symbols_and_argtypes():
    L = A.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert len(A.BAND_EXACT_ABI_SYMBOLS) == 4
    for s in A.BAND_EXACT_ABI_SYMBOLS:
        assert s in exported and s in A.ABI_SYMBOLS, s
        assert getattr(L, s).argtypes, s
    assert len(L.ta_align_batch_banded_exact.argtypes) == len(L.ta_align_batch_banded.argtypes) + 2
    assert len(L.ta_align_batch_banded_affine_exact.argtypes) == len(L.ta_align_batch_banded_affine.argtypes) + 2
    assert len(L.ta_banded_plan_certify.argtypes) == len(L.ta_banded_affine_plan_certify.argtypes) == 5
    for name in ("align_batch_banded_exact", "align_batch_banded_affine_exact"):
        assert callable(getattr(A.Aligner, name))
    assert callable(A.align_banded_exact) and callable(A.DevicePlan.certify)
    assert {"band_used", "rounds"} <= set(A.BatchResult.__dataclass_fields__)
    ML = M.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in ("tm_map_batch_band_exact", "tm_map_files_band_exact"):
        assert s in exported and s in M.ABI_SYMBOLS, s
    assert len(ML.tm_map_batch_band_exact.argtypes) == len(ML.tm_map_batch_x.argtypes) + 1  # the nullable gap open
    assert len(ML.tm_map_files_band_exact.argtypes) == len(ML.tm_map_files_x.argtypes) + 1


def test_python_argument_errors():
    with pytest.raises(ValueError, match="auto"):
        M.Index.map_batch(None, [b"ACGT"], M.Options.make(), band="wide")
    with pytest.raises(ValueError, match="auto"):
        M.map_files("ref.fa", "reads.fa", band="wide")
    with pytest.raises(AttributeError, match="not a banded plan"):
        A.DevicePlan.certify_async(type("P", (), {"banded": False})())


# ---- the rule's two functions under ASan + UBSan, as a program of its own
def test_rule_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "band_exact_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CS,
                           os.path.join(ROOT, "tests", "cpp", "band_exact_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    word, cases, below = r.stdout.split()
    assert word == "ok" and int(cases) >= 3000 and int(below) >= 1000
