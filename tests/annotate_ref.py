"""Test-side reference for the annotate pass (TEST INFRASTRUCTURE ONLY).

``goal()`` is a small DP of its own (tests/annotate_dp.c, compiled here with
the system C compiler) that returns a pair's score and goal cell by the
reference's rule; ``expected()`` expands a CIGAR -- the oracle's -- over the
two sequences in plain Python and returns the ta_pair_info fields and the
=/X CIGAR bytes the device must produce.  ``pin()`` ties the two to the
oracle: the DP's score and target_begin equal the oracle's and its goal is
consistent with the CIGAR's consumption."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIELDS = ("query_begin", "query_end", "target_begin", "target_end", "n_eq", "n_x", "n_ins", "n_del", "n_gap_runs",
          "n_free")
GLOBAL, LOCAL, SEMI = 0, 1, 2

_lib = None


def _dp():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "annotate_dp.c")
        out = os.path.join(ROOT, "build", "annotate_ref")
        os.makedirs(out, exist_ok=True)
        so = os.path.join(out, "libannotate_dp.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            tmp = f"{so}.{os.getpid()}"
            subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", tmp, src])
            os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.annotate_goal.argtypes = [C.c_char_p, C.c_uint, C.c_char_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    return _lib


def goal(q: bytes, t: bytes, mode: int, match: int, mismatch: int, gap: int, gap_open: int = 0):
    """(score, goal_i, goal_j); gap is gap_extend when gap_open != 0."""
    sc, gi, gj = C.c_int(0), C.c_uint(0), C.c_uint(0)
    r = _dp().annotate_goal(q, len(q), t, len(t), int(mode), match, mismatch, gap_open, gap, C.byref(sc), C.byref(gi),
                            C.byref(gj))
    assert r == 0
    return sc.value, gi.value, gj.value


def ops_of(cigar: bytes) -> str:
    """The op string of a run-length CIGAR ("1\\0" is the empty one)."""
    if cigar == b"1\0":
        return ""
    runs = re.findall(rb"(\d+)([A-Z=])", cigar)
    assert b"".join(c + o for c, o in runs) == cigar, cigar
    return "".join(o.decode() * int(c) for c, o in runs)


def rle(ops: str) -> bytes:
    if not ops:
        return b"1\0"
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append(f"{e - k}{ops[k]}")
        k = e
    return "".join(out).encode()


def collapse(eqx: bytes) -> bytes:
    """=/X back to M with adjacent runs merged: the base CIGAR."""
    return rle(ops_of(eqx).replace("=", "M").replace("X", "M"))


def expected(q: bytes, t: bytes, mode: int, cigar: bytes, gi: int, gj: int):
    """(info dict, eqx bytes) of a pair whose CIGAR is ``cigar`` and goal cell (gi, gj)."""
    ops = ops_of(cigar)
    n, m = len(q), len(t)
    i = j = 0
    if mode == LOCAL:  # the path ends at the goal cell: it starts there minus its consumption
        i, j = gi - sum(o in "MD" for o in ops), gj - sum(o in "MI" for o in ops)
    i0, j0 = i, j
    ext, free, pos = [], [], []
    lead = 0  # the free first run (semi-global): I along row 0 or D along column 0
    if mode == SEMI and ops and ops[0] in "ID":
        while lead < len(ops) and ops[lead] == ops[0]:
            lead += 1
    for k, o in enumerate(ops):
        pos.append((i, j))
        trailing = mode == SEMI and i >= gi and j >= gj  # the path has reached the goal cell
        free.append(trailing or (mode == SEMI and k < lead))
        if o == "M":
            ext.append("=" if q[i] == t[j] else "X")
            i, j = i + 1, j + 1
        elif o == "I":
            ext.append("I")
            j += 1
        else:
            assert o == "D", o
            ext.append("D")
            i += 1
    info = dict.fromkeys(FIELDS, 0)
    prev = None
    for k, o in enumerate(ext):
        key = (o, free[k])
        if free[k]:
            info["n_free"] += 1
        else:
            info[{"=": "n_eq", "X": "n_x", "I": "n_ins", "D": "n_del"}[o]] += 1
            if o in "ID" and key != prev:
                info["n_gap_runs"] += 1
        prev = key
    if mode == GLOBAL:
        assert (i, j) == (n, m)
        span = (0, n, 0, m)
    elif mode == LOCAL:
        assert (i, j) == (gi, gj)
        span = (i0, gi, j0, gj)
    else:
        assert (i, j) == (n, m)
        # the cell after the leading run (columns past the goal cell belong to the trailing run)
        lead_cnt = sum(1 for k in range(lead) if not (pos[k][0] >= gi and pos[k][1] >= gj))
        b = pos[lead_cnt] if lead_cnt < len(ops) else (i, j)
        span = (b[0], gi, b[1], gj)
    info["query_begin"], info["query_end"], info["target_begin"], info["target_end"] = span
    return info, rle("".join(ext))


def pin(q, t, mode, scoring, gap_open, cigar, oracle_score, oracle_tb):
    """The helper's DP against the oracle's results for this pair; returns its goal cell."""
    sc, gi, gj = goal(q, t, mode, *scoring, gap_open=gap_open or 0)
    assert sc == oracle_score, (sc, oracle_score)
    assert oracle_tb == (gj + 1 if mode == LOCAL else 0)
    ops = ops_of(cigar)
    qc = sum(o in "MD" for o in ops)
    tc = sum(o in "MI" for o in ops)
    if mode == LOCAL:
        assert qc <= gi and tc <= gj
    else:
        assert (qc, tc) == (len(q), len(t))
        if mode == GLOBAL:
            assert (gi, gj) == (len(q), len(t))
        else:  # what follows the goal cell is the appended run: I when gi == n, else D
            assert gi == len(q) or gj == len(t)
            i = j = k = 0
            while k < len(ops) and not (i >= gi and j >= gj):
                i += ops[k] in "MD"
                j += ops[k] in "MI"
                k += 1
            assert (i, j) == (gi, gj)
            assert set(ops[k:]) <= ({"I"} if gi == len(q) else {"D"})
    return gi, gj


def score_from_info(info, scoring, gap_open=None):
    match, mismatch, gap = scoring
    s = match * info["n_eq"] + mismatch * info["n_x"] + gap * (info["n_ins"] + info["n_del"])
    return s + (gap_open or 0) * info["n_gap_runs"]
