"""Directed inputs for the mapper stages (chaining and minimizers), shared by
the CPU tests (tests/test_mapper_cases.py) and the GPU stage tests
(tests/test_mapper_stages_gpu.py).  Plain data builders only: no GPU import.

``chain_cases()``     -> [(name, hits)], name = "<group>/<what>"; every list
                         is built so that the FindLIS rule its group names
                         decides the summary (length, first hit, last hit).
``minimizer_cases()`` -> [(name, seq, k, w)] with the tile (1,024 entries) and
                         entry-group boundaries of tm_minimizers.hip placed
                         one below, on and one above a tile edge.
"""
from __future__ import annotations

import random

GAP = 5000  # FindLIS chains two hits only if both unsigned differences are below this
TILE = 1024  # minimizer entries per workgroup (tm_internal.h: kMinTile)
SIZES = (1, 2, 255, 256, 257, 3071, 3072, 3073, 12287, 12288, 12289)
KW = ((1, 1), (1, 64), (15, 1), (15, 5), (15, 64), (7, 33))
P31 = 2 ** 31 - 1


def summary(chain):
    """What tm_chain_batch reports of a chain: (length, first hit, last hit)."""
    return (len(chain), chain[0] if chain else (0, 0), chain[-1] if chain else (0, 0))


def sorted_end(hits):
    """Length of the prefix over which f is non-decreasing (the kernel's S)."""
    for j in range(len(hits) - 1):
        if hits[j + 1][0] < hits[j][0]:
            return j + 1
    return len(hits)


# --------------------------------------------------------------------------
# chaining
# --------------------------------------------------------------------------
def _gap_cases():
    out = []
    for d in (GAP - 1, GAP, GAP + 1):
        for axis, (df, dr) in (("f", (d, 10)), ("r", (10, d)), ("both", (d, d))):
            x = (100, 100)
            y = (100 + df, 100 + dr)
            z = (y[0] + 7, y[1] + 7)
            # x-y chains only below the limit: (3, x, z), else (2, y, z)
            out.append((f"gap/{axis}{d}", [x, y, z]))
            # the same gap in the middle of two runs: one chain of 8 or the first run of 4
            a = [(50 + 3 * i, 60 + 2 * i) for i in range(4)]
            b = [(a[-1][0] + df + 3 * i, a[-1][1] + dr + 2 * i) for i in range(4)]
            out.append((f"gap/runs_{axis}{d}", a + b))
    return out


def _equal_f_cases():
    return [
        ("equal_f/rising_r", [(10, 100), (10, 200), (10, 300)]),
        ("equal_f/equal_r", [(10, 100), (20, 100), (30, 100)]),
        ("equal_f/falling_r", [(10, 300), (20, 200), (30, 100)]),
        # the second (10, .) may not sit on the first: 3 hits chain, not 4
        ("equal_f/inner", [(5, 50), (10, 100), (10, 200), (20, 300)]),
        # equal f at the chain's end: the last hit is (10, 100), not (10, 200)
        ("equal_f/last", [(5, 50), (10, 100), (10, 200)]),
        # equal f at the head: with the rule the chain starts at the first (7, .)
        ("equal_f/head", [(7, 10), (7, 20), (9, 30), (11, 40)]),
        ("equal_f/far_r", [(300, 1), (300, 4000), (300, 8000), (301, 8001)]),
    ]


def _tie_prev_cases():
    out = []
    a = [(100, 2000), (200, 2100)]
    b = [(300, 1000), (400, 1100)]
    # both a[-1] and b[-1] carry lis 2: the smaller j (a) wins, first = a[0]
    out.append(("tie_prev/two_heads", a + b + [(500, 3000)]))
    c = [(410, 500), (420, 600)]
    out.append(("tie_prev/three_heads", a + b + c + [(500, 3000), (510, 3010)]))
    # 300 heads that cannot chain with each other (falling r), then one hit all
    # of them reach: the candidates of one i spread over every thread of a workgroup
    heads = [(10 + i, 4000 - i) for i in range(300)]
    out.append(("tie_prev/300_heads", heads + [(400, 4500)]))
    # the first five heads are out of reach in r: the winner is j = 5
    far = [(1 + i, 9500 - i) for i in range(5)]
    out.append(("tie_prev/first_reachable", far + [(h[0], h[1]) for h in heads[:290]] + [(400, 4500)]))
    # the tie is between j = i - 1 and j = i - 2
    out.append(("tie_prev/adjacent", [(10, 300), (20, 200), (30, 400)]))
    return out


def _tie_best_cases():
    a = [(100, 2000), (200, 2100), (300, 2200)]
    b = [(400, 1000), (500, 1100), (600, 1200)]
    inter = [x for p in zip(a, [(150, 1000), (250, 1100), (350, 1200)]) for x in p]
    # two chains of 300: the maximum is met at i = 299 and again at i = 599
    la = [(10 + 3 * i, 9000 + 2 * i) for i in range(300)]
    lb = [(1000 + 3 * i, 100 + 2 * i) for i in range(300)]
    return [("tie_best/disjoint", a + b), ("tie_best/interleaved", inter), ("tie_best/long", la + lb),
            ("tie_best/singletons", [(10, 300), (20, 200), (30, 100)])]


def _window_cases():
    out = []
    cl = [(1 + i, 1001 + i) for i in range(5)]
    d = (4000, 500)  # a head of its own: r below the cluster's
    # lo moves past hits 0..3 at once and stops on (5, 1005), exactly 4999 back;
    # a bound one too far would leave only d: (2, d, x) instead of (6, cl[0], x)
    out.append(("window/meet_4999", cl + [d, (5004, 5400)]))
    # the same with lo stopping one hit earlier (4998 back): both (4, .) and (5, .) are in
    out.append(("window/meet_4998", cl + [d, (5003, 5400)]))
    # jlo == i: every earlier hit is 5000 or more back
    out.append(("window/jlo_eq_i", [(1, 1), (2, 2), (5002, 3), (5003, 4)]))
    # jlo == i - 1: only the hit just before is in reach (4999 back), then the window holds two
    out.append(("window/jlo_eq_i_minus_1", [(1, 1), (2, 2), (3, 3), (5002, 5002), (5003, 5003)]))
    # lo jumps over a whole block of 600 hits (more than one stride of the workgroup)
    blk = [(1 + i // 2, 1 + i) for i in range(600)]
    out.append(("window/jump_600", blk + [(5299, 700), (5300, 701), (5301, 702)]))
    # lo advances by one at every hit: a sliding window that always holds the last 4999 bases
    out.append(("window/slide", [(1 + 1250 * i, 1 + 1249 * i) for i in range(40)]))
    # equal f at the window's lower edge: both are exactly 4999 back, the first wins
    out.append(("window/edge_equal_f", [(10, 900), (10, 800), (5009, 1000)]))
    return out


def _tail_cases():
    out = []
    # S = 1: the list descends at once; every later hit scans all earlier j.
    # Tail hits lie below the prefix in f: the unsigned difference wraps, no link.
    out.append(("tail/S1", [(1000, 100), (10, 500), (20, 600), (30, 550)]))
    # S = 2
    out.append(("tail/S2", [(1000, 100), (1001, 101), (10, 500), (20, 600), (5, 700), (25, 800)]))
    # S = n - 1: one tail hit, below every earlier f
    out.append(("tail/Sn1_below", [(100 + i, 100 + i) for i in range(20)] + [(50, 5000)]))
    # S = n - 1: one tail hit that extends the chain through a hit in mid-prefix
    out.append(("tail/Sn1_link", [(100 + 10 * i, 100 + 10 * i) for i in range(20)] + [(155, 4000)]))
    # the prefix runs far ahead (lo ends near its last hits); the tail's first
    # hit chains onto (100, 100), far before lo; the others lie below every f
    pre = [(100, 100)] + [(10000 + 1000 * i, 90 - i) for i in range(21)]
    out.append(("tail/far_before_lo", pre + [(150, 200), (50, 300), (60, 400)]))
    # the same with a long prefix (the tail scans more than one stride)
    pre = [(100, 100), (101, 99)] + [(6000 + 10 * i, 95 - (i % 90)) for i in range(700)]
    out.append(("tail/far_before_lo_long", pre + [(150, 200), (50, 300), (60, 400), (160, 250)]))
    return out


def _big_pos_cases():
    return [
        ("big_pos/chain_4999", [(P31 - 4999, P31 - 4999), (P31, P31)]),
        ("big_pos/break_5000", [(P31 - 5000, P31 - 5000), (P31, P31), (P31, 7)]),
        ("big_pos/f_only", [(P31 - 10, 5), (P31 - 5, 9), (P31, 11)]),
        ("big_pos/r_only", [(5, P31 - 10), (9, P31 - 5), (11, P31)]),
        ("big_pos/low_after_high", [(P31, 5), (3, 10), (4, 11)]),
        ("big_pos/span", [(1, 1), (P31, P31), (2, 2)]),
    ]


def sizes_case(n):
    """n hits, sorted by f: one colinear chain (f step 2, r step 1) with a decoy
    at either end and after every 50th hit.  Inner decoys share the f of the hit
    before them (they cannot sit on it) and tie with it as a predecessor of the
    next chain hit; the end decoys keep the chain's first and last hit off
    index 0 and n - 1."""
    if n == 1:
        return [(7, 9)]
    if n == 2:
        return [(7, 9), (8, 9000)]  # r out of reach: two singletons, the first wins
    hits = [(1, 900000)]
    f, r = 1, 1
    while len(hits) < n - 1:
        hits.append((f, r))
        if len(hits) % 50 == 0 and len(hits) < n - 1:
            hits.append((f, r + 1))
            r += 1
        f += 2
        r += 1
    hits.append((f, 1))
    assert len(hits) == n
    return hits


def chain_cases():
    out = (_gap_cases() + _equal_f_cases() + _tie_prev_cases() + _tie_best_cases() + _window_cases()
           + _tail_cases() + _big_pos_cases())
    out += [(f"sizes/n{n}", sizes_case(n)) for n in SIZES]
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def chain_group(name):
    return name.split("/")[0]


# --------------------------------------------------------------------------
# minimizers
# --------------------------------------------------------------------------
def n_lead(L, k, w):
    return 0 if L < k else w - 1


def n_full(L, k, w):
    return 0 if (L < k or L - k + 1 < w) else L - k + 1 - (w - 1)


def n_tail(L, k, w):
    return 0 if L < k else min(w - 1, L - k + 1)


def minimizer_lengths(k, w):
    """{L: why}.  With L >= w + k - 2 the entries are: NB = w - 1 leading ones,
    then the full windows up to entry NB + NF = L - k + 1, then the tail up to
    E = L - k + w.  NB is at most 63, so the lead->full boundary never reaches
    a tile edge: it lies inside the first tile of every case.  The other two
    boundaries are placed at 1024 t - 1, 1024 t and 1024 t + 1 for t = 1, 2."""
    out = {}
    for t in (1, 2):
        for d in (-1, 0, 1):
            v = TILE * t + d
            out.setdefault(v + k - 1, f"full_to_tail@{v}")  # NB + NF == v
            out.setdefault(v + 1 + k - w, f"last@{v}")  # E - 1 == v
        if w >= 3:  # the tail group [L-k+1, L-k+w-1) straddles the tile edge
            out.setdefault(TILE * t - (w - 1) // 2 + k - 1, f"tail_straddles@{TILE * t}")
            out.setdefault(TILE * t - 1 + k - 1 - (w - 3), f"tail_last_over@{TILE * t}")
    # the shortest lengths the reference defines, and sequences below k
    for L in (0, k - 1, w + k - 2, w + k - 1, w + k):
        if L >= 0:
            out.setdefault(L, "short")
    return {L: why for L, why in out.items() if L >= 0 and not (k <= L < w + k - 2)}


def minimizer_cases():
    rng = random.Random(0x317E)
    out = []
    for k, w in KW:
        for L, why in sorted(minimizer_lengths(k, w).items()):
            contents = {
                "homopolymer": b"ACGT"[(L + k) % 4:][:1] * L,
                "ac": (b"AC" * (L // 2 + 1))[:L],
                "acgt": bytes(rng.choice(b"ACGT") for _ in range(L)),
                "acgtn_lower": bytes(rng.choice(b"ACGTNacgt") for _ in range(L)),
            }
            for cname, seq in contents.items():
                if L == 0 and cname != "acgt":
                    continue
                out.append((f"k{k}w{w}/{why}/L{L}/{cname}", seq, k, w))
    # few distinct k-mers and a wide window: trailing entries that repeat the
    # argmin of a full window several entries back
    for k, w, L in ((1, 64, 200), (1, 64, 1025 + 31), (7, 33, 150), (7, 33, 1024 + 20), (15, 64, 1024 + 40),
                    (15, 5, 120)):
        for s in range(3):
            seq = bytes(rng.choice(b"ACGT") for _ in range(L))
            out.append((f"k{k}w{w}/trailing_repeat{s}/L{L}/acgt", seq, k, w))
    return out
