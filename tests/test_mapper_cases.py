"""The directed mapper cases (tests/mapper_cases.py) on the CPU: their expected
values agree between the restatements (and with the reference build, where
oracle/_ref exists), and the cases bite -- a FindLIS or Minimize that breaks
one rule changes the result on a case of the group named for that rule."""
import pytest

import mapper_cases as mc
from oracle import pymapper as pm

M32 = 0xFFFFFFFF
have_ref = pm.RefMapper.available()


@pytest.fixture(scope="module")
def chains():
    return mc.chain_cases()


@pytest.fixture(scope="module")
def mins():
    """[(name, seq, k, w, pm.minimize(seq, k, w))], computed once."""
    return [(name, s, k, w, pm.minimize(s, k, w, True)) for name, s, k, w in mc.minimizer_cases()]


# --------------------------------------------------------------------------
# the case lists are what they claim to be
# --------------------------------------------------------------------------
def test_chain_case_groups(chains):
    groups = {mc.chain_group(n) for n, _ in chains}
    assert groups == {"gap", "equal_f", "tie_prev", "tie_best", "window", "tail", "big_pos", "sizes"}
    by = dict(chains)
    assert [len(by[f"sizes/n{n}"]) for n in mc.SIZES] == list(mc.SIZES)
    assert {mc.sorted_end(h) for n, h in chains if n.startswith("tail/S")} >= {1, 2}
    assert all(mc.sorted_end(h) == len(h) - 1 for n, h in chains if n.startswith("tail/Sn1"))
    assert all(mc.sorted_end(h) == len(h) for n, h in chains if mc.chain_group(n) in ("window", "sizes", "gap"))
    assert max(max(max(x) for x in h) for n, h in chains if n.startswith("big_pos/")) == 2 ** 31 - 1
    for n, h in chains:
        assert all(1 <= f <= mc.P31 and 1 <= r <= mc.P31 for f, r in h), n


def test_sizes_chain_lengths(chains):
    """The long lists send the uint16 LIS/PREV arrays and the global path through long prev walks."""
    for name, hits in chains:
        if not name.startswith("sizes/"):
            continue
        n, c = len(hits), pm.find_lis(hits)
        if n >= 12287:
            assert len(c) >= 12000, name
        elif n >= 3071:
            assert len(c) >= 3000, name
        if n > 2:  # the end decoys keep the chain off the first and the last hit
            assert c[0] == hits[1] and c[-1] == hits[-2], name


def test_find_lis_fast_vs_slow(chains):
    for name, hits in chains:
        if len(hits) <= 3073:
            assert pm.find_lis(hits) == pm.find_lis_slow(hits), name


@pytest.mark.skipif(not have_ref, reason="oracle/_ref not built (reference sources absent)")
def test_find_lis_vs_reference_build(chains):
    ref = pm.RefMapper()
    for name, hits in chains:
        want = ref.find_lis(hits)
        assert pm.find_lis(hits) == want, name
        if len(hits) <= 3073:
            assert pm.find_lis_slow(hits) == want, name


@pytest.mark.skipif(not have_ref, reason="oracle/_ref not built (reference sources absent)")
def test_minimize_vs_reference_build(mins):
    ref = pm.RefMapper()
    for name, s, k, w, got in mins:
        want, uniq = ref.minimize(s, k, w, True)
        assert got == want, name
        assert len(set(want)) == uniq == len(pm.first_occurrences(got)), name


def test_minimizer_case_geometry(mins):
    """Every (k, w) has the full->tail boundary and the last entry one below, on
    and one above both tile edges, and a tail group across each edge; no length
    lies where the reference reads past its string."""
    seen = {}
    for name, s, k, w, m in mins:
        L = len(s)
        assert L < k or L >= w + k - 2, name
        assert len(m) == mc.n_lead(L, k, w) + mc.n_full(L, k, w) + mc.n_tail(L, k, w), name
        if L >= k:
            d = seen.setdefault((k, w), {"ft": set(), "last": set(), "straddle": set()})
            nbf = mc.n_lead(L, k, w) + mc.n_full(L, k, w)
            d["ft"].add(nbf)
            d["last"].add(len(m) - 1)
            for t in (1, 2):
                if nbf < mc.TILE * t < len(m) - 1:
                    d["straddle"].add(t)
    assert set(seen) == set(mc.KW)
    edges = {mc.TILE * t + e for t in (1, 2) for e in (-1, 0, 1)}
    for (k, w), d in seen.items():
        assert edges <= d["ft"] and edges <= d["last"], (k, w)
        assert d["straddle"] == ({1, 2} if w >= 3 else set()), (k, w)
    alpha = [set(s) for _, s, _, _, _ in mins]
    assert any(len(a) == 1 for a in alpha) and any(a == set(b"AC") for a in alpha)
    assert any(a & set(b"Nacgt") for a in alpha)


def _drop_adjacent_repeats(m):
    return [x for i, x in enumerate(m) if i == 0 or x != m[i - 1]]


def test_trailing_entries_repeat_non_adjacent(mins):
    """At least four cases hold a trailing entry equal to an argmin several
    entries back: first_occurrences keeps fewer than "drop adjacent repeats"."""
    n = 0
    for name, s, k, w, m in mins:
        adj, fo = _drop_adjacent_repeats(m), pm.first_occurrences(m)
        if len(fo) < len(adj):
            nt = mc.n_tail(len(s), k, w)
            far = [i for i in range(1, len(m)) if m[i] != m[i - 1] and m[i] in m[:i - 1]]
            assert far and far[0] >= len(m) - nt, name  # only trailing entries repeat from afar
            n += 1
    assert n >= 4, n


# --------------------------------------------------------------------------
# the cases bite: wrong variants of FindLIS
# --------------------------------------------------------------------------
def lis_variant(hits, bound_le=False, f_rule=True, last_j=False, last_best=False, signed=False, tail_window=False,
                narrow_window=False):
    """find_lis_slow with one rule broken.  tail_window and narrow_window break
    the kernel's moving lower bound `lo` (tm_chain.hip), which the reference
    does not have: the bound kept for the unsorted tail, or one hit too tight."""
    n = len(hits)
    if n == 0:
        return []
    S = mc.sorted_end(hits)
    lis, prev = [1] * n, [-1] * n
    lo = 0
    for i in range(1, n):
        fi, ri = hits[i]
        if i < S:
            while lo < i and fi - hits[lo][0] >= (4999 if narrow_window else 5000):
                lo += 1
        for j in range(lo if ((tail_window and i >= S) or (narrow_window and i < S)) else 0, i):
            fj, rj = hits[j]
            df, dr = (fi - fj, ri - rj) if signed else ((fi - fj) & M32, (ri - rj) & M32)
            near = (df <= 5000 and dr <= 5000) if bound_le else (df < 5000 and dr < 5000)
            better = lis[j] + 1 >= max(lis[i], 2) if last_j else lis[j] + 1 > lis[i]
            if ri > rj and (fi != fj or not f_rule) and near and better:
                lis[i] = lis[j] + 1
                prev[i] = j
    best = max(range(n), key=lambda i: (lis[i], i if last_best else -i))
    chain = []
    i = best
    while i >= 0:
        chain.append(hits[i])
        i = prev[i]
    return chain[::-1]


def test_variant_without_a_broken_rule_is_find_lis(chains):
    for name, hits in chains:
        if len(hits) <= 800:
            assert lis_variant(hits) == pm.find_lis(hits), name


VARIANTS = [("gap", dict(bound_le=True)), ("equal_f", dict(f_rule=False)), ("tie_prev", dict(last_j=True)),
            ("tie_best", dict(last_best=True)), ("tail", dict(signed=True)), ("tail", dict(tail_window=True)),
            ("window", dict(narrow_window=True))]


@pytest.mark.parametrize("group,broken", VARIANTS, ids=[next(iter(b)) for _, b in VARIANTS])
def test_chain_cases_bite(chains, group, broken):
    killed = [name for name, hits in chains if mc.chain_group(name) == group
              and mc.summary(lis_variant(hits, **broken)) != mc.summary(pm.find_lis(hits))]
    assert killed, f"no {group} case tells FindLIS from the variant {broken}"
    if group == "gap":  # exactly the lists with a gap of 5000
        assert killed == [n for n, _ in chains if n.startswith("gap/") and n.endswith("5000")]


# --------------------------------------------------------------------------
# the cases bite: wrong variants of Minimize / remove_duplicates
# --------------------------------------------------------------------------
def minimize_variant(seq, k, w, rightmost=False, pad=0):
    """pm.minimize with ties going to the rightmost k-mer, or with bytes past
    the end of the sequence read as code `pad`."""
    L = len(seq)
    if L < k:
        return []

    def code(i):
        c = 0
        for t in range(k):
            c = ((c << 2) | (int(pm._CODE[seq[i + t]]) if i + t < L else pad)) & M32
        return c

    def wmin(lo, hi):
        best, tup = M32, (0, 0, False)
        for i in range(lo, hi + 1):
            c = code(i)
            if c < best or (rightmost and c == best and c < M32):
                best, tup = c, (c, i + 1, True)
        return tup

    out = [wmin(0, u - k) for u in range(k, w + k - 1)]
    out += [wmin(i - w + 1, i) for i in range(w - 1, L - k + 1)]
    out += [wmin(L - u, L - k) for u in range(k, w + k - 1) if L >= u]
    return out


def _short(mins, limit=260):
    return [c for c in mins if len(c[1]) <= limit]


def test_minimize_variant_without_a_broken_rule_is_minimize(mins):
    for name, s, k, w, m in _short(mins):
        assert minimize_variant(s, k, w) == m, name


def test_minimizer_cases_bite_rightmost_minimum(mins):
    killed = [name for name, s, k, w, m in _short(mins) if minimize_variant(s, k, w, rightmost=True) != m]
    assert killed
    assert any("homopolymer" in n for n in killed) and any("/ac" in n for n in killed)


def test_minimizer_cases_bite_adjacent_dedup(mins):
    killed = [name for name, s, k, w, m in mins if _drop_adjacent_repeats(m) != pm.first_occurrences(m)]
    assert len(killed) >= 4
    assert {(k, w) for name, s, k, w, m in mins if name in killed} >= {(1, 64), (7, 33), (15, 64)}


def test_minimizer_cases_never_read_past_the_end(mins):
    """The third variant the cases were asked to kill -- bytes past the end read
    as another code than 0 -- cannot be told apart on any admissible input:
    Minimize reads k-mers up to max(L - k, w - 2), that is bytes up to
    max(L, w + k - 2) - 1, and every length with k <= L < w + k - 2 is left out
    (the reference reads past its string there).  So this asserts the opposite:
    no case depends on what lies past the end, at the shortest admissible
    lengths included."""
    n = 0
    for name, s, k, w, m in mins:
        L = len(s)
        assert L < k or max(L - k, w - 2) + k - 1 <= L - 1, name
        if L <= 130:
            assert minimize_variant(s, k, w, pad=3) == m, name
            n += L == w + k - 2
    assert n >= len(mc.KW)
