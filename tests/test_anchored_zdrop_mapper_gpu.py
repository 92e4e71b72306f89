"""The mapper's end extension with z-drop (tm_map_batch_band_ends_zdrop,
tm_map_files_band_ends_zdrop, team_mapper_amd --band N --extend-ends --zdrop Z,
Index.map_batch(band=, extend_ends=True, zdrop=)): as
tests/test_anchored_mapper_gpu.py, the lines of the command without the options
give each read's window and middle CIGAR; the expected lines are the window
plus the two ends of the z-drop definition (tests/anchored_zdrop_ref.py),
stitched on the host, and the CLI and Python must equal them byte for byte.

Scoring 2/-4/-4 (a drop needs negative drift), band 16.  Z = 10^6 never fires:
the lines are --extend-ends' own.  Small Z, found on the CPU from the windows
of the committed global run (tests/golden/mapper/run3.paf, r60k.fasta, 46
non-empty ends, 4,475 fill steps): at Z = 10 the reference drops 3 ends, at
Z = 0 it drops 5 and sweeps 2,058 steps.  The fixture reads are related to the
genome to their ends, so every one of those drops comes after the end's best
cell and no line changes; the test asserts the counts it relies on.

Lines that DO change need an end that dies and comes back: plain anchored
alignment already stops at its best cell, so junk alone clips the same with or
without Z.  The second half of the file builds such reads from the genome -- an
exact core (the seeds), then 80 bases with a substitution at every 10th base
(no 15-mer survives, so the chain's window ends at the core; score about +110),
150 unrelated bases (a dip of several hundred), and 400 bases of the first kind
again (about +560: plain anchored alignment runs to the read's end) -- on the
right, on the left and on both sides (the fixture reads above cover the reverse strand).  At Z = 40 the
reference clips such an end after its first 80 bases; the mapper must equal the
reference composition byte for byte, which it cannot do if either end plan
ignores Z."""
import ctypes as C
import os

import anchored_ref as AR
import anchored_zdrop_ref as ZR
import pytest
from conftest import GOLDEN
from test_anchored_mapper_gpu import _cli, _records, _revcomp

from bioinfo1_amd import mapper as M

pytestmark = pytest.mark.gpu
MG = os.path.join(GOLDEN, "mapper")
GENOME = os.path.join(MG, "g60k.fasta")
BAND = 16
SC = (2, -4, -4)
BASE = ["-a", "global", "-c", "-m", "2", "-n", "-4", "-g", "-4", "--band", str(BAND)]
BIG = 10 ** 6
SMALL = (10, 0)


@pytest.fixture(scope="module")
def genome():
    return _records(GENOME)[0]


@pytest.fixture(scope="module")
def base(genome):
    """r60k.fasta: the lines without the options and, per line, the window and the two ends' cell values."""
    return build_base([GENOME, os.path.join(MG, "r60k.fasta")], genome)


def build_base(files, genome):
    by_name = dict(_records(files[1]))
    g = genome[1]
    rc, L = _revcomp(g), len(g)
    lines = _cli(BASE + files).splitlines()
    ends = []
    for ln in lines:
        c = ln.split(b"\t")
        R = by_name[c[0]]
        fwd = c[4] == b"+"
        S = g if fwd else rc
        qb, qe = int(c[2]), int(c[3]) - 1
        tb, te = (int(c[7]), int(c[8]) - 1) if fwd else (L - int(c[8]), L - int(c[7]) - 1)
        nr = len(R) - 1 - qe
        mr = min(L - 1 - te, nr + BAND)
        ml = min(tb, qb + BAND)
        right = ZR.fill(R[qe + 1:], S[te + 1:te + 1 + mr], *SC, BAND)
        left = ZR.fill(R[:qb][::-1], S[tb - ml:tb][::-1], *SC, BAND)
        ends.append((fwd, qb, qe, tb, te, left, right))
    return files, lines, ends, L


def expected_lines(base, z):
    """-> (lines, ends that dropped, steps swept)."""
    _, lines, ends, L = base
    out, drops, steps = [], 0, 0
    for ln, (fwd, qb, qe, tb, te, lf, rf) in zip(lines, ends):
        c = ln.split(b"\t")
        left, right = ZR.result(lf, z), ZR.result(rf, z)
        drops += (left.drop is not None) + (right.drop is not None)
        steps += left.swept_steps + right.swept_steps
        qb2, qe2, tb2, te2 = qb - left.gi, qe + right.gi, tb - left.gj, te + right.gj
        ts, tend = (tb2, te2 + 1) if fwd else (L - te2 - 1, L - tb2)
        cigar = AR.stitch(left.cigar, c[12][5:], right.cigar)
        assert AR.consumed(cigar) == (qe2 - qb2 + 1, te2 - tb2 + 1)
        out.append(b"\t".join([c[0], c[1], b"%d" % qb2, b"%d" % (qe2 + 1), c[4], c[5], c[6], b"%d" % ts, b"%d" % tend,
                               b"%d" % (int(c[9]) + left.score + right.score), b"%d" % (qe2 - qb2 + 1), c[11],
                               b"cg:Z:" + cigar]))
    return out, drops, steps


def test_huge_z_is_extend_ends_alone(base):
    files = base[0]
    plain = _cli(BASE + ["--extend-ends"] + files)
    assert _cli(BASE + ["--extend-ends", "--zdrop", str(BIG)] + files) == plain and plain
    want, drops, _ = expected_lines(base, BIG)
    assert drops == 0 and plain.splitlines() == want


@pytest.mark.parametrize("z", SMALL)
def test_cli_lines_equal_the_definition(base, z):
    files = base[0]
    want, drops, steps = expected_lines(base, z)
    _, none, all_steps = expected_lines(base, None)
    print("Z", z, "ends that drop", drops, "steps", steps, "of", all_steps)
    assert none == 0 and drops >= 1 and (drops, steps, all_steps) == {10: (3, 4475, 4475), 0: (5, 2058, 4475)}[z]
    got = _cli(BASE + ["--extend-ends", "--zdrop", str(z)] + files).splitlines()
    assert len(got) == len(want) > 0
    for a, b in zip(got, want):
        assert a == b, (z, a[:120], b[:120])
    # anywhere among the options
    assert _cli(["--zdrop", str(z)] + BASE + ["--extend-ends"] + files).splitlines() == got
    assert _cli(BASE[:2] + files + ["--extend-ends"] + BASE[2:] + ["--zdrop", str(z)]).splitlines() == got


def test_python_agrees_with_the_cli(base, genome, tmp_path):
    files, _, _, L = base
    z = SMALL[0]
    want, _, _ = expected_lines(base, z)
    seqs = [s for _, s in _records(files[1])]
    mp = M.Mapper(0)
    idx = M.Index(mp, genome[0].decode(), genome[1], 15, 5, 0.001)
    try:
        opt = M.Options.make(type=0, match=SC[0], mismatch=SC[1], gap=SC[2], want_cigar=True)
        res = idx.map_batch(seqs, opt, band=BAND, extend_ends=True, zdrop=z)
        stages, _ = mp.stage_times()
        assert len(stages) == len(M.Mapper.STAGES) == 8  # no stage added
        assert int(res.mapped.sum()) == len(want)
        k = 0
        for i in range(len(seqs)):
            if not res.mapped[i]:
                continue
            c = want[k].split(b"\t")
            fwd = bool(res.strand_fwd[i])
            tb, te = int(res.t_begin[i]), int(res.t_end[i])
            ts, tend = (tb, te + 1) if fwd else (L - te - 1, L - tb)
            assert (int(c[2]), int(c[3]) - 1, int(c[7]), int(c[8])) == (int(res.q_begin[i]), int(res.q_end[i]), ts, tend), i
            assert int(c[9]) == int(res.scores[i]) and c[12][5:] == res.cigar(i), i
            k += 1
    finally:
        idx.close()
        mp.close()
    out = str(tmp_path / "z.paf")
    M.map_files(files[0], files[1], out=out, band=BAND, extend_ends=True, zdrop=z, type=0, match=SC[0],
                mismatch=SC[1], gap=SC[2], want_cigar=True)
    assert open(out, "rb").read().splitlines() == want


def test_affine_gaps_with_z(base, genome):
    """--gap-open with --zdrop: both end plans are the affine z-drop plans."""
    files = base[0]
    args = BASE[:7] + ["-g", "-1", "--band", str(BAND), "--gap-open", "-3"]
    plain = _cli(args + ["--extend-ends"] + files)
    assert _cli(args + ["--extend-ends", "--zdrop", str(BIG)] + files) == plain and plain
    got = _cli(args + ["--extend-ends", "--zdrop", "0"] + files).splitlines()
    assert len(got) == len(plain.splitlines())


def test_argument_errors(genome):
    files = [GENOME, os.path.join(MG, "r60k.fasta")]
    for args in (BASE + ["--zdrop", "10"],                      # without --extend-ends
                 ["-a", "global", "-c", "--zdrop", "10"],
                 BASE + ["--extend-ends", "--zdrop", "-1"],     # a negative value
                 BASE + ["--extend-ends", "--zdrop", "ten"],    # not a number
                 BASE + ["--extend-ends", "--zdrop", "10x"],
                 BASE + ["--extend-ends", "--zdrop", "2147483648"]):
        p = M.run_cli(args + files, timeout=120)
        assert p.returncode == 1 and b"--zdrop" in p.stderr and p.stdout == b"", args
    with pytest.raises(ValueError, match="zdrop"):
        M.map_files(files[0], files[1], band=16, zdrop=10)
    with pytest.raises(ValueError, match="zdrop"):
        M.map_files(files[0], files[1], band=16, extend_ends=True, zdrop=-1)
    # the C entries: zdrop < 0 is tm_map_files_band_ends itself; the other rules stay (TM_ERR_ARG = 3)
    L = M.lib()
    r = L.tm_map_files_band_ends_zdrop(files[0].encode(), files[1].encode(), C.byref(M.Options.make(type=1)), b"-", 0,
                                       0, 16, None, 10)
    assert r == 3
    mp = M.Mapper(0)
    idx = M.Index(mp, genome[0].decode(), genome[1], 15, 5, 0.001)
    try:
        with pytest.raises(ValueError, match="zdrop"):
            idx.map_batch([b"ACGT" * 20], M.Options.make(), band=16, zdrop=10)
        with pytest.raises(ValueError, match="zdrop"):
            idx.map_batch([b"ACGT" * 20], M.Options.make(), band=16, extend_ends=True, zdrop="10")
    finally:
        idx.close()
        mp.close()


# ---- reads whose ends die and come back: Z changes their lines
Z_DIE = 40
CORE, NEAR, JUNK, FAR = 400, 80, 150, 400


def _mutate(b: bytes) -> bytes:
    """A substitution at every 10th base: no exact 15-mer survives, the drift stays positive."""
    b = bytearray(b)
    for k in range(4, len(b), 10):
        b[k] = {65: 67, 67: 71, 71: 84, 84: 65}.get(b[k], 65)
    return bytes(b)


def dying_reads(g: bytes):
    """[(name, read)]: `right` / `left` / `both` have ends that die and come back; `junk` only dies."""
    import numpy as np

    rng = np.random.default_rng(0x2D60)

    def junk(n):
        return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))

    def right_end(a):  # after a core that ends at genome position a
        return _mutate(g[a:a + NEAR]) + junk(JUNK) + _mutate(g[a + NEAR + JUNK:a + NEAR + JUNK + FAR])

    def left_end(a):  # before a core that begins at genome position a
        return _mutate(g[a - NEAR - JUNK - FAR:a - NEAR - JUNK]) + junk(JUNK) + _mutate(g[a - NEAR:a])

    def core(a):
        return g[a:a + CORE]

    return [(b"right", core(5000) + right_end(5000 + CORE)),
            (b"left", left_end(15000) + core(15000)),
            (b"both", left_end(25000) + core(25000) + right_end(25000 + CORE)),
            (b"junk", core(45000) + junk(JUNK))]


@pytest.fixture(scope="module")
def dying(genome, tmp_path_factory):
    reads = dying_reads(genome[1])
    fn = str(tmp_path_factory.mktemp("zdrop") / "dying.fasta")
    with open(fn, "wb") as f:
        for name, seq in reads:
            f.write(b">" + name + b"\n" + seq + b"\n")
    return build_base([GENOME, fn], genome)


def test_reads_whose_ends_die_and_come_back(dying, genome):
    files, lines, ends, _ = dying
    names = [ln.split(b"\t")[0] for ln in lines]
    assert names == [b"right", b"left", b"both", b"junk"]  # one line per read, in read order
    want, drops, steps = expected_lines(dying, Z_DIE)
    plain, none, all_steps = expected_lines(dying, None)
    print("dying reads: ends that drop", drops, "steps", steps, "of", all_steps)
    # on the reference: which end of which read drops, and which lines Z changes
    dropped = {}
    for name, (fwd, qb, qe, tb, te, lf, rf) in zip(names, ends):
        dropped[name] = (ZR.result(lf, Z_DIE).drop is not None, ZR.result(rf, Z_DIE).drop is not None)
    assert dropped[b"right"] == (False, True) and dropped[b"left"] == (True, False), dropped
    assert dropped[b"both"] == (True, True), dropped
    changed = {n for n, a, b in zip(names, want, plain) if a != b}
    assert changed == {b"right", b"left", b"both"}, changed  # junk alone clips the same without Z
    assert none == 0 and steps < all_steps
    for a, b in zip(want, plain):  # a clipped end: a shorter aligned block
        assert int(a.split(b"\t")[10]) <= int(b.split(b"\t")[10])
    # the mapper
    assert _cli(BASE + ["--extend-ends"] + files).splitlines() == plain
    assert _cli(BASE + ["--extend-ends", "--zdrop", str(BIG)] + files).splitlines() == plain
    got = _cli(BASE + ["--extend-ends", "--zdrop", str(Z_DIE)] + files).splitlines()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b, (a[:120], b[:120])
    nocig = _cli([x for x in BASE if x != "-c"] + ["--extend-ends", "--zdrop", str(Z_DIE)] + files).splitlines()
    assert [ln.split(b"\t") for ln in nocig] == [ln.split(b"\t")[:12] for ln in want]  # the score-only fills
    # Index.map_batch
    seqs = [s for _, s in _records(files[1])]
    L = len(genome[1])
    mp = M.Mapper(0)
    idx = M.Index(mp, genome[0].decode(), genome[1], 15, 5, 0.001)
    try:
        opt = M.Options.make(type=0, match=SC[0], mismatch=SC[1], gap=SC[2], want_cigar=True)
        for z, exp in ((Z_DIE, want), (None, plain)):
            res = idx.map_batch(seqs, opt, band=BAND, extend_ends=True, zdrop=z)
            assert res.mapped.all()
            for i, ln in enumerate(exp):
                c = ln.split(b"\t")
                fwd = bool(res.strand_fwd[i])
                tb, te = int(res.t_begin[i]), int(res.t_end[i])
                ts, tend = (tb, te + 1) if fwd else (L - te - 1, L - tb)
                assert (int(c[2]), int(c[3]) - 1, int(c[7]), int(c[8])) == (int(res.q_begin[i]), int(res.q_end[i]), ts, tend), (z, i)
                assert int(c[9]) == int(res.scores[i]) and c[12][5:] == res.cigar(i), (z, i)
    finally:
        idx.close()
        mp.close()


def test_affine_ends_that_die_and_come_back(dying):
    """--gap-open: the affine z-drop plans change the same lines."""
    files = dying[0]
    args = BASE[:7] + ["-g", "-2", "--band", str(BAND), "--gap-open", "-4", "--extend-ends"]
    plain = _cli(args + files).splitlines()
    got = _cli(args + ["--zdrop", str(Z_DIE)] + files).splitlines()
    assert len(got) == len(plain) == 4
    changed = {a.split(b"\t")[0] for a, b in zip(got, plain) if a != b}
    assert changed == {b"right", b"left", b"both"}, changed


def test_wide_band_warns(dying):
    files = dying[0]
    args = ["-a", "global", "-c", "-m", "2", "-n", "-4", "-g", "-4", "--extend-ends", "--zdrop", "40"]
    p = M.run_cli(args + ["--band", "64"] + files, timeout=120)
    assert p.returncode == 0 and b"warning: --zdrop" in p.stderr and p.stdout
    p = M.run_cli(args + ["--band", "32"] + files, timeout=120)
    assert p.returncode == 0 and b"warning" not in p.stderr
