"""The mapper's end extension (tm_map_batch_band_ends, tm_map_files_band_ends,
team_mapper_amd --band N --extend-ends, Index.map_batch(band=, extend_ends=True)):
the lines of the same command without the option give each read's window and
middle CIGAR; from those the test builds the expected lines with the anchored
definition (tests/anchored_ref.py) and the Python stitcher -- the reverse
complement for '-' reads, the reversed ends for the left side -- and the CLI
output must equal them byte for byte.  Then: Python agrees with the CLI, affine
gaps against the affine model, the same coordinates and scores without -c, and
the argument errors."""
import ctypes as C
import os

import anchored_ref as AR
import pytest
from conftest import GOLDEN

from bioinfo1_amd import mapper as M

pytestmark = pytest.mark.gpu
MG = os.path.join(GOLDEN, "mapper")
GENOME = os.path.join(MG, "g60k.fasta")
BAND = 16
BASE = ["-a", "global", "-c", "--band", str(BAND)]


def _cli(args):
    p = M.run_cli(args, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout


def _records(fn):
    """[(name, sequence)] of a FASTA or FASTQ file."""
    lines = open(fn, "rb").read().splitlines()
    recs = []
    if lines and lines[0].startswith(b"@"):
        for k in range(0, len(lines) - 1, 4):
            recs.append((lines[k][1:].split()[0], lines[k + 1].strip()))
        return recs
    for ln in lines:
        if ln.startswith(b">"):
            recs.append([ln[1:].split()[0], b""])
        elif recs:
            recs[-1][1] += ln.strip()
    return [(n, s) for n, s in recs]


def _revcomp(g: bytes) -> bytes:
    """team_mapper.cpp:47-63: A<->T, C<->G, others unchanged."""
    return g[::-1].translate(bytes.maketrans(b"ATCG", b"TAGC"))


def expected_lines(base_lines, reads, g, gap_open=None):
    """The extended lines from the lines without the option (scoring 1 / -1 / -1, band BAND)."""
    rc, L = _revcomp(g), len(g)
    by_name = dict(reads)
    out, stats = [], dict(grew=0, reach=0, short=0, longest=0)
    for ln in base_lines:
        c = ln.split(b"\t")
        R = by_name[c[0]]
        assert len(R) == int(c[1])
        fwd = c[4] == b"+"
        S = g if fwd else rc
        qb, qe = int(c[2]), int(c[3]) - 1
        tb, te = (int(c[7]), int(c[8]) - 1) if fwd else (L - int(c[8]), L - int(c[7]) - 1)
        nr = len(R) - 1 - qe
        mr = min(L - 1 - te, nr + BAND)
        right = AR.align_full(R[qe + 1:], S[te + 1:te + 1 + mr], 1, -1, -1, BAND, gap_open=gap_open)
        nl = qb
        ml = min(tb, nl + BAND)
        left = AR.align_full(R[:qb][::-1], S[tb - ml:tb][::-1], 1, -1, -1, BAND, gap_open=gap_open)
        qb2, qe2, tb2, te2 = qb - left.gi, qe + right.gi, tb - left.gj, te + right.gj
        ts, tend = (tb2, te2 + 1) if fwd else (L - te2 - 1, L - tb2)
        score = int(c[9]) + left.score + right.score
        cigar = AR.stitch(left.cigar, c[12][5:], right.cigar)
        assert AR.consumed(cigar) == (qe2 - qb2 + 1, te2 - tb2 + 1)
        out.append(b"\t".join([c[0], c[1], b"%d" % qb2, b"%d" % (qe2 + 1), c[4], c[5], c[6], b"%d" % ts, b"%d" % tend,
                               b"%d" % score, b"%d" % (qe2 - qb2 + 1), c[11], b"cg:Z:" + cigar]))
        stats["grew"] += left.gi + right.gi > 0
        for n_end, gi in ((nl, left.gi), (nr, right.gi)):
            if n_end:
                stats["reach" if gi == n_end else "short"] += 1
            stats["longest"] = max(stats["longest"], gi)
    return out, stats


@pytest.fixture(scope="module")
def genome():
    return _records(GENOME)[0]


@pytest.fixture(scope="module", params=["r60k.fastq", "r60k.fasta"])
def run(request, genome):
    """One reads file: its lines without and with the option, and the expected lines."""
    files = [GENOME, os.path.join(MG, request.param)]
    reads = _records(files[1])
    base = _cli(BASE + files).splitlines()
    got = _cli(BASE + ["--extend-ends"] + files).splitlines()
    want, stats = expected_lines(base, reads, genome[1])
    return request.param, files, reads, base, got, want, stats


def test_cli_lines_equal_the_definition(run):
    name, _, _, base, got, want, stats = run
    assert len(got) == len(base) == len(want) > 0
    for a, b in zip(got, want):
        assert a == b, (name, a[:120], b[:120])
    print(name, "lines", len(got), stats)
    fastq = name.endswith("fastq")
    assert stats["grew"] >= (40 if fastq else 22), stats
    assert stats["short"] >= 5, stats  # natural soft clipping: ends that stop short of the read's end
    assert stats["reach"] >= 5, stats
    if not fastq:
        assert stats["longest"] > 1024, stats  # an end that crosses a pass boundary


def test_anywhere_among_the_options(run):
    _, files, _, _, got, _, _ = run
    assert _cli(["--extend-ends"] + BASE + files).splitlines() == got
    assert _cli(BASE[:2] + files + BASE[2:] + ["--extend-ends"]).splitlines() == got


def test_without_cigar_same_coordinates_and_scores(run):
    _, files, _, _, got, _, _ = run
    nocig = _cli(["-a", "global", "--band", str(BAND), "--extend-ends"] + files).splitlines()
    assert len(nocig) == len(got)
    for a, b in zip(nocig, got):
        assert a.split(b"\t") == b.split(b"\t")[:12], a


def test_python_agrees_with_the_cli(run, genome):
    _, _, reads, _, got, _, _ = run
    mp = M.Mapper(0)
    idx = M.Index(mp, genome[0].decode(), genome[1], 15, 5, 0.001)
    try:
        seqs = [s for _, s in reads]
        fastq = run[0].endswith("fastq")
        opt = M.Options.make(type=0, want_cigar=True, fastq_rules=fastq)
        res = idx.map_batch(seqs, opt, band=BAND, extend_ends=True)
        stages, _ = mp.stage_times()
        assert len(stages) == len(M.Mapper.STAGES) == 8 and stages["align"] > 0  # no stage added
        stats = mp.align_plan_stats()
        assert stats["pairs"] == int(res.mapped.sum()) == len(got) and stats["chunks"] >= 3  # three plans
        L, k = len(genome[1]), 0
        for i in range(len(seqs)):
            if not res.mapped[i]:
                continue
            c = got[k].split(b"\t")
            fwd = bool(res.strand_fwd[i])
            tb, te = int(res.t_begin[i]), int(res.t_end[i])
            ts, tend = (tb, te + 1) if fwd else (L - te - 1, L - tb)
            assert (int(c[2]), int(c[3]) - 1, int(c[7]), int(c[8])) == (int(res.q_begin[i]), int(res.q_end[i]), ts, tend), i
            assert int(c[9]) == int(res.scores[i]) and c[12][5:] == res.cigar(i), i
            k += 1
        nocig = idx.map_batch(seqs, M.Options.make(type=0, want_cigar=False, fastq_rules=fastq), band=BAND,
                              extend_ends=True)
        for f in ("mapped", "q_begin", "q_end", "t_begin", "t_end", "scores"):
            assert (getattr(nocig, f) == getattr(res, f)).all(), f
    finally:
        idx.close()
        mp.close()


def test_affine_gaps_against_the_affine_model(genome):
    files = [GENOME, os.path.join(MG, "r60k.fasta")]
    reads = _records(files[1])
    base = _cli(BASE + ["--gap-open", "-2"] + files).splitlines()
    got = _cli(BASE + ["--gap-open", "-2", "--extend-ends"] + files).splitlines()
    want, stats = expected_lines(base, reads, genome[1], gap_open=-2)
    assert len(got) == len(want) > 0
    for a, b in zip(got, want):
        assert a == b, (a[:120], b[:120])
    assert stats["grew"] >= 22, stats


def test_any_band_is_cheap_to_ask_for(genome):
    """--band 4000000000 is the full band: the same lines as any band that holds every end, and an
    arena whose size does not grow with the band."""
    files = [GENOME, os.path.join(MG, "r60k.fasta")]
    wide = _cli(["-a", "global", "-c", "--band", "4000000000", "--extend-ends"] + files)
    assert wide == _cli(["-a", "global", "-c", "--band", "70000", "--extend-ends"] + files) and wide
    mp = M.Mapper(0)
    idx = M.Index(mp, genome[0].decode(), genome[1], 15, 5, 0.001)
    try:
        seqs = [s for _, s in _records(files[1])]
        res = idx.map_batch(seqs, M.Options.make(type=0, want_cigar=True), band=4000000000, extend_ends=True)
        assert res.arena.size <= 16 * sum(len(s) for s in seqs) + 30 * len(seqs)  # 4 len + 2 + 4 (3 len + 6) + 4
        lines = wide.splitlines()
        assert int(res.mapped.sum()) == len(lines)
        got = [res.cigar(i) for i in range(len(seqs)) if res.mapped[i]]
        assert got == [ln.split(b"\t")[12][5:] for ln in lines]
    finally:
        idx.close()
        mp.close()


def test_argument_errors(genome):
    files = [GENOME, os.path.join(MG, "r60k.fasta")]
    for args in (["-a", "global", "-c", "--band", "auto", "--extend-ends"],
                 ["-a", "global", "-c", "--extend-ends"],
                 ["-a", "local", "-c", "--band", "16", "--extend-ends"],
                 ["-a", "semiGlobal", "-c", "--band", "16", "--extend-ends"],
                 ["-a", "global", "-c", "--band", "16", "--eqx", "--extend-ends"]):
        p = M.run_cli(args + files, timeout=120)
        assert p.returncode == 1 and b"--extend-ends" in p.stderr and p.stdout == b"", args
    with pytest.raises(ValueError, match="extend_ends"):
        M.map_files(files[0], files[1], extend_ends=True)
    with pytest.raises(ValueError, match="extend_ends"):
        M.map_files(files[0], files[1], band="auto", extend_ends=True)
    with pytest.raises(ValueError, match="extend_ends"):
        M.map_files(files[0], files[1], band=16, extend_ends=True, type=1)
    # the C entries themselves: TM_ERR_ARG (3) for a type other than global and for TM_MAP_EQX
    L = M.lib()
    for opt, flags in ((M.Options.make(type=1), 0), (M.Options.make(type=2), 0), (M.Options.make(type=0), M.TM_MAP_EQX)):
        r = L.tm_map_files_band_ends(files[0].encode(), files[1].encode(), C.byref(opt), b"-", 0, flags, 16, None)
        assert r == 3, (opt.type, flags, r)
    mp = M.Mapper(0)
    idx = M.Index(mp, genome[0].decode(), genome[1], 15, 5, 0.001)
    try:
        for kw in (dict(type=1), dict(type=2)):
            with pytest.raises(ValueError, match="extend_ends"):
                idx.map_batch([b"ACGT" * 20], M.Options.make(**kw), band=16, extend_ends=True)
        with pytest.raises(ValueError, match="extend_ends"):
            idx.map_batch([b"ACGT" * 20], M.Options.make(), band=16, extend_ends=True, eqx=True)
        with pytest.raises(ValueError, match="extend_ends"):
            idx.map_batch([b"ACGT" * 20], M.Options.make(), extend_ends=True)
    finally:
        idx.close()
        mp.close()
