"""The mapper's band (tm_map_batch_band, tm_map_files_band, team_mapper_amd
--band, Index.map_batch(band=...)): a band that holds every window reproduces
the committed PAF fixtures byte for byte; with a small band every CIGAR still
consumes its windows, no score is above the unbanded one, and the Python entry
agrees with the CLI."""
import json
import os

import annotate_ref as R
import pytest
from conftest import GOLDEN

from bioinfo1_amd import mapper as M

pytestmark = pytest.mark.gpu
MG = os.path.join(GOLDEN, "mapper")
FULL = "100000000"

with open(os.path.join(MG, "runs.json")) as f:
    RUNS = json.load(f)["runs"]


def _files(r):
    return [os.path.join(MG, r["genome"]), os.path.join(MG, r["reads"])]


def _cli(args):
    p = M.run_cli(args, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout


# a FASTA and a FASTQ run with -c, a local one with its own scoring, and the demo
@pytest.mark.parametrize("run", [0, 1, 6, 7])
def test_full_band_reproduces_the_paf_fixtures(run):
    r = RUNS[run]
    assert "-c" in r["args"]
    want = open(os.path.join(MG, r["paf"]), "rb").read()
    assert _cli(["--band", FULL] + r["args"] + _files(r)) == want
    assert _cli(r["args"] + _files(r) + ["--band", FULL]) == want  # accepted anywhere among the options


def test_full_band_with_eqx():
    r = RUNS[1]
    plain = _cli(["--eqx"] + r["args"] + _files(r))
    assert _cli(["--eqx", "--band", FULL] + r["args"] + _files(r)) == plain
    want = open(os.path.join(MG, r["paf"]), "rb").read().splitlines()
    for a, b in zip(want, plain.splitlines()):
        ca, cb = a.split(b"\t"), b.split(b"\t")
        assert ca[:12] == cb[:12] and R.collapse(cb[12][5:]) == ca[12][5:]


def test_band_argument_errors():
    r = RUNS[7]
    for bad in (["--band", "x"], ["--band", "-3"], ["--band", "4294967296"]):
        p = M.run_cli(bad + r["args"] + _files(r), timeout=120)
        assert p.returncode == 1 and b"--band" in p.stderr


def _check_lines(r, band):
    """The banded CLI lines beside the unbanded ones: same windows, CIGARs that
    consume them, scores never above."""
    plain = open(os.path.join(MG, r["paf"]), "rb").read().splitlines()
    got = _cli(r["args"] + ["--band", str(band)] + _files(r)).splitlines()
    assert len(got) == len(plain) > 0
    local = "local" in r["args"]
    changed = 0
    for a, b in zip(plain, got):
        ca, cb = a.split(b"\t"), b.split(b"\t")
        assert ca[:9] == cb[:9] and ca[10:12] == cb[10:12]
        assert int(cb[9]) <= int(ca[9])
        ops = R.ops_of(cb[12][5:])
        nq, nt = int(cb[3]) - int(cb[2]), int(cb[8]) - int(cb[7])
        cq, ct = sum(o in "MD" for o in ops), sum(o in "MI" for o in ops)
        assert (cq <= nq and ct <= nt) if local else (cq == nq and ct == nt), b
        changed += ca[12] != cb[12]
    return got, changed


@pytest.mark.parametrize("run", [7, 8, 9])
def test_small_band_on_the_demo_files(run):
    _check_lines(RUNS[run], 1)
    _check_lines(RUNS[run], 0)


def test_small_band_on_long_reads_and_python_agrees():
    r = RUNS[0]  # g60k / r60k.fasta, semi-global, -c
    got, changed = _check_lines(r, 4)
    assert changed > 0  # the band binds on some windows
    def fasta(fn):
        recs, cur = [], None
        for ln in open(fn, "rb").read().splitlines():
            if ln.startswith(b">"):
                cur = [ln[1:].split()[0], b""]
                recs.append(cur)
            elif cur is not None:
                cur[1] += ln.strip()
        return recs

    (name, g), reads = fasta(_files(r)[0])[0], [s for _, s in fasta(_files(r)[1])]
    mp = M.Mapper(0)
    idx = M.Index(mp, name.decode(), g, 15, 5, 0.001)
    opt = M.Options.make(type=2, want_cigar=True)
    res = idx.map_batch(reads, opt, band=4)
    st = mp.align_plan_stats()
    assert st["pairs"] == int(res.mapped.sum()) == len(got) and st["chunks"] >= 1
    assert st["dual_pairs"] == 0 and st["flex_pairs"] == 0 and st["workspace_bytes"] > 0
    k = 0
    for i in range(len(reads)):
        if not res.mapped[i]:
            continue
        cols = got[k].split(b"\t")
        assert int(cols[9]) == int(res.scores[i]) and cols[12][5:] == res.cigar(i), i
        k += 1
    # the =/X form of the same banded alignments
    x = idx.map_batch(reads, opt, eqx=True, band=4)
    for i in range(len(reads)):
        if res.mapped[i]:
            assert R.collapse(x.cigar(i)) == res.cigar(i) and int(x.scores[i]) == int(res.scores[i])
    # no band: the reference-exact plan still runs (its packed fills take the pairs)
    base = idx.map_batch(reads, opt)
    assert (res.scores <= base.scores).all()
    idx.close()
    mp.close()
