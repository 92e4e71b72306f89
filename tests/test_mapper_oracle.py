"""The CPU restatement of the mapper stages (oracle/pymapper.py) is pinned to
the reference: minimizers.json was produced by the reference's own
team::KMER::Minimize (compiled from /root/reference into oracle/_ref by
oracle/Makefile, tests/golden/make_mapper_golden.py); where oracle/_ref is
built, fresh random sequences and hit lists are compared too."""
import json
import os
import random

import pytest
from conftest import GOLDEN

from oracle import pymapper as pm

MG = os.path.join(GOLDEN, "mapper")


def minimizer_cases():
    with open(os.path.join(MG, "minimizers.json")) as f:
        return json.load(f)["cases"]


def test_minimize_matches_reference_fixtures():
    cases = minimizer_cases()
    assert len(cases) > 300
    for c in cases:
        s = c["seq"].encode("latin1")
        got = pm.minimize(s, c["k"], c["w"], c["is_fwd"])
        want = list(zip(c["hash"], c["pos"], [bool(x) for x in c["strand"]]))
        assert got == want, (c["source"], c["k"], c["w"])
        assert len(set(want)) == c["n_unique"]


def test_mapper_fixtures_present():
    with open(os.path.join(MG, "runs.json")) as f:
        runs = json.load(f)["runs"]
    assert len(runs) >= 9
    for r in runs:
        assert os.path.exists(os.path.join(MG, r["paf"]))
        assert open(os.path.join(MG, r["paf"]), "rb").read().count(b"\n") == r["lines"]


def test_slide17_published_paf_fixture():
    """run9 is the reference's published mapper run (pptx slide 16/17,
    `-a local -m 2 -n -1 -g 2 -k 3 -w 2 -c ref.fasta seq.fasta.txt`): its PAF
    fixture holds the two published lines literally."""
    with open(os.path.join(MG, "runs.json")) as f:
        r = [x for x in json.load(f)["runs"] if x["genome"] == "demo_ref9.fasta"][0]
    assert r["args"] == ["-a", "local", "-m", "2", "-n", "-1", "-g", "2", "-k", "3", "-w", "2", "-c"]
    lines = open(os.path.join(MG, r["paf"]), "rb").read().splitlines()
    assert b"seq1\t6\t1\t6\t-\tref\t9\t0\t5\t18\t5\t60\tcg:Z:1M4D4I" in lines
    assert b"seq2\t7\t0\t5\t+\tref\t9\t3\t8\t18\t5\t60\tcg:Z:1M4D4I" in lines
    if pm.RefMapper.available():  # the reference build (oracle/_ref/ref_mapper) reproduces the fixture
        import subprocess

        res = subprocess.run([pm.REF_MAPPER_BIN] + r["args"] + [os.path.join(MG, r["genome"]),
                                                                os.path.join(MG, r["reads"])],
                             capture_output=True, check=True, timeout=60)
        assert res.stdout.splitlines() == lines


def edge_runs():
    with open(os.path.join(MG, "edge_runs.json")) as f:
        return json.load(f)


def read_fastx(path):
    """[(name, seq)] of a fixture written by make_mapper_golden.py (FASTA or 4-line FASTQ)."""
    lines = open(path, "rb").read().split(b"\n")
    if path.endswith(".fastq"):
        return [(lines[i][1:].split()[0].decode(), lines[i + 1]) for i in range(0, len(lines) - 1, 4)]
    out = []
    for line in lines:
        if line.startswith(b">"):
            out.append([line[1:].split()[0].decode(), b""])
        elif line:
            out[-1][1] += line
    return [(n, s) for n, s in out]


def paf_rows(path):
    """{read: columns} of a PAF fixture (one line per read at most)."""
    rows = {}
    for line in open(path, "rb").read().splitlines():
        c = line.split(b"\t")
        assert c[0].decode() not in rows
        rows[c[0].decode()] = c
    return rows


def test_edge_fixtures_present():
    e = edge_runs()
    assert len(e["runs"]) >= 12
    g = read_fastx(os.path.join(MG, "gedge.fasta"))
    assert len(g) == 2 and len(g[0][1]) == e["genome_length"]  # the second record is a decoy
    for r in e["runs"]:
        paf = open(os.path.join(MG, r["paf"]), "rb").read()
        assert paf.count(b"\n") == r["lines"] > 0
        assert len(read_fastx(os.path.join(MG, r["reads"]))) == r["n_reads"]
    for name in os.listdir(MG):  # no new file is larger than g60k.fasta
        if "edge" in name:
            assert os.path.getsize(os.path.join(MG, name)) <= os.path.getsize(os.path.join(MG, "g60k.fasta")), name
    args = [" ".join(r["args"]) for r in e["runs"]]
    assert "" in args and any("-w 64" in a for a in args) and any("-k 5 -w 1 -f 0" in a for a in args)
    assert any("-f 0.2" in a for a in args) and any("-m 2 -n -3 -g -2" in a for a in args)
    assert any(a.endswith("-g 2") for a in args)
    for t in ("local", "global", "semiGlobal"):
        assert {"-c" in r["args"] for r in e["runs"] if r["args"][:2] == ["-a", t]} == {True, False}, t


@pytest.mark.skipif(not pm.RefMapper.available(), reason="oracle/_ref not built (reference sources absent)")
def test_edge_fixtures_reproduced_by_reference_build():
    import subprocess

    for r in edge_runs()["runs"]:
        res = subprocess.run([pm.REF_MAPPER_BIN] + r["args"] + [os.path.join(MG, r["genome"]),
                                                                os.path.join(MG, r["reads"])],
                             capture_output=True, check=True, timeout=120)
        assert res.stdout == open(os.path.join(MG, r["paf"]), "rb").read(), r["paf"]


def test_edge_family_contains_what_it_claims():
    """Read off the committed inputs and PAFs: the strand, boundary, gap and
    tie cases the family was built for are there."""
    e = edge_runs()
    L = e["genome_length"]
    g = read_fastx(os.path.join(MG, "gedge.fasta"))[0][1]
    seg = e["segments"]
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    # the genome: unique ends, a segment and its reverse complement, tandem, homopolymer, N run, lowercase
    q = g[seg["q"][0]:seg["q"][1]]
    assert g[seg["q_rc"][0]:seg["q_rc"][1]] == q[::-1].translate(rc) and len(q) >= 600
    t = g[seg["tandem"][0]:seg["tandem"][1]]
    assert len(t) >= 2900 and t[7:] == t[:-7]
    assert g[seg["homopolymer"][0]:seg["homopolymer"][1]] == b"A" * 200
    assert g[seg["n_run"][0]:seg["n_run"][1]] == b"N" * 50
    low = g[seg["lower"][0]:seg["lower"][1]]
    assert low and low == low.lower() and low != low.upper()
    assert g.count(g[:300]) == 1 and g.count(g[-300:]) == 1
    for r in e["runs"]:
        k = int(r["args"][r["args"].index("-k") + 1]) if "-k" in r["args"] else 15
        w = int(r["args"][r["args"].index("-w") + 1]) if "-w" in r["args"] else 5
        reads = dict(read_fastx(os.path.join(MG, r["reads"])))
        rows = paf_rows(os.path.join(MG, r["paf"]))
        for n in [L] + [len(s) for s in reads.values()]:
            assert not (k <= n < w + k - 2), (r["paf"], n)
        # reads below k, of w+k-2 and w+k-1 bases (and of k bases where [k, w+k-2) is empty)
        lens = {len(s) for s in reads.values()}
        assert min(lens) < k and {w + k - 2, w + k - 1} <= lens and (w > 2 or k in lens)
        # a read with no line in every run
        assert set(rows) < set(reads) and "below_k" not in rows, r["paf"]
        if k == 15:
            assert "unrelated" not in rows, r["paf"]
        # exact substrings: the reads at either end of the genome, as read and reverse-complemented
        assert reads["fwd_start"] == g[:400] and reads["rc_end"] == g[-400:][::-1].translate(rc)
        assert rows["fwd_start"][4] == b"+" and int(rows["fwd_start"][7]) == 0
        assert rows["fwd_end"][4] == b"+" and int(rows["fwd_end"][8]) == L
        if r["reads"].endswith(".fastq"):  # FASTA rules take reverse hits only for hashes of the forward index
            assert rows["rc_start"][4] == b"-" and int(rows["rc_start"][7]) == 0
            assert rows["rc_end"][4] == b"-" and int(rows["rc_end"][8]) == L
        # the palindrome is a strand tie: '+' wins
        assert rows["palindrome"][4] == b"+", r["paf"]
        # the gap next to the 5,000 limit.  Two hits chain if their reference
        # positions differ by less than 5,000, and the k-mers on either side of
        # the junction start at least k apart: with k = 15 a skip of 4,970 bases
        # still chains, 4,990 (+15) and 5,010 do not; with k = 5 and -f 0 random
        # 5-mer hits bridge every gap.
        span = {s: int(rows[f"skip{s}"][3]) - int(rows[f"skip{s}"][2]) for s in (4970, 4990, 5010)}
        if k == 15 and w == 5:
            assert span[4970] >= 590 and int(rows["skip4970"][8]) - int(rows["skip4970"][7]) >= 590 + 4970
            assert span[4990] <= 300 and span[5010] <= 300, r["paf"]
        if k == 5:
            assert span[4990] == 600
    # FASTA and FASTQ rules differ on the same reads and options
    for r in e["runs"]:
        if r["reads"] == "redge.fastq":
            rows = paf_rows(os.path.join(MG, r["paf"]))
            assert sum(c[4] == b"-" for c in rows.values()) >= 3
    a, b = paf_rows(os.path.join(MG, "edge10.paf")), paf_rows(os.path.join(MG, "edge13.paf"))
    assert e["runs"][10]["reads"] == "redge.fasta" and e["runs"][13]["reads"] == "redge.fastq"
    fasta_vs_fastq = [n for n in b if n not in a or a[n][:12] != b[n][:12]]
    assert "rc_start" in fasta_vs_fastq and "rc_mid" in fasta_vs_fastq
    # nothing banned: the tandem read maps (its forward hit list passes 12,288: asserted by the generator)
    assert "tandem1500" in b and "tandem1500" not in a


@pytest.mark.skipif(not pm.RefMapper.available(), reason="oracle/_ref not built (reference sources absent)")
def test_restatement_vs_reference_fuzz():
    ref = pm.RefMapper()
    rng = random.Random(77)
    for t in range(300):
        L = rng.randint(0, 80)
        alpha = rng.choice([b"ACGT", b"AC", b"ACGTN", b"acgtACGT", b"G"])
        s = bytes(rng.choice(alpha) for _ in range(L))
        k, w = rng.randint(1, 16), rng.randint(1, 9)
        if L >= k and L < w + k - 2:
            continue  # the reference reads past the end of its string there (UB)
        for fwd in (True, False):
            m, u = ref.minimize(s, k, w, fwd)
            assert pm.minimize(s, k, w, fwd) == m, (s, k, w)
            assert len(set(m)) == u
    for t in range(200):
        n = rng.randint(0, 60)
        hits = [(rng.randint(1, 12000), rng.randint(1, 12000)) for _ in range(n)]
        if t % 2:
            hits.sort(key=lambda h: h[0])
        assert pm.find_lis(hits) == ref.find_lis(hits)
