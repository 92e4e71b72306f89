"""The mapper's TM_MAP_EQX flag (tm_map_batch_x, tm_map_files_x, team_mapper_amd
--eqx) on the demo fixtures: flags 0 is tm_map_batch, the extended CIGARs
collapse to the base ones, the info records match the test-side reference
(tests/annotate_ref.py) on each read's windows, and the CLI lines are the plain
ones with cg:Z: extended and NM:i: appended."""
import ctypes as C
import os

import annotate_ref as R
import numpy as np
import pytest
from conftest import GOLDEN

from bioinfo1_amd import mapper as M
from bioinfo1_amd import synth
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.gpu
MG = os.path.join(GOLDEN, "mapper")
# (genome, reads, CLI arguments, the same as tm_options): runs 7-9 of runs.json
DEMOS = [("demo.fasta", "demo_reads.fasta", ["-k", "3", "-w", "2"], dict(type=0, k=3, w=2)),
         ("demo.fasta", "demo_reads.fasta", ["-a", "local", "-k", "4", "-w", "3"], dict(type=1, k=4, w=3)),
         ("demo_ref9.fasta", "demo_reads.fasta", ["-a", "local", "-m", "2", "-n", "-1", "-g", "2", "-k", "3", "-w", "2"],
          dict(type=1, match=2, mismatch=-1, gap=2, k=3, w=2)),
         ("demo.fasta", "demo_reads.fasta", ["-a", "semiGlobal", "-k", "3", "-w", "2"], dict(type=2, k=3, w=2))]


def _fasta(name):
    recs, cur = [], None
    for ln in open(os.path.join(MG, name), "rb").read().splitlines():
        if ln.startswith(b">"):
            cur = [ln[1:].split()[0], b""]
            recs.append(cur)
        elif cur is not None:
            cur[1] += ln.strip()
    return recs


@pytest.fixture(scope="module")
def mp():
    return M.Mapper(0)


@pytest.mark.parametrize("demo", range(len(DEMOS)))
def test_map_batch_x(mp, demo):
    genome, reads_f, _, o = DEMOS[demo]
    name, g = _fasta(genome)[0]
    reads = [s for _, s in _fasta(reads_f)]
    idx = M.Index(mp, name.decode(), g, o["k"], o["w"], 0.001)
    opt = M.Options.make(want_cigar=True, **o)
    base = idx.map_batch(reads, opt)
    # flags 0, no info: tm_map_batch in every output
    L = M.lib()
    b, off, ln = M._soa(reads)
    n = len(ln)
    out = [np.zeros(n, t) for t in (np.uint8, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32, np.int32)]
    arena = np.zeros(len(base.arena), np.uint8)
    co, cl = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    r = L.tm_map_batch_x(mp._h, idx._h, n, b.ctypes.data, off.ctypes.data_as(C.POINTER(C.c_uint64)),
                         ln.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(opt),
                         *[a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in out[:2]],
                         *[a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in out[2:6]],
                         out[6].ctypes.data_as(C.POINTER(C.c_int32)), arena.ctypes.data, len(arena),
                         co.ctypes.data_as(C.POINTER(C.c_uint64)), cl.ctypes.data_as(C.POINTER(C.c_uint32)), 0, None)
    assert r == 0
    for a, w in zip(out, (base.mapped, base.strand_fwd, base.q_begin, base.q_end, base.t_begin, base.t_end,
                          base.scores)):
        np.testing.assert_array_equal(a, w)
    np.testing.assert_array_equal(cl, base.cigar_len)
    np.testing.assert_array_equal(co, base.cigar_off)
    assert arena.tobytes() == base.arena.tobytes()
    # TM_MAP_EQX
    x = idx.map_batch(reads, opt, eqx=True)
    for f in ("mapped", "strand_fwd", "q_begin", "q_end", "t_begin", "t_end", "scores"):
        np.testing.assert_array_equal(getattr(x, f), getattr(base, f))
    nocig = idx.map_batch(reads, M.Options.make(want_cigar=False, **o), eqx=True)  # records without -c
    assert nocig.info.tobytes() == x.info.tobytes()
    oracle = Oracle()
    rc = synth.reverse_complement(np.frombuffer(g, np.uint8)).tobytes()
    sc = (opt.match, opt.mismatch, opt.gap)
    assert base.mapped.any()
    for i, read in enumerate(reads):
        if not base.mapped[i]:
            assert x.info[i].tobytes() == bytes(40)
            continue
        assert R.collapse(x.cigar(i)) == base.cigar(i), i
        qw = read[int(base.q_begin[i]):int(base.q_end[i]) + 1]
        tw = (g if base.strand_fwd[i] else rc)[int(base.t_begin[i]):int(base.t_end[i]) + 1]
        score, cig, tb = oracle.align(qw, tw, o["type"], *sc)
        assert (score, cig) == (int(base.scores[i]), base.cigar(i))
        gi, gj = R.pin(qw, tw, o["type"], sc, None, cig, score, tb)
        info, eqx = R.expected(qw, tw, o["type"], cig, gi, gj)
        assert {f: int(x.info[f][i]) for f in R.FIELDS} == info, i
        assert x.cigar(i) == eqx, i
    idx.close()


@pytest.mark.parametrize("demo", range(len(DEMOS)))
def test_cli_eqx(demo):
    genome, reads_f, args, _ = DEMOS[demo]
    files = [os.path.join(MG, genome), os.path.join(MG, reads_f)]
    plain = M.run_cli(args + ["-c"] + files, timeout=120)
    nocig = M.run_cli(args + files, timeout=120)
    assert plain.returncode == 0 and nocig.returncode == 0, plain.stderr.decode()
    for eargs in (["--eqx", "-c"] + args + files, args + ["-c"] + files + ["--eqx"]):  # accepted anywhere
        ext = M.run_cli(eargs, timeout=120)
        assert ext.returncode == 0, ext.stderr.decode()
        pl, el = plain.stdout.splitlines(), ext.stdout.splitlines()
        assert len(pl) == len(el) > 0
        for a, b in zip(pl, el):
            ca, cb = a.split(b"\t"), b.split(b"\t")
            assert ca[:12] == cb[:12] and len(cb) == 14
            assert cb[12].startswith(b"cg:Z:") and cb[13].startswith(b"NM:i:")
            x = cb[12][5:]
            assert R.collapse(x) == ca[12][5:]
            ops = R.ops_of(x)
            assert int(cb[13][5:]) <= sum(o in "XID" for o in ops)  # free ends are not edits
            if "semiGlobal" not in args:
                assert int(cb[13][5:]) == sum(o in "XID" for o in ops)
    # without -c: the plain line plus the tag
    ext = M.run_cli(["--eqx"] + args + files, timeout=120)
    assert ext.returncode == 0
    for a, b, c in zip(nocig.stdout.splitlines(), ext.stdout.splitlines(), el):
        assert b == a + b"\t" + c.split(b"\t")[13]
