#!/usr/bin/env python3
"""Device time of the anchored plan with z-drop beside the same plan with z-drop
off (whose kernels are the parent commit's), and the mapper's wall time with
and without --zdrop.

(a) Overhead when nothing drops: scripts/anchored_time.py's four lines -- whole
    related pairs at 1/-1/-1, CIGAR on -- with Z = 2^31 - 1, which never fires.
(b) Dying ends: 4,096 pairs of 2,000 x 2,064 at 2/-4/-4, w = 64, Z = 100; a
    related prefix of 100 / 500 / 1,000 / 2,000 bases (synth.related_batch),
    then unrelated bases (synth.uniform_batch); linear gaps, and affine gaps
    (open -4, extend -2).  Time on / off beside the sum of swept_steps on / off.
Method (anchored_time.py's): the two plans of a line live in this process on
one context; after WARMUP executions each they are timed alternately, REPS
executions each, one HIP event pair around one execution; a figure is the
median of the REPS; three repeats: per plan the three medians, their median
and their spread (max - min).
(c) The mapper: anchored_time.py's 3,000 ONT-like reads, map_files at -a global
    -c -m 2 -n -4 -g -4 --band 64 --extend-ends with and without --zdrop 100:
    wall time (once to warm up, then the median of three each, alternately), the
    share of reads whose line changed, and -- from the windows of the same
    command without --extend-ends, the ends rebuilt on the host and run through
    ta_align_batch_anchored_zdrop -- the share of non-empty ends that dropped.

Writes profiles/bench/anchored_zdrop_time.json and prints it.  Not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEVER = (1 << 31) - 1


def total_steps(n, m, w):
    """The fill steps of a pair that does not drop (ta_layout.h band_drop_steps over its passes)."""
    if n == 0 or m == 0:
        return 0
    w = min(w, max(n, m))
    lo, hi = min(0, m - n) - w, max(0, m - n) + w
    steps = 0
    for p in range((n + 1023) // 1024):
        rows = min(1024, n - 1024 * p)
        c0, c1 = max(1, 1024 * p + 1 + lo), min(m, 1024 * p + rows + hi)
        steps += c1 - c0 + 1 + (rows + 15) // 16 - 1
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs-10k", type=int, default=4096)
    ap.add_argument("--pairs-32k", type=int, default=2048)
    ap.add_argument("--pairs-ends", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mapper-reads", type=int, default=3000)
    ap.add_argument("--skip", default="", help="comma list of parts to skip: a, b, c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench", "anchored_zdrop_time.json"))
    a = ap.parse_args()
    skip = set(a.skip.split(","))

    import numpy as np
    import torch

    from bioinfo1_amd import mapper as M
    from bioinfo1_amd import synth
    from bioinfo1_amd.align import Aligner, DevicePlan

    al = Aligner(0)

    def once(plan):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def time_pair(off, on):
        """-> per plan (median of the repeats' medians, the medians, their spread)."""
        plans = {"off": off, "on": on}
        meds = {k: [] for k in plans}
        for _ in range(a.repeats):
            for _ in range(a.warmup):
                for p in plans.values():
                    once(p)
            t = {k: [] for k in plans}
            for _ in range(a.reps):  # alternately, in the same process
                for k, p in plans.items():
                    t[k].append(once(p))
            for k in plans:
                meds[k].append(statistics.median(t[k]))
        for p in plans.values():
            p.check()
        out = {}
        for k in plans:
            out[k + "_ms"] = round(statistics.median(meds[k]), 3)
            out[k + "_medians_ms"] = [round(x, 3) for x in meds[k]]
            out[k + "_spread_ms"] = round(max(meds[k]) - min(meds[k]), 3)
        out["on_over_off"] = round(out["on_ms"] / out["off_ms"], 4)
        out["beyond_off_spread"] = bool(abs(out["on_ms"] - out["off_ms"]) > out["off_spread_ms"])
        return out

    # ---- (a) nothing drops
    overhead = []
    shapes = ((10000, a.pairs_10k, (128, 512), 0), (32768, a.pairs_32k, (512,), 0), (10000, a.pairs_10k, (512,), -3))
    batch, last = None, None
    for length, pairs, bands, gap_open in shapes if "a" not in skip else ():
        if (length, pairs) != last:
            batch = synth.related_batch(pairs, length, length, 0x5EED)
            last = (length, pairs)
        inputs = None
        for w in bands:
            off = DevicePlan.anchored(al, batch, 1, -1, -1, w, gap_open=gap_open, inputs=inputs)
            inputs = (off.qbytes, off.qoff, off.tbytes, off.toff)
            on = DevicePlan.anchored(al, batch, 1, -1, -1, w, gap_open=gap_open, inputs=inputs, zdrop=NEVER)
            line = {"shape": f"{pairs} pairs {length} x {length}, 1/-1/-1, CIGAR, related 0x5EED", "band": w,
                    "gap_open": gap_open, "zdrop": NEVER, "band_cells": off.band_cells}
            line.update(time_pair(off, on))
            steps = on.swept_steps()
            line["every_step_swept"] = bool(int(steps.astype(np.uint64).sum()) == sum(
                total_steps(int(batch.qlen[p]), int(batch.tlen[p]), w) for p in range(batch.n_pairs)))
            line["same_scores"] = bool((on.results().scores == off.results().scores).all())
            overhead.append(line)
            print(json.dumps(line), flush=True)
            off.close()
            on.close()
        al.release()
        torch.cuda.empty_cache()

    # ---- (b) dying ends
    dying = []
    P, n, m, w, z = a.pairs_ends, 2000, 2064, 64, 100
    for L in (100, 500, 1000, 2000) if "b" not in skip else ():
        c = synth.related_batch(P, L, L, 0x2D20 + L)
        u = synth.uniform_batch(P, n - L, m - L, seed=0x2D21 + L)
        batch = synth.from_pairs([(c.query(p) + u.query(p), c.target(p) + u.target(p)) for p in range(P)])
        assert (batch.qlen == n).all() and (batch.tlen == m).all()
        inputs = None
        for name, sc, gap_open in (("linear", (2, -4, -4), 0), ("affine", (2, -4, -2), -4)):
            off = DevicePlan.anchored(al, batch, *sc, w, gap_open=gap_open, inputs=inputs)
            inputs = (off.qbytes, off.qoff, off.tbytes, off.toff)
            on = DevicePlan.anchored(al, batch, *sc, w, gap_open=gap_open, inputs=inputs, zdrop=z)
            line = {"shape": f"{P} pairs {n} x {m}, related prefix {L}, then unrelated", "prefix": L, "gaps": name,
                    "scoring": list(sc) + [gap_open], "band": w, "zdrop": z}
            line.update(time_pair(off, on))
            steps = on.swept_steps().astype(np.uint64)
            all_steps = P * total_steps(n, m, w)
            line["steps_on"], line["steps_off"] = int(steps.sum()), all_steps
            line["steps_on_over_off"] = round(int(steps.sum()) / all_steps, 4)
            line["pairs_dropped_share"] = round(float((steps < total_steps(n, m, w)).mean()), 4)
            r_on, r_off = on.results(), off.results()
            line["same_scores_share"] = round(float((r_on.scores == r_off.scores).mean()), 4)
            # fill and walk apart, once each (the walk is the floor a drop cannot lower)
            torch.cuda.synchronize()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for plan, key in ((off, "off"), (on, "on")):
                e[0].record()
                for ch in range(plan.chunks):
                    plan.run_fill(ch)
                e[1].record()
                for ch in range(plan.chunks):
                    plan.run_traceback(ch)
                e[2].record()
                e[2].synchronize()
                line[key + "_fill_ms_once"] = round(e[0].elapsed_time(e[1]), 3)
                line[key + "_walk_ms_once"] = round(e[1].elapsed_time(e[2]), 3)
            dying.append(line)
            print(json.dumps(line), flush=True)
            off.close()
            on.close()
        al.release()
        torch.cuda.empty_cache()

    # ---- (c) the mapper, on files
    mapper = {}
    if "c" not in skip:
        g = synth.genome(synth.ECOLI_LEN)
        rs = synth.ont_reads(a.mapper_reads, g)
        sc = dict(type=0, match=2, mismatch=-4, gap=-4, want_cigar=True)
        with tempfile.TemporaryDirectory() as tmp:
            ref, reads = os.path.join(tmp, "ref.fasta"), os.path.join(tmp, "reads.fasta")
            with open(ref, "wb") as f:
                f.write(b">genome\n" + g.tobytes() + b"\n")
            with open(reads, "wb") as f:
                for r in range(rs.n_reads):
                    f.write(b">r%d\n" % r + rs.read(r) + b"\n")
            outs = {None: os.path.join(tmp, "ends.paf"), 100: os.path.join(tmp, "z.paf")}

            def run(zd):
                t0 = time.perf_counter()
                M.map_files(ref, reads, out=outs[zd], band=64, extend_ends=True, zdrop=zd, **sc)
                return time.perf_counter() - t0

            run(None)
            run(100)
            t = {None: [], 100: []}
            for _ in range(3):
                for zd in (None, 100):
                    t[zd].append(run(zd))
            plain = open(outs[None], "rb").read().splitlines()
            zl = open(outs[100], "rb").read().splitlines()
            assert len(plain) == len(zl)
            changed = sum(x != y for x, y in zip(plain, zl))
            shorter = sum(int(y.split(b"\t")[10]) < int(x.split(b"\t")[10]) for x, y in zip(plain, zl))
            # the ends, rebuilt from the windows of the command without --extend-ends
            win = os.path.join(tmp, "win.paf")
            M.map_files(ref, reads, out=win, band=64, **sc)
            gb = g.tobytes()
            rc, GL = gb[::-1].translate(bytes.maketrans(b"ATCG", b"TAGC")), len(gb)
            ends = []
            for ln in open(win, "rb").read().splitlines():
                col = ln.split(b"\t")
                R = rs.read(int(col[0][1:]))
                fwd = col[4] == b"+"
                S = gb if fwd else rc
                qb, qe = int(col[2]), int(col[3]) - 1
                tb, te = (int(col[7]), int(col[8]) - 1) if fwd else (GL - int(col[8]), GL - int(col[7]) - 1)
                nr = len(R) - 1 - qe
                ends.append((R[qe + 1:], S[te + 1:te + 1 + min(GL - 1 - te, nr + 64)]))
                ends.append((R[:qb][::-1], S[tb - min(tb, qb + 64):tb][::-1]))
            ends = [(q, s) for q, s in ends if q and s]
            eb = synth.from_pairs(ends)
            res = al.align_batch_anchored(eb, 2, -4, -4, 64, want_cigar=False, zdrop=100)
            full = np.array([total_steps(len(q), len(s), 64) for q, s in ends], np.uint64)
            mapper = {"reads": rs.n_reads, "read_bases": int(rs.len.sum()), "mapped": len(plain),
                      "command": "-a global -c -m 2 -n -4 -g -4 --band 64 --extend-ends [--zdrop 100]",
                      "extend_ends_wall_s": round(statistics.median(t[None]), 3),
                      "extend_ends_walls_s": [round(x, 3) for x in t[None]],
                      "zdrop_wall_s": round(statistics.median(t[100]), 3), "zdrop_walls_s": [round(x, 3) for x in t[100]],
                      "lines_changed_share": round(changed / max(len(plain), 1), 4),
                      "lines_shorter_share": round(shorter / max(len(plain), 1), 4),
                      "nonempty_ends": len(ends),
                      "ends_dropped_share": round(float((res.swept_steps < full).mean()), 4),
                      "ends_steps_on_over_off": round(int(res.swept_steps.astype(np.uint64).sum()) / max(int(full.sum()), 1), 4)}
            print(json.dumps(mapper), flush=True)
    al.close()

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "repeats": a.repeats,
           "overhead_when_nothing_drops": overhead, "dying_ends": dying, "mapper": mapper}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
