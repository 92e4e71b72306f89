#!/usr/bin/env python3
"""Device time of the anchored plan under the row-stripe z-drop rule beside the
same plan with z-drop off (whose kernels are the parent commit's) and under the
segment rule, and the mapper's wall time under either rule.

(a) Overhead when nothing drops: scripts/anchored_time.py's four lines -- whole
    related pairs at 1/-1/-1, CIGAR on -- with Z = 2^31 - 1, which never fires.
(b) Dying ends: scripts/anchored_zdrop_time.py's eight lines -- 4,096 pairs of
    2,000 x 2,064 at 2/-4/-4, w = 64, Z = 100; a related prefix of 100 / 500 /
    1,000 / 2,000 bases, then unrelated bases; linear gaps, and affine gaps
    (open -4, extend -2).  Time beside the sum of swept_steps, per rule; the
    steps of the first pairs of every line are also predicted by the two
    references (tests/anchored_zdrop_ref.py, tests/anchored_zdrop_stripe_ref.py)
    and compared exactly.
Method (anchored_zdrop_time.py's): the three plans of a line live in this
process on one context; after WARMUP executions each they are timed in turn,
REPS executions each, one HIP event pair around one execution; a figure is the
median of the REPS; three repeats: per plan the three medians, their median and
their spread (max - min).
(c) The mapper: anchored_time.py's 3,000 ONT-like reads, map_files at -a global
    -c -m 2 -n -4 -g -4 --band 64 --extend-ends, without --zdrop and with
    --zdrop 100 under either rule: wall time (once to warm up, then the median
    of three each, in turn), the share of lines that change against the run
    without --zdrop, and -- from the windows of the same command without
    --extend-ends, the ends rebuilt on the host -- the share of non-empty ends
    that stop early.

Writes profiles/bench/anchored_zdrop_stripe_time.json and prints it.  Not part of bench.py.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEVER = (1 << 31) - 1
RULES = ("segment", "stripe")


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
    ap.add_argument("--ref-pairs", type=int, default=16, help="pairs per line of (b) predicted by the references")
    ap.add_argument("--skip", default="", help="comma list of parts to skip: a, b, c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench", "anchored_zdrop_stripe_time.json"))
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

    def time_plans(plans):
        """plans: {"off", "segment", "stripe"} -> per plan (median of the repeats' medians, the medians, their spread)."""
        meds = {k: [] for k in plans}
        for _ in range(a.repeats):
            for _ in range(a.warmup):
                for p in plans.values():
                    once(p)
            t = {k: [] for k in plans}
            for _ in range(a.reps):  # in turn, in the same process
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
        for k in RULES:
            out[k + "_over_off"] = round(out[k + "_ms"] / out["off_ms"], 4)
        out["stripe_minus_segment_ms"] = round(out["stripe_ms"] - out["segment_ms"], 3)
        out["stripe_beyond_segment_by_more_than_off_spread"] = bool(
            out["stripe_ms"] - out["segment_ms"] > out["off_spread_ms"])
        return out

    def three_plans(batch, sc, w, gap_open, z, inputs):
        off = DevicePlan.anchored(al, batch, *sc, w, gap_open=gap_open, inputs=inputs)
        inputs = (off.qbytes, off.qoff, off.tbytes, off.toff)
        plans = {"off": off}
        for rule in RULES:
            plans[rule] = DevicePlan.anchored(al, batch, *sc, w, gap_open=gap_open, inputs=inputs, zdrop=z,
                                              zdrop_rule=rule)
        return plans, inputs

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
            plans, inputs = three_plans(batch, (1, -1, -1), w, gap_open, NEVER, inputs)
            line = {"shape": f"{pairs} pairs {length} x {length}, 1/-1/-1, CIGAR, related 0x5EED", "band": w,
                    "gap_open": gap_open, "zdrop": NEVER, "band_cells": plans["off"].band_cells}
            line.update(time_plans(plans))
            want = sum(total_steps(int(batch.qlen[p]), int(batch.tlen[p]), w) for p in range(batch.n_pairs))
            off_scores = plans["off"].results().scores
            for rule in RULES:
                line[rule + "_every_step_swept"] = bool(int(plans[rule].swept_steps().astype(np.uint64).sum()) == want)
                line[rule + "_same_scores"] = bool((plans[rule].results().scores == off_scores).all())
            overhead.append(line)
            print(json.dumps(line), flush=True)
            for p in plans.values():
                p.close()
        al.release()
        torch.cuda.empty_cache()

    # ---- (b) dying ends
    import anchored_zdrop_ref as ZR
    import anchored_zdrop_stripe_ref as SR

    dying = []
    P, n, m, w, z = a.pairs_ends, 2000, 2064, 64, 100
    full = total_steps(n, m, w)
    for L in (100, 500, 1000, 2000) if "b" not in skip else ():
        c = synth.related_batch(P, L, L, 0x2D20 + L)
        u = synth.uniform_batch(P, n - L, m - L, seed=0x2D21 + L)
        batch = synth.from_pairs([(c.query(p) + u.query(p), c.target(p) + u.target(p)) for p in range(P)])
        assert (batch.qlen == n).all() and (batch.tlen == m).all()
        inputs = None
        for name, sc, gap_open in (("linear", (2, -4, -4), 0), ("affine", (2, -4, -2), -4)):
            plans, inputs = three_plans(batch, sc, w, gap_open, z, inputs)
            line = {"shape": f"{P} pairs {n} x {m}, related prefix {L}, then unrelated", "prefix": L, "gaps": name,
                    "scoring": list(sc) + [gap_open], "band": w, "zdrop": z}
            line.update(time_plans(plans))
            off_res = plans["off"].results()
            oq, ot = plans["off"].ends()
            line["steps_off"] = P * full
            steps = {}
            for rule in RULES:
                steps[rule] = plans[rule].swept_steps().astype(np.uint64)
                res = plans[rule].results()
                rq, rt = plans[rule].ends()
                line[rule + "_steps"] = int(steps[rule].sum())
                line[rule + "_steps_over_off"] = round(int(steps[rule].sum()) / (P * full), 4)
                line[rule + "_pairs_dropped_share"] = round(float((steps[rule] < full).mean()), 4)
                line[rule + "_same_scores_share"] = round(float((res.scores == off_res.scores).mean()), 4)
                line[rule + "_same_ends_share"] = round(float(((rq == oq) & (rt == ot)).mean()), 4)
            line["stripe_minus_segment_steps_per_pair"] = round(
                (int(steps["stripe"].sum()) - int(steps["segment"].sum())) / P, 1)
            # the first pairs through the two references: the step counts must be the kernels', exactly
            k = a.ref_pairs if name == "linear" else max(a.ref_pairs // 4, 1)
            pred = {r: 0 for r in RULES}
            for p in range(k):
                f = ZR.fill(batch.query(p), batch.target(p), *sc, w, gap_open if gap_open else None)
                pred["segment"] += ZR.result(f, z, want_cigar=False).swept_steps
                pred["stripe"] += SR.result(f, z, want_cigar=False).swept_steps
            line["reference_pairs"] = k
            for rule in RULES:
                line[rule + "_reference_steps"] = pred[rule]
                line[rule + "_reference_steps_match"] = bool(pred[rule] == int(steps[rule][:k].sum()))
            dying.append(line)
            print(json.dumps(line), flush=True)
            for p in plans.values():
                p.close()
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
            kinds = (None,) + RULES
            outs = {k: os.path.join(tmp, f"{k}.paf") for k in kinds}

            def run(kind):
                t0 = time.perf_counter()
                if kind is None:
                    M.map_files(ref, reads, out=outs[kind], band=64, extend_ends=True, **sc)
                else:
                    M.map_files(ref, reads, out=outs[kind], band=64, extend_ends=True, zdrop=100, zdrop_rule=kind, **sc)
                return time.perf_counter() - t0

            for k in kinds:
                run(k)
            t = {k: [] for k in kinds}
            for _ in range(3):
                for k in kinds:
                    t[k].append(run(k))
            lines = {k: open(outs[k], "rb").read().splitlines() for k in kinds}
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
            full_e = np.array([total_steps(len(q), len(s), 64) for q, s in ends], np.uint64)
            plain_e = al.align_batch_anchored(eb, 2, -4, -4, 64, want_cigar=False)
            mapper = {"reads": rs.n_reads, "read_bases": int(rs.len.sum()), "mapped": len(lines[None]),
                      "command": "-a global -c -m 2 -n -4 -g -4 --band 64 --extend-ends [--zdrop 100 --zdrop-rule R]",
                      "extend_ends_wall_s": round(statistics.median(t[None]), 3),
                      "extend_ends_walls_s": [round(x, 3) for x in t[None]], "nonempty_ends": len(ends),
                      "ends_longer_than_1024": int(sum(len(q) > 1024 for q, _ in ends))}
            for k in RULES:
                assert len(lines[k]) == len(lines[None])
                res = al.align_batch_anchored(eb, 2, -4, -4, 64, want_cigar=False, zdrop=100, zdrop_rule=k)
                mapper[k] = {
                    "wall_s": round(statistics.median(t[k]), 3), "walls_s": [round(x, 3) for x in t[k]],
                    "lines_changed_share": round(sum(x != y for x, y in zip(lines[None], lines[k])) /
                                                 max(len(lines[None]), 1), 4),
                    "ends_stopped_early_share": round(float((res.swept_steps < full_e).mean()), 4),
                    "ends_steps_over_off": round(int(res.swept_steps.astype(np.uint64).sum()) /
                                                 max(int(full_e.sum()), 1), 4),
                    "ends_with_another_goal_share": round(float(((res.query_ends != plain_e.query_ends) |
                                                                 (res.target_ends != plain_e.target_ends)).mean()), 4),
                    # an end cut at row 1,024 exactly that plain anchored alignment carries further: the pass-tail clip
                    "ends_clipped_at_row_1024": int(((res.query_ends == 1024) & (plain_e.query_ends > 1024)).sum())}
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
