#!/usr/bin/env python3
"""Device time of the anchored plan beside the banded global and banded local
plans of the same batch, and the mapper's wall time with and without
--extend-ends.

Alignment shapes: the banded table's -- 4,096 pairs of 10 kb x 10 kb at w = 128
and 512 and 2,048 pairs of 32,768 x 32,768 at w = 512 -- plus one affine line
(10 kb, w = 512, gap_open -3); synth.related_batch seed 0x5EED, 1/-1/-1, CIGAR
on.  The three plans of a line live in this process on one context; after
WARMUP executions each they are timed alternately, REPS executions each, one HIP
event pair around one execution on one stream; a figure is the median of the
REPS.  That is repeated three times: per plan the three medians, their median
and their spread (max - min).  The anchored cell update is local's minus the
clamp and the STOP ballots, so the expectation is a time between global's and
local's; "above_local_by_more_than_spread" says whether the anchored median
exceeds local's by more than the spread of local's three medians.

Mapper: reads of synth.cfg3_batch's kind (ONT-like, of a 4.64 Mb genome) written
as FASTA; wall time of mapper.map_files at -a global -c --band 64 with and
without extend_ends (once to warm up, then the median of three each,
alternately), and the share of mapped reads whose ends grew.

Writes profiles/bench/anchored_time.json and prints it.  Not part of bench.py.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs-10k", type=int, default=4096)
    ap.add_argument("--pairs-32k", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mapper-reads", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench", "anchored_time.json"))
    a = ap.parse_args()

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

    lines = []
    shapes = ((10000, a.pairs_10k, (128, 512), None), (32768, a.pairs_32k, (512,), None),
              (10000, a.pairs_10k, (512,), -3))
    batch, last = None, None
    for length, pairs, bands, gap_open in shapes:
        if (length, pairs) != last:
            batch = synth.related_batch(pairs, length, length, 0x5EED)
            last = (length, pairs)
        inputs = None
        for w in bands:
            if gap_open is None:
                glob = DevicePlan(al, batch, 0, 1, -1, -1, True, band=w, inputs=inputs)
                inputs = (glob.qbytes, glob.qoff, glob.tbytes, glob.toff)
                loc = DevicePlan(al, batch, 1, 1, -1, -1, True, band=w, inputs=inputs)
                anc = DevicePlan.anchored(al, batch, 1, -1, -1, w, inputs=inputs)
            else:
                glob = DevicePlan.banded_affine(al, batch, 0, 1, -1, gap_open, -1, w, inputs=inputs)
                inputs = (glob.qbytes, glob.qoff, glob.tbytes, glob.toff)
                loc = DevicePlan.banded_affine(al, batch, 1, 1, -1, gap_open, -1, w, inputs=inputs)
                anc = DevicePlan.anchored(al, batch, 1, -1, -1, w, gap_open=gap_open, inputs=inputs)
            plans = {"anchored": anc, "global": glob, "local": loc}
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
            qe, te = anc.ends()
            line = {"shape": f"{pairs} pairs {length} x {length}, 1/-1/-1, CIGAR, related 0x5EED",
                    "band": w, "gap_open": gap_open or 0, "band_cells": anc.band_cells, "swept_cells": anc.swept_cells,
                    "workspace_bytes": anc.workspace_bytes, "chunks": anc.chunks,
                    "goals_at_the_corner_share": round(float(((qe == batch.qlen) & (te == batch.tlen)).mean()), 4)}
            for k in plans:
                line[k + "_ms"] = round(statistics.median(meds[k]), 3)
                line[k + "_medians_ms"] = [round(x, 3) for x in meds[k]]
                line[k + "_spread_ms"] = round(max(meds[k]) - min(meds[k]), 3)
            line["band_gcups"] = round(anc.band_cells / line["anchored_ms"] / 1e6, 1)
            line["between_global_and_local"] = bool(line["global_ms"] <= line["anchored_ms"] <= line["local_ms"])
            line["above_local_by_more_than_spread"] = bool(line["anchored_ms"] - line["local_ms"] > line["local_spread_ms"])
            lines.append(line)
            print(json.dumps(line), flush=True)
            for p in plans.values():
                p.close()
        al.release()
        torch.cuda.empty_cache()
    al.close()

    # ---- the mapper, on files
    g = synth.genome(synth.ECOLI_LEN)
    rs = synth.ont_reads(a.mapper_reads, g)
    mapper = {}
    with tempfile.TemporaryDirectory() as tmp:
        ref, reads = os.path.join(tmp, "ref.fasta"), os.path.join(tmp, "reads.fasta")
        with open(ref, "wb") as f:
            f.write(b">genome\n" + g.tobytes() + b"\n")
        with open(reads, "wb") as f:
            for r in range(rs.n_reads):
                f.write(b">r%d\n" % r + rs.read(r) + b"\n")
        outs = {False: os.path.join(tmp, "plain.paf"), True: os.path.join(tmp, "ends.paf")}

        def run(ext):
            t0 = time.perf_counter()
            M.map_files(ref, reads, out=outs[ext], band=64, extend_ends=ext, type=0, want_cigar=True)
            return time.perf_counter() - t0

        run(False)
        run(True)
        t = {False: [], True: []}
        for _ in range(3):
            for ext in (False, True):
                t[ext].append(run(ext))
        plain = open(outs[False], "rb").read().splitlines()
        ends = open(outs[True], "rb").read().splitlines()
        assert len(plain) == len(ends)
        grew = full = 0
        for x, y in zip(plain, ends):
            cx, cy = x.split(b"\t"), y.split(b"\t")
            grew += (int(cy[2]), int(cy[3])) != (int(cx[2]), int(cx[3]))
            full += int(cy[2]) == 0 and int(cy[3]) == int(cy[1])
        mapper = {"reads": rs.n_reads, "read_bases": int(rs.len.sum()), "mapped": len(plain),
                  "command": "-a global -c --band 64 [--extend-ends], 1/-1/-1",
                  "plain_wall_s": round(statistics.median(t[False]), 3), "plain_walls_s": [round(x, 3) for x in t[False]],
                  "extend_ends_wall_s": round(statistics.median(t[True]), 3),
                  "extend_ends_walls_s": [round(x, 3) for x in t[True]],
                  "ends_grew_share": round(grew / max(len(plain), 1), 4),
                  "whole_read_aligned_share": round(full / max(len(plain), 1), 4)}
        print(json.dumps(mapper), flush=True)

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "repeats": a.repeats,
           "lines": lines, "mapper": mapper}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
