#!/usr/bin/env python3
"""Device time of the banded affine plan beside the full affine plan on the
same pairs.

Shapes: semi-global, 1/-1 with gap open -2 / extend -1, CIGAR on,
synth.related_batch with seed 0x5EED; 4,096 pairs of 10 kb x 10 kb with w in
{128, 256, 512} and 512 pairs of 32,768 x 32,768 with w = 512.  Both plans
live in this process on one context; after a warm-up the two are timed
alternately, REPS repetitions each, one HIP event pair around one execution on
one stream; each figure is the median.  Per line: ms of each plan and their
ratio, in-band and swept cells, in-band GCUPS, workspace bytes and chunks of
both plans and whether every banded result (score, target_begin, CIGAR) is
byte-identical to the full plan's.  The 32 k line carries the gate: the banded
affine plan at least 2 x faster than the full affine plan.  Writes
profiles/bench/banded_affine_time.json and prints it.  Not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCORING = (1, -1, -2, -1)  # match, mismatch, gap open, gap extend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs-10k", type=int, default=4096)
    ap.add_argument("--pairs-32k", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench", "banded_affine_time.json"))
    a = ap.parse_args()
    assert a.reps >= 20

    import numpy as np
    import torch

    from bioinfo1_amd import synth
    from bioinfo1_amd.align import Aligner, DevicePlan

    al = Aligner(0)
    ma, mi, go, ge = SCORING

    def once(plan):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def identical(x, y, P):
        same = (x.scores == y.scores) & (x.target_begins == y.target_begins) & (x.cigar_lens == y.cigar_lens)
        n = 0
        for p in np.flatnonzero(same):
            n += x.cigar(int(p)) == y.cigar(int(p))
        return n / P

    lines = []
    for length, pairs, bands in ((10000, a.pairs_10k, (128, 256, 512)), (32768, a.pairs_32k, (512,))):
        batch = synth.related_batch(pairs, length, length, 0x5EED)
        full = DevicePlan(al, batch, 2, ma, mi, ge, True, gap_open=go)
        inputs = (full.qbytes, full.qoff, full.tbytes, full.toff)
        full.run()
        want = full.results()
        for w in bands:
            plan = DevicePlan.banded_affine(al, batch, 2, ma, mi, go, ge, w, True, inputs=inputs)
            for _ in range(a.warmup):
                once(plan)
                once(full)
            tb, tf = [], []
            for _ in range(a.reps):  # alternately, in the same process
                tb.append(once(plan))
                tf.append(once(full))
            got = plan.results()
            full.check()
            mb, mf = statistics.median(tb), statistics.median(tf)
            share = identical(got, want, pairs)
            line = {"shape": f"{pairs} pairs {length} x {length}, semi-global, 1/-1, open -2 / extend -1, CIGAR, "
                             "related 0x5EED",
                    "band": w, "banded_affine_ms": round(mb, 3), "full_affine_ms": round(mf, 3),
                    "banded_affine_min_max_ms": [round(min(tb), 3), round(max(tb), 3)],
                    "full_affine_min_max_ms": [round(min(tf), 3), round(max(tf), 3)],
                    "speedup": round(mf / mb, 3), "band_cells": plan.band_cells, "swept_cells": plan.swept_cells,
                    "swept_over_band": round(plan.swept_cells / plan.band_cells, 3),
                    "full_cells": int(batch.cells), "band_gcups": round(plan.band_cells / mb / 1e6, 1),
                    "banded_affine_workspace_bytes": plan.workspace_bytes, "banded_affine_chunks": plan.chunks,
                    "full_affine_workspace_bytes": full.workspace_bytes, "full_affine_chunks": full.chunks,
                    "full_affine_dual_pairs": full.dual_pairs,
                    "identical_share": round(share, 4), "all_identical": bool(share == 1.0)}
            if length == 32768:
                line["gate_2x"] = bool(mf / mb >= 2.0)
            lines.append(line)
            print(json.dumps(line), flush=True)
            plan.close()
        full.close()
        del full, want
        al.release()
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "lines": lines}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
