#!/usr/bin/env python3
"""Device time of the annotate pass beside the plan's own execution, on the
config-2 batch (10,000 pairs of 1 kb x 1 kb, local, 1/-1/-1).

Runs the plan once (the annotate pass needs its outputs), then times, in this
process, with HIP events on one stream, after a warm-up, REPS repetitions each
of: run() alone, annotate() with eqx off, annotate() with eqx on.  Each figure
is the median over the repetitions of one event pair around one enqueue.
Writes profiles/bench/annotate_time.json and prints it.  Not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--related", action="store_true", help="the related variant (5%% sub/ins/del) instead of i.i.d.")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench", "annotate_time.json"))
    a = ap.parse_args()
    assert a.reps >= 20

    import torch

    from bioinfo1_amd import synth
    from bioinfo1_amd.align import Aligner, DevicePlan

    gen = synth.related_batch if a.related else synth.uniform_batch
    batch = gen(a.pairs, 1000, 1000, 0x5EED)
    plan = DevicePlan(Aligner(0), batch, 1, 1, -1, -1, True)
    plan.run()
    plan.check()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                "max_ms": round(max(ms), 4)}

    out = {"workload": f"{a.pairs} pairs 1000 x 1000, local, 1/-1/-1, {'related' if a.related else 'uniform'}",
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "run": timed(plan.run),
           "annotate_info_only": timed(lambda: plan.annotate(eqx=False)),
           "annotate_eqx": timed(lambda: plan.annotate(eqx=True))}
    plan.check()
    ann = plan.annotation()
    lens = plan.cigar_len.cpu().numpy()
    out["cigar_bytes_per_pair"] = round(float(lens.mean()), 1)
    out["eqx_bytes_per_pair"] = round(float(ann.eqx_lens.mean()), 1)
    cols = sum(int(ann.info[f].astype("int64").sum()) for f in ("n_eq", "n_x", "n_ins", "n_del", "n_free"))
    out["columns_per_pair"] = round(cols / a.pairs, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    plan.close()


if __name__ == "__main__":
    main()
