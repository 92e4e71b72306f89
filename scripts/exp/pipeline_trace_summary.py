"""The pipelined steps of a rocprofv3 kernel trace (bench.py's default run, no --serial), per steady-state step:
start and end of the checkpoint fill, of the hand-back int32 fill launch, of the walk and of the formatter, the
idle gap between one fill's end and the next fill's start, how far a fill reaches into the fill before it, and
the step period; the walk chain (walk start to next walk start), where each formatter ran (its queue, and how
much of it overlapped the next step's walk) and each walk's distance from its own step's hand-back launch.
Usage: pipeline_trace_summary.py <run_kernel_trace.csv> <out.json> [steps, default 20]"""
import csv
import json
import os
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
k = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Queue_Id"],
            int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)) for r in rows)


def of(sub, not_sub=None):
    return [x for x in k if sub in x[2] and not (not_sub and not_sub in x[2])]


fills = of("dual_fill_ck_kernel")
walks = of("traceback_ck_kernel")
fmts = of("format_runs_kernel")
# the hand-back launch right after a checkpoint fill on its queue: fill_back_kernel (before it: the int32 fill_kernel)
backs = of("fill_back_kernel") or [x for x in of("fill_kernel", "dual_fill") if "fill_pipe" not in x[2]]
fills = fills[-steps - 1:]  # the last steps of the timed loop: steady state
t0 = fills[0][0]


def us(a):
    return round(a / 1e3, 1)


def stat(v):
    v = [x / 1e3 for x in v]
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} if v else None


def inside(xs):
    return [x for x in xs if t0 <= x[0] <= fills[-1][1]]


# A walk's formatter.  Every step launches one walk and one formatter, so the two lists pair by ordinal over
# the whole trace (walks in start order, formatters in start order: one walk stream runs the walks in step
# order, and the formatters follow their walks in step order on the walk's queue or on the caller's).  Only
# where the counts differ or a formatter so paired starts before its walk has ended (several walk streams,
# whose walks may end out of step order) it is the first formatter on the walk's own queue from its end on.
_ordinal = len(walks) == len(fmts) and all(f[0] >= w[1] - 1000 for w, f in zip(walks, fmts))
_fmt_of = {w: f for w, f in zip(walks, fmts)} if _ordinal else {}


def format_of(walk):
    if _ordinal:
        return _fmt_of[walk]
    return next((x for x in fmts if x[0] >= walk[1] - 1000 and x[3] == walk[3]), None)


def overlap(x, y):
    return max(0, min(x[1], y[1]) - max(x[0], y[0]))


per_step = []
for a, b in zip(fills, fills[1:]):
    back = next((x for x in backs if x[0] >= a[1] - 1000 and x[3] == a[3] and x[0] < a[1] + 2_000_000), None)
    walk = next((x for x in walks if x[0] >= a[1] - 1000), None)
    fmt = format_of(walk) if walk else None
    per_step.append({"fill": [us(a[0] - t0), us(a[1] - t0)], "fill_queue": a[3],
                     "hand_back": [us(back[0] - t0), us(back[1] - t0)] if back else None,
                     "walk": [us(walk[0] - t0), us(walk[1] - t0)] if walk else None,
                     "format": [us(fmt[0] - t0), us(fmt[1] - t0)] if fmt else None,
                     "format_queue": fmt[3] if fmt else None, "walk_queue": walk[3] if walk else None,
                     "walk_start_minus_hand_back_end_us": us(walk[0] - back[1]) if walk and back else None,
                     "next_fill_start_minus_fill_end_us": us(b[0] - a[1])})
gaps = [b[0] - a[1] for a, b in zip(fills, fills[1:])]
# the walks of consecutive steps (in start order) and each one's formatter (the next one on its queue):
# how far walk k+1 reaches into walk k and into walk k's formatter, and the walk chain per step
# (from one walk's start to the next one's), which is the period when the walks are what binds
wk = inside(walks)
wf = [format_of(w) for w in wk]
pairs = [(a, fa, b) for a, fa, b in zip(wk, wf, wk[1:]) if fa]
walk_chain = {
    "walk_start_to_next_walk_start": stat([b[0] - a[0] for a, _, b in pairs]),
    "next_walk_start_minus_walk_end": stat([b[0] - a[1] for a, _, b in pairs]),  # < 0: the walks overlap
    "next_walk_start_minus_format_end": stat([b[0] - fa[1] for a, fa, b in pairs]),  # < 0: beside the formatter
    "walks_overlapping_the_previous_walk": sum(b[0] < a[1] for a, _, b in pairs),
    "walks_starting_before_the_previous_format_ends": sum(b[0] < fa[1] for a, fa, b in pairs),
    "walk_plus_format": stat([fa[1] - a[0] for a, fa, _ in pairs]),
    "format_start_minus_walk_end": stat([fa[0] - a[1] for a, fa, _ in pairs]),
    # where the formatters ran: on their walk's queue (behind it, in the chain) or on another (the caller's),
    # and how much of formatter k ran while walk k+1 was running
    "formats_on_their_walk_queue": sum(fa[3] == a[3] for a, fa, _ in pairs),
    "format_queues": sorted({fa[3] for _, fa, _ in pairs}),
    "format_overlap_with_next_walk": stat([overlap(fa, b) for _, fa, b in pairs]),
    "format_fraction_beside_next_walk_median": round(statistics.median(
        [overlap(fa, b) / max(fa[1] - fa[0], 1) for _, fa, b in pairs]), 3) if pairs else None,
    "formats_wholly_beside_next_walk": sum(overlap(fa, b) == fa[1] - fa[0] for _, fa, b in pairs),
    "of": len(pairs)}
# step by step over the whole trace (one fill, one hand-back launch and one walk per step, each kind in step
# order): does a walk wait for its own step's hand-back launch?  (~0: it started when that launch ended)
all_f, all_b, all_w = of("dual_fill_ck_kernel"), backs, sorted(walks, key=lambda x: x[1])
if len(all_f) == len(all_b) == len(all_w):
    own = list(zip(all_f, all_b, all_w))[-steps:]
    walk_chain["walk_start_minus_own_hand_back_end"] = stat([w[0] - b[1] for _, b, w in own])
    walk_chain["walk_start_minus_own_fill_end"] = stat([w[0] - f[1] for f, _, w in own])
    walk_chain["walks_within_20us_of_own_hand_back_end"] = sum(0 <= w[0] - b[1] < 20_000 for _, b, w in own)
out = {"trace": os.path.basename(os.path.dirname(os.path.abspath(sys.argv[1]))), "steps": len(per_step),
       "fill_queues": sorted({x[3] for x in fills}), "walk_queues": sorted({x[3] for x in inside(walks)}),
       "fill_blocks": fills[0][4], "hand_back_blocks": sorted({x[4] for x in inside(backs)}),
       "walk_blocks": sorted({x[4] for x in inside(walks)}),
       "period": stat([b[0] - a[0] for a, b in zip(fills, fills[1:])]),
       "fill": stat([e - s for s, e, *_ in fills]),
       "hand_back": stat([e - s for s, e, *_ in inside(backs)]),
       "walk": stat([e - s for s, e, *_ in inside(walks)]),
       "format": stat([e - s for s, e, *_ in inside(fmts)]),
       # > 0: the GPU had no fill for that long; < 0: the next fill started that long before this one ended
       "gap_fill_end_to_next_fill_start": stat(gaps),
       "fills_overlapping_the_previous_fill": sum(g < 0 for g in gaps),
       "walk_start_minus_its_fill_end": stat([(p["walk"][0] - p["fill"][1]) * 1e3 for p in per_step if p["walk"]]),
       "formats_paired_by_ordinal": _ordinal,
       "walk_chain": walk_chain,
       "per_step": per_step}
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(json.dumps({a: b for a, b in out.items() if a != "per_step"}, indent=1))
