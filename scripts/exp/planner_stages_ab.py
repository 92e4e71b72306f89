#!/usr/bin/env python3
"""Planning time of two planners side by side, on the CPU (scripts/exp/planner_time.cpp).

    python scripts/exp/planner_stages_ab.py --parent-src DIR [--runs 9] [--out FILE.json]

DIR holds the other commit's ta_planner.cpp, ta_planner.h and ta_layout.h
(git show COMMIT:bioinfo1_amd/csrc/NAME > DIR/NAME).  Both builds run alternately,
RUNS times each; per shape and plan family the change passes when its median does
not exceed the parent's median by more than the parent's own max - min.  Prints the
result as JSON (and merges it into FILE.json under "planning_time")."""
import argparse
import json
import os
import statistics
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CS = os.path.join(ROOT, "bioinfo1_amd", "csrc")


def build(src_dir, exe):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", src_dir, os.path.join(ROOT, "scripts", "exp", "planner_time.cpp"),
                           os.path.join(src_dir, "ta_planner.cpp"), "-o", exe])


def run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {ln.split()[0]: (float(ln.split()[1]), float(ln.split()[2])) for ln in out.splitlines()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-src", required=True)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"parent": os.path.join(tmp, "parent"), "change": os.path.join(tmp, "change")}
        build(a.parent_src, exes["parent"])
        build(CS, exes["change"])
        runs = {"parent": [], "change": []}
        for k in range(a.runs):
            for who in (("parent", "change") if k % 2 == 0 else ("change", "parent")):
                runs[who].append(run(exes[who]))
    result = {"what": "ns per call of build_plan (linear) and build_affine_plan (affine), %d alternating runs per build; "
                      "gate: change median <= parent median + (parent max - parent min)" % a.runs,
              "shapes": {}}
    ok = True
    for shape in runs["parent"][0]:
        for f, family in enumerate(("linear", "affine")):
            row = {}
            for who in ("parent", "change"):
                v = [r[shape][f] for r in runs[who]]
                row[who] = {"runs": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
            p, c = row["parent"], row["change"]
            row["change_vs_parent_pct"] = round(100 * (c["median"] / p["median"] - 1), 2)
            row["pass"] = c["median"] <= p["median"] + (p["max"] - p["min"])
            ok = ok and row["pass"]
            result["shapes"]["%s_%s" % (shape, family)] = row
    result["all_pass"] = ok
    print(json.dumps(result, indent=1))
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                doc = json.load(fh)
        doc["planning_time"] = result
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
