"""Alternating bench.py runs of a parent checkout and this tree with a forced number of walk
streams (align.DevicePipeline(walk_streams=...), ta_pipeline_create_ex): the table of
profiles/bench/walk_streams_ab.json.

  walk_streams_ab.py --parent DIR --out FILE.json --key NAME --rounds N --variants parent,w1,w2,w3,default
                     [--hwq Q] [-- bench.py arguments]

Per round every variant runs once, in the order given, each a fresh process under a time limit;
the first run that fails ends the script (nothing more is started on the GPU).  `parent` runs DIR's
own bench.py on DIR's own library; `wN` runs this tree's bench.py with DevicePipeline's default
walk_streams replaced by N; `default` runs it untouched (the library's choice).  --hwq sets
TA_BENCH_HW_QUEUES (bench.py's hardware-queue count) for every run.  The JSON (one entry per --key,
merged into FILE.json after every run) keeps each variant's ms_per_step per run, median, min, max."""
import json
import os
import runpy
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(w, bench_args):
    sys.path.insert(0, ROOT)
    import bioinfo1_amd.align as A

    init = A.DevicePipeline.__init__

    def forced(self, *a, **kw):
        kw.setdefault("walk_streams", w)
        init(self, *a, **kw)
        print(f"walk_streams_ab: walk_streams {self.walk_streams}", file=sys.stderr, flush=True)

    A.DevicePipeline.__init__ = forced
    sys.argv = [os.path.join(ROOT, "bench.py")] + bench_args
    runpy.run_path(sys.argv[0], run_name="__main__")


def main():
    argv = sys.argv[1:]
    bench_args = []
    if "--" in argv:
        bench_args = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    if argv and argv[0] == "--child":
        return child(int(argv[1]), bench_args)
    opt = dict(zip(argv[::2], argv[1::2]))
    parent, out, key = opt.get("--parent"), opt["--out"], opt["--key"]
    rounds, variants = int(opt.get("--rounds", 3)), opt.get("--variants", "parent,default").split(",")
    env = dict(os.environ)
    if "--hwq" in opt:
        env["TA_BENCH_HW_QUEUES"] = opt["--hwq"]
    runs = {v: [] for v in variants}
    seen = {}
    for r in range(rounds):
        for v in variants:
            if v == "parent":
                cmd, cwd = [sys.executable, "-u", "bench.py"] + bench_args, parent
            elif v == "default":
                cmd, cwd = [sys.executable, "-u", "bench.py"] + bench_args, ROOT
            else:
                cmd, cwd = [sys.executable, "-u", os.path.abspath(__file__), "--child", v[1:], "--"] + bench_args, ROOT
            p = subprocess.run(["timeout", "-k", "10", "240"] + cmd, cwd=cwd, env=env, capture_output=True, text=True)
            line = next((ln for ln in reversed(p.stdout.splitlines()) if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                print(f"{key} {v} round {r}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
                return 1
            d = json.loads(line)
            runs[v].append(d["ms_per_step"])
            seen[v] = next((ln.split()[-1] for ln in p.stderr.splitlines() if ln.startswith("walk_streams_ab:")), None)
            print(f"{key} {v} round {r}: {d['ms_per_step']} ms", flush=True)
            table = json.load(open(out)) if os.path.exists(out) else {}
            table[key] = {"args": " ".join(bench_args), "hw_queues": opt.get("--hwq", "bench.py's 16"),
                          **{u: {"runs": x, "median": round(statistics.median(x), 4), "min": min(x), "max": max(x),
                                 **({"walk_streams": int(seen[u])} if seen.get(u) else {})}
                             for u, x in runs.items() if x}}
            json.dump(table, open(out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
