"""Every field of the host planner's output (bioinfo1_amd/csrc/ta_planner.cpp),
digested per group of batches by tests/cpp/plan_dump.cpp, against
tests/golden/plans/digest.json: a change of the planner that moves a kernel
choice, an offset, a chunk cut or a ticket fails here, on the CPU."""
import json
import os
import subprocess

from conftest import ROOT

CS = os.path.join(ROOT, "bioinfo1_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plans", "digest.json")


def test_plan_digest(tmp_path):
    """The linear, affine and banded plans of 3,000 random batches and of the directed
    batches at the planner's edges equal, field by field, those of the planner that
    the golden file was made from.

    The file was made by the planner of commit 74c9ddd, before it was split into stages;
    a refactor leaves it alone.  A change that moves plans on purpose regenerates it,

        g++ -std=c++17 -O2 -I bioinfo1_amd/csrc tests/cpp/plan_dump.cpp bioinfo1_amd/csrc/ta_planner.cpp -o plan_dump
        ./plan_dump digest      # one "name batches fnv1a64" line per group -> digest.json

    and says which groups moved and why; `plan_dump text NAME` of the planner before
    and after, diffed, shows the fields."""
    exe = str(tmp_path / "plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", CS, os.path.join(ROOT, "tests", "cpp", "plan_dump.cpp"),
                           os.path.join(CS, "ta_planner.cpp"), "-o", exe])
    out = subprocess.run([exe, "digest"], capture_output=True, text=True, timeout=120, check=True).stdout
    got = {}
    for ln in out.splitlines():
        name, batches, digest = ln.split()
        got[name] = {"batches": int(batches), "fnv1a64": digest}
    with open(GOLDEN) as f:
        want = json.load(f)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
