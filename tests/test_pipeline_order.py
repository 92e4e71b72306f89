"""The dependency structure of ta_pipeline_step (bioinfo1_amd/csrc/ta_pipeline.cpp)
on the CPU: the file is built with g++ against stub_ta.cpp's contexts and the
recording stand-ins of tests/cpp/pipeline_order.cpp for the HIP runtime's
streams and events and the plans' fill / traceback calls.  The program asserts,
for depth 2 and 3 over 8 steps (one and two chunks, with and without a ready
event), what every launch follows: fill k the previous use of its slot (step
k - depth: fills, walks and what the caller queued after them) and nothing of
the steps in between, walk k its fill, the caller's stream walk k; and that
argument errors enqueue nothing."""
import os
import subprocess

from conftest import ROOT

OUT = os.path.join(ROOT, "build", "san")


def test_pipeline_order():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "pipeline_order")
    oracle_o = os.path.join(OUT, "pipeline_order_align_oracle.o")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-c", os.path.join(ROOT, "oracle", "align_oracle.c"),
                           "-o", oracle_o])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-pthread",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pipeline_order.cpp"),
                           os.path.join(ROOT, "bioinfo1_amd", "csrc", "ta_pipeline.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "stub_ta.cpp"), oracle_o, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fails 0" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
