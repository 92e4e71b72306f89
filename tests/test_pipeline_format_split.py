"""The dependency structure of ta_pipeline_step when the slots' tracebacks are
split into a walk and a run formatter (ta_plan_execute_walk / _format,
bioinfo1_amd/csrc/ta_pipeline.cpp) on the CPU: the file is built with g++
against stub_ta.cpp's contexts and the recording stand-ins of
tests/cpp/pipeline_format_split.cpp for the HIP runtime's streams and events
and the plans' fill / walk / format / traceback calls.  The program asserts,
for depth 2 and 3 over 8 steps (with and without a ready event): walk k on the
one walk stream after its fill and walk k - 1, and after the formats of steps
0 .. k - depth only (not format k - 1); format k on the caller's stream after
walk k; the caller's work after format k; fill k after format k - depth and
after nothing of the steps in between; depth + 1 streams, one of high priority,
all destroyed; and, for two chunks, format_stream = 1, affine slots and plans
without a formatter kernel, the combined order pipeline_order.cpp asserts."""
import os
import subprocess

from conftest import ROOT

OUT = os.path.join(ROOT, "build", "san")


def test_pipeline_format_split():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "pipeline_format_split")
    oracle_o = os.path.join(OUT, "pipeline_format_split_align_oracle.o")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    # (stub_ta.cpp's host-batch stand-ins call oracle_align: the program does not link without it)
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-c", os.path.join(ROOT, "oracle", "align_oracle.c"),
                           "-o", oracle_o])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-pthread",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pipeline_format_split.cpp"),
                           os.path.join(ROOT, "bioinfo1_amd", "csrc", "ta_pipeline.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "stub_ta.cpp"), oracle_o, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fails 0" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
