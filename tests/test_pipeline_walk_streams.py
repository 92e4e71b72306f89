"""The dependency structure of ta_pipeline_step with several walk streams
(ta_pipeline_create_ex, bioinfo1_amd/csrc/ta_pipeline.cpp) on the CPU: the file
is built with g++ against stub_ta.cpp's contexts and the recording stand-ins of
tests/cpp/pipeline_walk_streams.cpp for the HIP runtime's streams and events
and the plans' fill / traceback calls.  The program asserts, for depth 2, 3, 4
x walk_streams 1, 2, depth (one and two chunks, with and without a ready
event): depth + w streams, exactly w of high priority; walk k on walk stream
k % w after its own fill and, for w >= 2, not after walk k - 1; fill k after
exactly the steps up to k - depth (and its upload); the caller's stream after
walk k; a chunk's fill after the walk of the chunk before it; everything
destroyed; walk_streams > depth a TA_ERR_ARG that enqueues nothing; and
walk_streams = 0 resolved against GPU_MAX_HW_QUEUES (set inside the program)."""
import os
import subprocess

import pytest
from conftest import ROOT

OUT = os.path.join(ROOT, "build", "san")


@pytest.mark.parametrize("default", ["shipped", "2", "3"])
def test_pipeline_walk_streams(default):
    """shipped: the header's TA_PIPELINE_WALK_STREAMS_DEFAULT; 2, 3: the library and the program
    built with that default instead, so the queue rule is exercised whatever the header ships."""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, f"pipeline_walk_streams_{default}")
    oracle_o = os.path.join(OUT, f"pipeline_walk_streams_{default}_align_oracle.o")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    define = [] if default == "shipped" else [f"-DTA_PIPELINE_WALK_STREAMS_DEFAULT={default}u"]
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-c", os.path.join(ROOT, "oracle", "align_oracle.c"),
                           "-o", oracle_o])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-pthread"] + define +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pipeline_walk_streams.cpp"),
                           os.path.join(ROOT, "bioinfo1_amd", "csrc", "ta_pipeline.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "stub_ta.cpp"), oracle_o, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fails 0" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
