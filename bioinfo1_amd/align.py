"""Python host-side mirror of the team_alignment interface.

``align()`` mirrors ``team::Align`` (/root/reference/team_alignment/
team_alignment.hpp:14-23): same arguments, same results -- the int score, the
CIGAR bytes the reference assigns to ``*cigar`` (``None`` when no CIGAR is
requested, like passing ``cigar = nullptr``) and ``*target_begin`` -- and the
same error: an unknown type raises ``ValueError("Unknown AlignmentType
provided.")`` (the reference's ``std::invalid_argument``).

``Aligner.align_batch()`` is the batched form (host memory in and out) and
``DevicePlan`` the device-resident form (torch CUDA tensors in HBM) used by
bench.py.  Everything goes through the extern "C" ABI of
``libteam_alignment.so`` (include/team_align_c.h) into the gfx950 HIP
kernels; there is no CPU fallback -- if the library or a gfx950 GPU is
missing, these raise.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libteam_alignment.so")

TA_OK, TA_ERR_BAD_TYPE, TA_ERR_CIGAR, TA_ERR_ARG, TA_ERR_DEVICE, TA_ERR_CAPACITY, TA_ERR_RANGE, TA_ERR_UNSERVED = range(8)
# ta_plan_create flags (include/team_align_c.h): kernel selection, same results
TA_PLAN_INT32_ONLY, TA_PLAN_NO_FLEX, TA_PLAN_UNFUSED, TA_PLAN_WALK1, TA_PLAN_WALK2 = 1, 2, 4, 8, 16
TA_PLAN_SERIAL_PASSES, TA_PLAN_PASS_MAJOR, TA_PLAN_NO_BLK, TA_PLAN_NO_CK, TA_PLAN_CK = 32, 64, 128, 256, 512
TA_PLAN_NO_FLEX_CK = 1024


class AlignmentType(enum.IntEnum):
    """team::AlignmentType (team_alignment.hpp:8-12), underlying int."""

    global_ = 0
    local = 1
    semiGlobal = 2


class DeviceError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load libteam_alignment.so (fails loudly if it was not built).

    torch, when importable, is imported first so that the process has a single
    HIP runtime (torch's libamdhip64 satisfies the library's dependency)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    u32p, u64p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    L.ta_status_string.restype = C.c_char_p
    L.ta_status_string.argtypes = [C.c_int]
    L.ta_last_error.restype = C.c_char_p
    L.ta_last_error.argtypes = [C.c_void_p]
    L.ta_context_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.ta_context_destroy.argtypes = [C.c_void_p]
    L.ta_context_destroy.restype = None
    L.ta_cigar_slot_bytes.restype = C.c_uint64
    L.ta_cigar_slot_bytes.argtypes = [C.c_uint32, C.c_uint32]
    L.ta_align_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, u64p, u32p, C.c_void_p, u64p, u32p, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, i32p, u32p, C.c_void_p, C.c_uint64, u64p, u32p]
    L.ta_align_batch_flags.argtypes = L.ta_align_batch.argtypes + [C.c_uint32]
    L.ta_context_release.argtypes = [C.c_void_p]
    L.ta_context_release.restype = None
    L.ta_context_held_bytes.argtypes = [C.c_void_p]
    L.ta_context_held_bytes.restype = C.c_uint64
    L.ta_set_default_device.argtypes = [C.c_int]
    L.ta_set_thread_device.argtypes = [C.c_int]
    L.ta_plan_create.argtypes = [C.c_void_p, C.c_uint32, u32p, u32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ta_plan_destroy.argtypes = [C.c_void_p]
    L.ta_plan_destroy.restype = None
    for f in ("ta_plan_cigar_slots_bytes", "ta_plan_workspace_bytes"):
        getattr(L, f).restype = C.c_uint64
        getattr(L, f).argtypes = [C.c_void_p]
    L.ta_plan_chunks.restype = C.c_uint32
    L.ta_plan_chunks.argtypes = [C.c_void_p]
    L.ta_plan_dual_pairs.restype = C.c_uint32
    L.ta_plan_dual_pairs.argtypes = [C.c_void_p]
    L.ta_plan_flex_pairs.restype = C.c_uint32
    L.ta_plan_flex_pairs.argtypes = [C.c_void_p]
    L.ta_plan_fused.argtypes = [C.c_void_p]
    L.ta_plan_walk.argtypes = [C.c_void_p]
    L.ta_plan_pair_chunks.argtypes = [C.c_void_p, u32p]
    L.ta_affine_plan_pair_chunks.argtypes = [C.c_void_p, u32p]
    L.ta_plan_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_plan_check.argtypes = [C.c_void_p]
    L.ta_compact_cigars.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    L.ta_plan_execute_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_plan_execute_traceback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_plan_execute_walk.argtypes = L.ta_plan_execute_traceback.argtypes
    L.ta_plan_execute_format.argtypes = L.ta_plan_execute_traceback.argtypes
    L.ta_plan_format_is_split.argtypes = [C.c_void_p, C.c_uint32]
    L.ta_pipeline_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ta_pipeline_create_affine.argtypes = L.ta_pipeline_create.argtypes
    L.ta_pipeline_create_ex.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.ta_pipeline_create_affine_ex.argtypes = L.ta_pipeline_create_ex.argtypes
    L.ta_pipeline_walk_streams.argtypes = [C.c_void_p]
    L.ta_pipeline_walk_streams.restype = C.c_uint32
    L.ta_pipeline_format_split.argtypes = [C.c_void_p]
    L.ta_pipeline_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u32p]
    L.ta_pipeline_destroy.argtypes = [C.c_void_p]
    L.ta_pipeline_destroy.restype = None
    # affine-gap extension (include/team_align_c.h, no reference counterpart)
    L.ta_align_batch_affine.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, u64p, u32p, C.c_void_p, u64p, u32p,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, u32p, C.c_void_p,
                                        C.c_uint64, u64p, u32p]
    L.ta_affine_plan_create.argtypes = [C.c_void_p, C.c_uint32, u32p, u32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ta_affine_plan_destroy.argtypes = [C.c_void_p]
    L.ta_affine_plan_destroy.restype = None
    for f in ("ta_affine_plan_cigar_slots_bytes", "ta_affine_plan_workspace_bytes"):
        getattr(L, f).restype = C.c_uint64
        getattr(L, f).argtypes = [C.c_void_p]
    L.ta_affine_plan_chunks.restype = C.c_uint32
    L.ta_affine_plan_chunks.argtypes = [C.c_void_p]
    L.ta_affine_plan_dual_pairs.restype = C.c_uint32
    L.ta_affine_plan_dual_pairs.argtypes = [C.c_void_p]
    L.ta_affine_plan_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_affine_plan_execute_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_affine_plan_execute_traceback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_affine_plan_check.argtypes = [C.c_void_p]
    # banded extension (include/team_align_c.h, no reference counterpart)
    L.ta_align_batch_banded.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, u64p, u32p, C.c_void_p, u64p, u32p, u32p,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, u32p, C.c_void_p,
                                        C.c_uint64, u64p, u32p]
    L.ta_banded_plan_create.argtypes = [C.c_void_p, C.c_uint32, u32p, u32p, u32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ta_banded_plan_destroy.argtypes = [C.c_void_p]
    L.ta_banded_plan_destroy.restype = None
    for f in ("ta_banded_plan_cigar_slots_bytes", "ta_banded_plan_workspace_bytes", "ta_banded_plan_band_cells",
              "ta_banded_plan_swept_cells"):
        getattr(L, f).restype = C.c_uint64
        getattr(L, f).argtypes = [C.c_void_p]
    L.ta_banded_plan_chunks.restype = C.c_uint32
    L.ta_banded_plan_chunks.argtypes = [C.c_void_p]
    L.ta_banded_plan_pair_chunks.argtypes = [C.c_void_p, u32p]
    L.ta_banded_plan_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_banded_plan_execute_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_banded_plan_execute_traceback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_banded_plan_check.argtypes = [C.c_void_p]
    L.ta_banded_plan_annotate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # banded affine extension (include/team_align_c.h, no reference counterpart)
    L.ta_align_batch_banded_affine.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, u64p, u32p, C.c_void_p, u64p, u32p,
                                               u32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, u32p,
                                               C.c_void_p, C.c_uint64, u64p, u32p]
    L.ta_banded_affine_plan_create.argtypes = [C.c_void_p, C.c_uint32, u32p, u32p, u32p, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32,
                                               C.POINTER(C.c_void_p)]
    L.ta_banded_affine_plan_destroy.argtypes = [C.c_void_p]
    L.ta_banded_affine_plan_destroy.restype = None
    for f in ("ta_banded_affine_plan_cigar_slots_bytes", "ta_banded_affine_plan_workspace_bytes",
              "ta_banded_affine_plan_band_cells", "ta_banded_affine_plan_swept_cells"):
        getattr(L, f).restype = C.c_uint64
        getattr(L, f).argtypes = [C.c_void_p]
    L.ta_banded_affine_plan_chunks.restype = C.c_uint32
    L.ta_banded_affine_plan_chunks.argtypes = [C.c_void_p]
    L.ta_banded_affine_plan_pair_chunks.argtypes = [C.c_void_p, u32p]
    L.ta_banded_affine_plan_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_banded_affine_plan_execute_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_banded_affine_plan_execute_traceback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_banded_affine_plan_check.argtypes = [C.c_void_p]
    L.ta_banded_affine_plan_annotate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # exact banded alignment: the certificate and the two-round host batches
    u8p = C.POINTER(C.c_uint8)
    L.ta_banded_plan_certify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_banded_affine_plan_certify.argtypes = L.ta_banded_plan_certify.argtypes
    L.ta_align_batch_banded_exact.argtypes = L.ta_align_batch_banded.argtypes + [u32p, u8p]
    L.ta_align_batch_banded_affine_exact.argtypes = L.ta_align_batch_banded_affine.argtypes + [u32p, u8p]
    # anchored (free-end) alignment (include/team_align_c.h, no reference counterpart)
    L.ta_align_batch_anchored.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, u64p, u32p, C.c_void_p, u64p, u32p, u32p,
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p, u32p, u32p, C.c_void_p,
                                          C.c_uint64, u64p, u32p]
    L.ta_anchored_plan_create.argtypes = [C.c_void_p, C.c_uint32, u32p, u32p, u32p, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ta_anchored_plan_destroy.argtypes = [C.c_void_p]
    L.ta_anchored_plan_destroy.restype = None
    for f in ("ta_anchored_plan_cigar_slots_bytes", "ta_anchored_plan_workspace_bytes",
              "ta_anchored_plan_band_cells", "ta_anchored_plan_swept_cells"):
        getattr(L, f).restype = C.c_uint64
        getattr(L, f).argtypes = [C.c_void_p]
    L.ta_anchored_plan_chunks.restype = C.c_uint32
    L.ta_anchored_plan_chunks.argtypes = [C.c_void_p]
    L.ta_anchored_plan_pair_chunks.argtypes = [C.c_void_p, u32p]
    L.ta_anchored_plan_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_anchored_plan_execute_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_anchored_plan_execute_traceback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.ta_anchored_plan_check.argtypes = [C.c_void_p]
    L.ta_anchored_plan_annotate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_anchored_plan_ends.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # z-drop on anchored alignment
    L.ta_anchored_plan_create_zdrop.argtypes = (L.ta_anchored_plan_create.argtypes[:-1]
                                                + [C.c_int32, C.POINTER(C.c_void_p)])
    L.ta_anchored_plan_swept_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_align_batch_anchored_zdrop.argtypes = L.ta_align_batch_anchored.argtypes + [C.c_int32, u32p]
    # ... with the rule chosen (TA_ZDROP_SEGMENT / TA_ZDROP_STRIPE)
    L.ta_anchored_plan_create_zdrop_rule.argtypes = (L.ta_anchored_plan_create.argtypes[:-1]
                                                     + [C.c_int32, C.c_int, C.POINTER(C.c_void_p)])
    L.ta_align_batch_anchored_zdrop_rule.argtypes = L.ta_align_batch_anchored.argtypes + [C.c_int32, C.c_int, u32p]
    # the annotate post-pass (info records, =/X CIGARs)
    L.ta_plan_annotate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ta_affine_plan_annotate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # the low-latency single-pair server (ta_server_*)
    L.ta_server_create.argtypes = [C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ta_server_destroy.argtypes = [C.c_void_p]
    L.ta_server_destroy.restype = None
    L.ta_server_fits.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int]
    L.ta_server_running.argtypes = [C.c_void_p]
    L.ta_server_last_times.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]
    L.ta_server_align.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_void_p,
                                  C.c_uint64, C.POINTER(C.c_uint32)]
    _lib = L
    return L


# Every symbol include/team_align_c.h declares (checked by tests/test_abi.py).
ABI_SYMBOLS = [
    "ta_status_string", "ta_last_error", "ta_context_create", "ta_context_destroy", "ta_context_release",
    "ta_context_held_bytes", "ta_set_default_device", "ta_set_thread_device", "ta_current_device", "ta_device_count",
    "ta_cigar_slot_bytes", "ta_align_batch", "ta_align_batch_flags", "ta_plan_create", "ta_plan_destroy", "ta_plan_cigar_slots_bytes",
    "ta_plan_workspace_bytes", "ta_plan_chunks", "ta_plan_dual_pairs", "ta_plan_flex_pairs", "ta_plan_fused", "ta_plan_walk",
    "ta_plan_execute", "ta_plan_check", "ta_plan_execute_fill", "ta_plan_pair_chunks", "ta_affine_plan_pair_chunks", "ta_plan_execute_traceback", "ta_compact_cigars",
    "ta_affine_plan_create", "ta_affine_plan_destroy", "ta_affine_plan_cigar_slots_bytes",
    "ta_affine_plan_workspace_bytes", "ta_affine_plan_chunks", "ta_affine_plan_dual_pairs", "ta_affine_plan_execute", "ta_affine_plan_execute_fill",
    "ta_affine_plan_execute_traceback", "ta_affine_plan_check", "ta_align_batch_affine",
    "ta_server_create", "ta_server_destroy", "ta_server_fits", "ta_server_align", "ta_server_running",
    "ta_server_last_times", "ta_server_pause", "ta_server_resume",
    "ta_plan_annotate", "ta_affine_plan_annotate",
    "ta_plan_context", "ta_affine_plan_context", "ta_context_device",
    "ta_pipeline_create", "ta_pipeline_create_affine", "ta_pipeline_step", "ta_pipeline_destroy",
    "ta_pipeline_create_ex", "ta_pipeline_create_affine_ex", "ta_pipeline_walk_streams",
    "ta_plan_execute_walk", "ta_plan_execute_format", "ta_plan_format_is_split", "ta_pipeline_format_split",
]
# The banded extension's symbols (checked by tests/test_banded_ref.py).
BANDED_ABI_SYMBOLS = [
    "ta_banded_plan_create", "ta_banded_plan_destroy", "ta_banded_plan_cigar_slots_bytes",
    "ta_banded_plan_workspace_bytes", "ta_banded_plan_chunks", "ta_banded_plan_pair_chunks",
    "ta_banded_plan_band_cells", "ta_banded_plan_swept_cells", "ta_banded_plan_execute",
    "ta_banded_plan_execute_fill", "ta_banded_plan_execute_traceback", "ta_banded_plan_check",
    "ta_banded_plan_annotate", "ta_align_batch_banded",
]
ABI_SYMBOLS += BANDED_ABI_SYMBOLS
# The banded affine extension's symbols (checked by tests/test_banded_affine_ref.py).
BANDED_AFFINE_ABI_SYMBOLS = [s.replace("banded", "banded_affine") for s in BANDED_ABI_SYMBOLS]
ABI_SYMBOLS += BANDED_AFFINE_ABI_SYMBOLS
# Exact banded alignment's symbols (checked by tests/test_band_exact_ref.py).
BAND_EXACT_ABI_SYMBOLS = [
    "ta_banded_plan_certify", "ta_banded_affine_plan_certify", "ta_align_batch_banded_exact",
    "ta_align_batch_banded_affine_exact",
]
ABI_SYMBOLS += BAND_EXACT_ABI_SYMBOLS
# Anchored (free-end) alignment's symbols (checked by tests/test_anchored_ref.py).
ANCHORED_ABI_SYMBOLS = [s.replace("banded", "anchored") for s in BANDED_ABI_SYMBOLS] + ["ta_anchored_plan_ends"]
ABI_SYMBOLS += ANCHORED_ABI_SYMBOLS
# Z-drop on anchored alignment (checked by tests/test_anchored_zdrop_ref.py).
ANCHORED_ZDROP_ABI_SYMBOLS = ["ta_anchored_plan_create_zdrop", "ta_anchored_plan_swept_steps",
                              "ta_align_batch_anchored_zdrop"]
ABI_SYMBOLS += ANCHORED_ZDROP_ABI_SYMBOLS
# The row-stripe z-drop rule's entries (checked by tests/test_anchored_zdrop_stripe_ref.py).
ANCHORED_ZDROP_RULE_ABI_SYMBOLS = ["ta_anchored_plan_create_zdrop_rule", "ta_align_batch_anchored_zdrop_rule"]
ABI_SYMBOLS += ANCHORED_ZDROP_RULE_ABI_SYMBOLS
TA_ZDROP_SEGMENT, TA_ZDROP_STRIPE = 0, 1  # the z-drop rules of include/team_align_c.h
TA_ANCHORED_AFFINE_KERNELS = 1  # ta_anchored_plan_create flag: the affine kernels even at gap_open == 0
# The drop-in C++ entry point (team_alignment.hpp), g++/libstdc++ cxx11 mangling.
TEAM_ALIGN_SYMBOL = ("_ZN4team5AlignEPKcjS1_jNS_13AlignmentTypeEiiiPNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEEPj")


def _check_type(type) -> int:
    t = int(type)
    if t not in (0, 1, 2):
        raise ValueError("Unknown AlignmentType provided.")
    return t


def _raise(status: int, ctx=None):
    L = lib()
    msg = L.ta_status_string(status).decode()
    if status in (TA_ERR_BAD_TYPE, TA_ERR_CIGAR, TA_ERR_RANGE):
        raise ValueError(msg)
    detail = L.ta_last_error(ctx).decode() if ctx else ""
    raise DeviceError(f"{msg}: {detail}" if detail else msg)


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _band_array(band, n_pairs: int) -> np.ndarray:
    """A band per pair as uint32 [P]: an int applies to every pair."""
    if np.ndim(band) == 0:
        b = np.full(n_pairs, int(band), np.int64)
    else:
        b = np.asarray(band, np.int64).reshape(-1)
        if b.size != n_pairs:
            raise ValueError(f"band: {b.size} entries for {n_pairs} pairs")
    if b.size and (b.min() < 0 or b.max() > 0xFFFFFFFF):
        raise ValueError("band: values must be in [0, 2^32)")
    return np.ascontiguousarray(b.astype(np.uint32))


def _check_zdrop(zdrop):
    """None (off) or an int in [0, INT32_MAX]."""
    if zdrop is None:
        return None
    if isinstance(zdrop, bool) or not isinstance(zdrop, (int, np.integer)) or not 0 <= int(zdrop) <= 0x7FFFFFFF:
        raise ValueError(f"zdrop: an int in [0, 2^31) or None, not {zdrop!r}")
    return int(zdrop)


def _check_zdrop_rule(rule) -> int:
    """"segment" (the rule on the fill's 64-step segments) or "stripe" (on 16-row stripes) -> TA_ZDROP_*."""
    if not isinstance(rule, str) or rule not in ("segment", "stripe"):
        raise ValueError(f'zdrop_rule: "segment" or "stripe", not {rule!r}')
    return TA_ZDROP_STRIPE if rule == "stripe" else TA_ZDROP_SEGMENT


@dataclass
class BatchResult:
    scores: np.ndarray  # int32 [P]
    target_begins: np.ndarray  # uint32 [P]
    cigar_offsets: np.ndarray | None  # uint64 [P]
    cigar_lens: np.ndarray | None  # uint32 [P]
    arena: np.ndarray | None  # uint8
    band_used: np.ndarray | None = None  # uint32 [P], the exact banded entries: the band of each result
    rounds: np.ndarray | None = None  # uint8 [P], the exact banded entries: 1 or 2
    query_ends: np.ndarray | None = None  # uint32 [P], the anchored entries: the goal cell's row
    target_ends: np.ndarray | None = None  # uint32 [P], ... and its column
    swept_steps: np.ndarray | None = None  # uint32 [P], the anchored entries with zdrop: the fill steps executed

    def cigar(self, p: int) -> bytes | None:
        if self.arena is None:
            return None
        o = int(self.cigar_offsets[p])
        return self.arena[o : o + int(self.cigar_lens[p])].tobytes()

    def cigars(self):
        return [self.cigar(p) for p in range(len(self.scores))]


class Aligner:
    """A device context (HIP stream + staging buffers) on one gfx950 GPU."""

    def __init__(self, device: int = 0):
        L = lib()
        h = C.c_void_p()
        r = L.ta_context_create(device, C.byref(h))
        if r != TA_OK:
            raise DeviceError(f"ta_context_create(device={device}): {L.ta_status_string(r).decode()}")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().ta_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def release(self):
        """ta_context_release: free the cached device workspace and staging."""
        lib().ta_context_release(self._h)

    def align_batch(self, batch, type, match: int, mismatch: int, gap: int, want_cigar: bool = True) -> BatchResult:
        """Batched team::Align over a bioinfo1_amd.synth.PairBatch."""
        return self._batch(batch, type, (match, mismatch, gap), want_cigar, affine=False)

    def align_batch_affine(self, batch, type, match: int, mismatch: int, gap_open: int, gap_extend: int,
                           want_cigar: bool = True) -> BatchResult:
        """The affine-gap extension (ta_align_batch_affine): a gap of length L costs
        gap_open + L*gap_extend.  No reference counterpart; gap_open == 0 gives
        exactly team::Align with gap = gap_extend."""
        return self._batch(batch, type, (match, mismatch, gap_open, gap_extend), want_cigar, affine=True)

    def align_batch_banded(self, batch, type, match: int, mismatch: int, gap: int, band,
                           want_cigar: bool = True) -> BatchResult:
        """The banded extension (ta_align_batch_banded): only the cells with
        min(0, m-n) - band <= j - i <= max(0, m-n) + band exist.  band: an int
        or one per pair.  No reference counterpart; a band >= max(n, m) gives
        exactly team::Align."""
        return self._batch(batch, type, (match, mismatch, gap), want_cigar, affine=False,
                           band=_band_array(band, batch.n_pairs))

    def align_batch_banded_affine(self, batch, type, match: int, mismatch: int, gap_open: int, gap_extend: int, band,
                                  want_cigar: bool = True) -> BatchResult:
        """The banded affine extension (ta_align_batch_banded_affine): the
        affine-gap extension over the cells of the banded extension's band.
        band: an int or one per pair.  gap_open == 0 gives exactly
        align_batch_banded with gap = gap_extend; a band >= max(n, m) exactly
        align_batch_affine."""
        return self._batch(batch, type, (match, mismatch, gap_open, gap_extend), want_cigar, affine=True,
                           band=_band_array(band, batch.n_pairs))

    def align_batch_banded_exact(self, batch, type, match: int, mismatch: int, gap: int, band_start=None,
                                 want_cigar: bool = True) -> BatchResult:
        """align_batch's results at banded cost (ta_align_batch_banded_exact):
        every pair runs at its start band (band_start: an int, one per pair,
        or None for max(64, ceil(min(n, m) / 16))); the pairs whose score does
        not certify their band run once more at the band that must.  The
        result also carries band_used and rounds (1 or 2) per pair."""
        return self._batch(batch, type, (match, mismatch, gap), want_cigar, affine=False, exact=True,
                           band=None if band_start is None else _band_array(band_start, batch.n_pairs))

    def align_batch_banded_affine_exact(self, batch, type, match: int, mismatch: int, gap_open: int, gap_extend: int,
                                        band_start=None, want_cigar: bool = True) -> BatchResult:
        """align_batch_affine's results at banded cost
        (ta_align_batch_banded_affine_exact); as align_batch_banded_exact."""
        return self._batch(batch, type, (match, mismatch, gap_open, gap_extend), want_cigar, affine=True, exact=True,
                           band=None if band_start is None else _band_array(band_start, batch.n_pairs))

    def align_batch_anchored(self, batch, match: int, mismatch: int, gap: int, band, gap_open: int = 0,
                             want_cigar: bool = True, zdrop=None, zdrop_rule: str = "segment") -> BatchResult:
        """Anchored (free-end) alignment (ta_align_batch_anchored): every path
        starts at (0, 0) and ends at the best in-band interior cell, or stays
        at (0, 0) with score 0 when none is positive.  band: an int or one
        per pair.  gap_open == 0: linear gaps; else affine with gap_extend =
        gap.  The result carries query_ends / target_ends (the goal cells);
        target_begins is all 0.  zdrop=Z (an int >= 0): the sweep of a pair
        stops once a 64-step segment's best has fallen more than Z below the
        best so far (ta_align_batch_anchored_zdrop; a scoring with negative
        drift, e.g. 2/-4/-4, is what makes a dead end fall), and the result
        carries swept_steps.  zdrop=None: off.  zdrop_rule="stripe": the drop
        is decided on 16-row stripes instead (ta_align_batch_anchored_zdrop_rule,
        TA_ZDROP_STRIPE) -- the rule to use above band 32, where the segment
        rule can clip a live end longer than 1,024 bases at a pass boundary."""
        z = _check_zdrop(zdrop)
        rule = _check_zdrop_rule(zdrop_rule)
        L = lib()
        P = batch.n_pairs
        bd = _band_array(band, P)
        sc = np.zeros(P, np.int32)
        qe = np.zeros(P, np.uint32)
        te = np.zeros(P, np.uint32)
        coff = clen = arena = None
        cap = 0
        if want_cigar:
            cap = int((2 * (batch.qlen.astype(np.uint64) + batch.tlen.astype(np.uint64)) + 2).sum()) if P else 0
            arena = np.zeros(max(cap, 1), np.uint8)
            coff = np.zeros(P, np.uint64)
            clen = np.zeros(P, np.uint32)
        qb = batch.qbytes if batch.qbytes.size else np.zeros(1, np.uint8)
        tbb = batch.tbytes if batch.tbytes.size else np.zeros(1, np.uint8)
        steps = None if z is None else np.zeros(P, np.uint32)
        tail = () if z is None else (z, _p(steps, C.c_uint32)) if rule == TA_ZDROP_SEGMENT else (
            z, rule, _p(steps, C.c_uint32))
        r = (L.ta_align_batch_anchored if z is None else L.ta_align_batch_anchored_zdrop if rule == TA_ZDROP_SEGMENT
             else L.ta_align_batch_anchored_zdrop_rule)(
            self._h, P, qb.ctypes.data, _p(batch.qoff, C.c_uint64), _p(batch.qlen, C.c_uint32), tbb.ctypes.data,
            _p(batch.toff, C.c_uint64), _p(batch.tlen, C.c_uint32),
            _p(bd if bd.size else np.zeros(1, np.uint32), C.c_uint32), match, mismatch, gap_open, gap,
            int(bool(want_cigar)), _p(sc, C.c_int32), _p(qe, C.c_uint32), _p(te, C.c_uint32),
            arena.ctypes.data if want_cigar else None, cap, _p(coff, C.c_uint64) if want_cigar else None,
            _p(clen, C.c_uint32) if want_cigar else None, *tail)
        if r != TA_OK:
            _raise(r, self._h)
        return BatchResult(sc, np.zeros(P, np.uint32), coff, clen, arena, query_ends=qe, target_ends=te,
                           swept_steps=steps)

    def _batch(self, batch, type, scoring, want_cigar, affine, band=None, exact=False) -> BatchResult:
        L = lib()
        t = _check_type(type)
        P = batch.n_pairs
        sc = np.zeros(P, np.int32)
        tb = np.zeros(P, np.uint32)
        coff = clen = arena = None
        cap = 0
        if want_cigar:
            cap = int((2 * (batch.qlen.astype(np.uint64) + batch.tlen.astype(np.uint64)) + 2).sum()) if P else 0
            arena = np.zeros(max(cap, 1), np.uint8)
            coff = np.zeros(P, np.uint64)
            clen = np.zeros(P, np.uint32)
        qb = batch.qbytes if batch.qbytes.size else np.zeros(1, np.uint8)
        tbb = batch.tbytes if batch.tbytes.size else np.zeros(1, np.uint8)
        fn = L.ta_align_batch_affine if affine else L.ta_align_batch
        extra = tail = ()
        used = rounds = None
        if exact:
            fn = L.ta_align_batch_banded_affine_exact if affine else L.ta_align_batch_banded_exact
            extra = (None if band is None else _p(band if band.size else np.zeros(1, np.uint32), C.c_uint32),)
            used = np.zeros(P, np.uint32)
            rounds = np.zeros(P, np.uint8)
            tail = (_p(used, C.c_uint32), _p(rounds, C.c_uint8))
        elif band is not None:
            fn = L.ta_align_batch_banded_affine if affine else L.ta_align_batch_banded
            extra = (_p(band if band.size else np.zeros(1, np.uint32), C.c_uint32),)
        r = fn(
            self._h, P, qb.ctypes.data, _p(batch.qoff, C.c_uint64), _p(batch.qlen, C.c_uint32), tbb.ctypes.data,
            _p(batch.toff, C.c_uint64), _p(batch.tlen, C.c_uint32), *extra, t, *scoring, int(bool(want_cigar)),
            _p(sc, C.c_int32), _p(tb, C.c_uint32), arena.ctypes.data if want_cigar else None, cap,
            _p(coff, C.c_uint64) if want_cigar else None, _p(clen, C.c_uint32) if want_cigar else None, *tail)
        if r != TA_OK:
            _raise(r, self._h)
        return BatchResult(sc, tb, coff, clen, arena, used, rounds)


_default: Aligner | None = None


def default_aligner() -> Aligner:
    global _default
    if _default is None:
        _default = Aligner(0)
    return _default


def align(query: bytes, target: bytes, type, match: int, mismatch: int, gap: int, want_cigar: bool = True):
    """team::Align for one pair -> (score, cigar bytes or None, target_begin)."""
    from .synth import from_pairs

    _check_type(type)
    res = default_aligner().align_batch(from_pairs([(bytes(query), bytes(target))]), type, match, mismatch, gap,
                                        want_cigar)
    return int(res.scores[0]), res.cigar(0), int(res.target_begins[0])


def align_affine(query: bytes, target: bytes, type, match: int, mismatch: int, gap_open: int, gap_extend: int,
                 want_cigar: bool = True):
    """The affine-gap extension for one pair -> (score, cigar bytes or None, target_begin)."""
    from .synth import from_pairs

    _check_type(type)
    res = default_aligner().align_batch_affine(from_pairs([(bytes(query), bytes(target))]), type, match, mismatch,
                                               gap_open, gap_extend, want_cigar)
    return int(res.scores[0]), res.cigar(0), int(res.target_begins[0])


def align_banded(query: bytes, target: bytes, type, match: int, mismatch: int, gap: int, band: int,
                 want_cigar: bool = True):
    """The banded extension for one pair -> (score, cigar bytes or None, target_begin)."""
    from .synth import from_pairs

    _check_type(type)
    res = default_aligner().align_batch_banded(from_pairs([(bytes(query), bytes(target))]), type, match, mismatch,
                                               gap, band, want_cigar)
    return int(res.scores[0]), res.cigar(0), int(res.target_begins[0])


def align_banded_affine(query: bytes, target: bytes, type, match: int, mismatch: int, gap_open: int, gap_extend: int,
                        band: int, want_cigar: bool = True):
    """The banded affine extension for one pair -> (score, cigar bytes or None, target_begin)."""
    from .synth import from_pairs

    _check_type(type)
    res = default_aligner().align_batch_banded_affine(from_pairs([(bytes(query), bytes(target))]), type, match,
                                                      mismatch, gap_open, gap_extend, band, want_cigar)
    return int(res.scores[0]), res.cigar(0), int(res.target_begins[0])


def align_anchored(query: bytes, target: bytes, match: int, mismatch: int, gap: int, band: int, gap_open: int = 0,
                   want_cigar: bool = True, zdrop=None, zdrop_rule: str = "segment"):
    """Anchored alignment for one pair -> (score, cigar bytes or None, query_end, target_end).
    zdrop, zdrop_rule: as Aligner.align_batch_anchored."""
    from .synth import from_pairs

    res = default_aligner().align_batch_anchored(from_pairs([(bytes(query), bytes(target))]), match, mismatch, gap,
                                                 band, gap_open, want_cigar, zdrop=zdrop,
                                                 zdrop_rule=zdrop_rule)
    return int(res.scores[0]), res.cigar(0), int(res.query_ends[0]), int(res.target_ends[0])


def align_banded_exact(query: bytes, target: bytes, type, match: int, mismatch: int, gap: int, band_start=None,
                       want_cigar: bool = True, gap_open=None):
    """Exact banded alignment for one pair -> (score, cigar bytes or None,
    target_begin): align()'s result (gap_open=o: align_affine()'s, with
    gap_extend = gap) computed inside a certified band."""
    from .synth import from_pairs

    _check_type(type)
    b = from_pairs([(bytes(query), bytes(target))])
    if gap_open is None:
        res = default_aligner().align_batch_banded_exact(b, type, match, mismatch, gap, band_start, want_cigar)
    else:
        res = default_aligner().align_batch_banded_affine_exact(b, type, match, mismatch, gap_open, gap, band_start,
                                                                want_cigar)
    return int(res.scores[0]), res.cigar(0), int(res.target_begins[0])


def align_annotated(query: bytes, target: bytes, type, match: int, mismatch: int, gap: int, gap_open=None):
    """One pair through a DevicePlan with the annotate pass ->
    (score, cigar bytes, target_begin, info dict, =/X cigar bytes).
    gap_open=None: linear gaps; else the affine extension with gap_extend = gap."""
    from .synth import from_pairs

    _check_type(type)
    plan = DevicePlan(default_aligner(), from_pairs([(bytes(query), bytes(target))]), type, match, mismatch, gap,
                      want_cigar=True, gap_open=gap_open)
    try:
        plan.run()
        plan.annotate(eqx=True)
        res = plan.results()
        ann = plan.annotation()
    finally:
        plan.close()
    info = {f: int(ann.info[f][0]) for f in PAIR_INFO_DTYPE.names}
    return int(res.scores[0]), res.cigar(0), int(res.target_begins[0]), info, ann.eqx(0)


class Server:
    """The low-latency single-pair path (ta_server_*): a resident kernel, one
    wave per slot, serves one team::Align call at a time per slot -- what the
    drop-in team::Align uses for pairs up to 4096 x 16384.  align() returns
    (score, cigar bytes or None, target_begin) like align(); a pair outside
    the server's limits raises LookupError (the caller takes a batch)."""

    def __init__(self, device: int, type, slots: int = 32):
        L = lib()
        h = C.c_void_p()
        r = L.ta_server_create(device, _check_type(type), slots, C.byref(h))
        if r != TA_OK:
            _raise(r)
        self._h = h
        self.type = int(type)

    def fits(self, n: int, m: int, match: int, mismatch: int, gap: int) -> bool:
        return bool(lib().ta_server_fits(self._h, n, m, match, mismatch, gap))

    def running(self) -> bool:
        return bool(lib().ta_server_running(self._h))

    def last_times(self, slot: int = 0):
        """Device phase times (us) of slot's last request: request + bytes to HBM,
        fill + walk, results out, 0 (the release store of `done` is the fence)."""
        out = (C.c_double * 4)()
        r = lib().ta_server_last_times(self._h, slot, out)
        if r != TA_OK:
            _raise(r)
        return list(out)

    def align(self, query: bytes, target: bytes, match: int, mismatch: int, gap: int, want_cigar: bool = True):
        query, target = bytes(query), bytes(target)
        cap = 2 * (len(query) + len(target)) + 2
        buf = C.create_string_buffer(cap) if want_cigar else None
        sc, tb, cl = C.c_int32(0), C.c_uint32(0), C.c_uint32(0)
        r = lib().ta_server_align(self._h, query, len(query), target, len(target), match, mismatch, gap,
                                  int(bool(want_cigar)), C.byref(sc), C.byref(tb), buf, cap, C.byref(cl))
        if r == TA_ERR_UNSERVED:
            raise LookupError("pair outside the single-pair server's limits")
        if r != TA_OK:
            _raise(r)
        return sc.value, (buf.raw[: cl.value] if want_cigar else None), tb.value

    def close(self):
        if getattr(self, "_h", None):
            lib().ta_server_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceIO(C.Structure):
    _fields_ = [("query_bytes", C.c_void_p), ("query_off", C.c_void_p), ("target_bytes", C.c_void_p),
                ("target_off", C.c_void_p), ("score", C.c_void_p), ("target_begin", C.c_void_p),
                ("cigar_slots", C.c_void_p), ("cigar_start", C.c_void_p), ("cigar_len", C.c_void_p)]


class PairInfo(C.Structure):
    """ta_pair_info (include/team_align_c.h)."""

    _fields_ = [(f, C.c_uint32) for f in ("query_begin", "query_end", "target_begin", "target_end", "n_eq", "n_x",
                                          "n_ins", "n_del", "n_gap_runs", "n_free")]


PAIR_INFO_DTYPE = np.dtype([(f, np.uint32) for f, _ in PairInfo._fields_])


class _AnnotateIO(C.Structure):
    _fields_ = [("info", C.c_void_p), ("eqx_slots", C.c_void_p), ("eqx_start", C.c_void_p), ("eqx_len", C.c_void_p)]


@dataclass
class Annotation:
    """What DevicePlan.annotation() returns: ``info`` is a structured array
    [P] with ta_pair_info's fields; ``eqx(p)`` the pair's =/X CIGAR bytes."""

    info: np.ndarray
    eqx_starts: np.ndarray | None
    eqx_lens: np.ndarray | None
    eqx_arena: np.ndarray | None

    def eqx(self, p: int) -> bytes | None:
        if self.eqx_arena is None:
            return None
        o = int(self.eqx_starts[p])
        return self.eqx_arena[o : o + int(self.eqx_lens[p])].tobytes()


def _results(o) -> BatchResult:
    o.torch.cuda.synchronize(o.dev)
    sc = o.score.cpu().numpy()
    tb = o.target_begin.cpu().numpy().view(np.uint32)
    if not o.want_cigar:
        return BatchResult(sc, tb, None, None, None)
    start = o.cigar_start.cpu().numpy().view(np.uint64)
    ln = o.cigar_len.cpu().numpy().view(np.uint32)
    slots = o.slots.cpu().numpy()
    return BatchResult(sc, tb, start, ln, slots)


class DevicePlan:
    """Device-resident batch: inputs and outputs are torch tensors in HBM.

    Mirrors the mapper-side batching of SURVEY §8f: lengths and scoring are
    fixed at plan time; ``run()`` enqueues the fill + traceback kernels on the
    current torch stream (asynchronous)."""

    def __init__(self, aligner: Aligner, batch, type, match, mismatch, gap, want_cigar=True, device=None,
                 workspace_budget: int = 0, gap_open=None, flags: int = 0, inputs=None, records=None, band=None,
                 _banded_affine: bool = False, _anchored: bool = False, _zdrop=None,
                 _zdrop_rule: str = "segment"):
        """gap_open=None: team::Align's linear gap.  gap_open=o: the affine-gap
        extension (ta_affine_plan_*) with gap_extend = gap.  flags: TA_PLAN_*
        kernel selection (tests / measurements; same results).  inputs: the
        batch already in HBM as (query bytes, query offsets, target bytes,
        target offsets) tensors -- then only batch.qlen / batch.tlen are read.
        records: an int32 device tensor of >= 3 * P entries that receives the
        scores, target_begins and CIGAR lengths back to back (one download).
        band=None: the whole matrix.  band=w (an int, or one per pair): the
        banded extension (ta_banded_plan_*); not together with gap_open --
        the banded affine extension is DevicePlan.banded_affine(...)."""
        import torch

        if band is not None and gap_open is not None and not _banded_affine:
            raise ValueError("band and gap_open cannot be combined here: the banded extension is linear-gap only; "
                             "use DevicePlan.banded_affine(...) for the banded affine extension")
        L = lib()
        t = () if _anchored else (_check_type(type),)  # (the anchored family takes no type)
        self.torch = torch
        self.dev = torch.device("cuda", aligner.device) if device is None else device
        self.P = batch.n_pairs
        self.want_cigar = bool(want_cigar)
        self.affine = gap_open is not None
        self.banded = band is not None
        self.anchored = _anchored
        self.zdrop = _check_zdrop(_zdrop) if _anchored else None
        self.zdrop_rule = _zdrop_rule
        rule = _check_zdrop_rule(_zdrop_rule)
        family = ("ta_anchored_plan_" if _anchored else "ta_banded_affine_plan_" if self.affine and self.banded else
                  "ta_affine_plan_" if self.affine else "ta_banded_plan_" if self.banded else "ta_plan_")
        self._fn = lambda name: getattr(L, name.replace("ta_plan_", family))
        h = C.c_void_p()
        scoring = (match, mismatch, gap_open, gap) if self.affine else (match, mismatch, gap)
        extra = ()
        if self.banded:
            self.band = _band_array(band, self.P)
            extra = (_p(self.band if self.band.size else np.zeros(1, np.uint32), C.c_uint32),)
        create, ztail = (("ta_plan_create", ()) if self.zdrop is None else
                         ("ta_plan_create_zdrop", (self.zdrop,)) if rule == TA_ZDROP_SEGMENT else
                         ("ta_plan_create_zdrop_rule", (self.zdrop, rule)))
        r = self._fn(create)(aligner.handle, self.P, _p(batch.qlen, C.c_uint32),
                             _p(batch.tlen, C.c_uint32), *extra, *t, *scoring, int(self.want_cigar),
                             workspace_budget, flags, *ztail, C.byref(h))
        if r != TA_OK:
            _raise(r, aligner.handle)
        self._h = h
        self._ctx = aligner.handle
        if inputs is None:
            f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)  # noqa: E731
            self.qbytes = f(batch.qbytes if batch.qbytes.size else np.zeros(1, np.uint8))
            self.tbytes = f(batch.tbytes if batch.tbytes.size else np.zeros(1, np.uint8))
            self.qoff = f(batch.qoff.view(np.int64))
            self.toff = f(batch.toff.view(np.int64))
        else:
            self.qbytes, self.qoff, self.tbytes, self.toff = inputs
        if records is not None:
            assert records.dtype == torch.int32 and records.numel() >= 3 * self.P and records.is_contiguous()
            self.score, self.target_begin = records[:self.P], records[self.P:2 * self.P]
        else:
            self.score = torch.zeros(self.P, dtype=torch.int32, device=self.dev)
            self.target_begin = torch.zeros(self.P, dtype=torch.int32, device=self.dev)
        self.slots_bytes = int(self._fn("ta_plan_cigar_slots_bytes")(h))
        self.slots = torch.zeros(max(self.slots_bytes, 1) if self.want_cigar else 1, dtype=torch.uint8,
                                 device=self.dev)
        self.cigar_start = torch.zeros(self.P, dtype=torch.int64, device=self.dev)
        self.cigar_len = (records[2 * self.P:3 * self.P] if records is not None
                          else torch.zeros(self.P, dtype=torch.int32, device=self.dev))
        self.io = _DeviceIO(self.qbytes.data_ptr(), self.qoff.data_ptr(), self.tbytes.data_ptr(),
                            self.toff.data_ptr(), self.score.data_ptr(), self.target_begin.data_ptr(),
                            self.slots.data_ptr(), self.cigar_start.data_ptr(), self.cigar_len.data_ptr())
        self.workspace_bytes = int(self._fn("ta_plan_workspace_bytes")(h))
        self.chunks = int(self._fn("ta_plan_chunks")(h))
        linear = not (self.affine or self.banded)
        self.dual_pairs = (0 if self.banded else int(L.ta_affine_plan_dual_pairs(h)) if self.affine else
                           int(L.ta_plan_dual_pairs(h)))
        self.flex_pairs = int(L.ta_plan_flex_pairs(h)) if linear else 0
        self.fused = bool(L.ta_plan_fused(h)) if linear else False
        w = int(L.ta_plan_walk(h)) if linear else -1
        self.walk, self.blk, self.ck = (w & 0xFF, bool(w & 0x100), bool(w & 0x200)) if w >= 0 else (None, False, False)
        self.aligner = aligner

    @classmethod
    def banded_affine(cls, aligner: Aligner, batch, type, match, mismatch, gap_open, gap_extend, band,
                      want_cigar=True, device=None, workspace_budget: int = 0, inputs=None, records=None):
        """A plan of the banded affine extension (ta_banded_affine_plan_*):
        affine gaps over the cells of the band.  band: an int, or one per
        pair.  The other arguments as the constructor's."""
        return cls(aligner, batch, type, match, mismatch, gap_extend, want_cigar, device, workspace_budget,
                   gap_open=gap_open, inputs=inputs, records=records, band=band, _banded_affine=True)

    @classmethod
    def anchored(cls, aligner: Aligner, batch, match, mismatch, gap, band, gap_open: int = 0, want_cigar=True,
                 workspace_budget: int = 0, flags: int = 0, device=None, inputs=None, records=None, zdrop=None,
                 zdrop_rule: str = "segment"):
        """A plan of anchored (free-end) alignment (ta_anchored_plan_*): every
        path starts at (0, 0) and ends at the best in-band interior cell.
        band: an int, or one per pair.  gap_open == 0: the linear kernels
        (flags=TA_ANCHORED_AFFINE_KERNELS: the affine ones); else affine gaps
        with gap_extend = gap.  run / results / annotate / pair_chunks /
        band_cells / swept_cells as on a banded plan; ends() returns the goal
        cells; certify() raises.  zdrop=Z (an int >= 0): a z-drop plan
        (ta_anchored_plan_create_zdrop) -- sized as without it; swept_steps()
        returns the fill steps each pair executed.  zdrop_rule="stripe": the
        row-stripe rule (ta_anchored_plan_create_zdrop_rule), the one to use
        above band 32; the plan is sized and driven as the segment rule's."""
        return cls(aligner, batch, None, match, mismatch, gap, want_cigar, device, workspace_budget,
                   gap_open=int(gap_open), flags=flags, inputs=inputs, records=records, band=band,
                   _banded_affine=True, _anchored=True, _zdrop=zdrop, _zdrop_rule=zdrop_rule)

    def swept_steps_async(self):
        """Z-drop plans: enqueue the copy of the last run()'s (or fills') per-pair
        step counts on the current stream (ta_anchored_plan_swept_steps) -> an
        int32 device tensor, allocated on first use."""
        if not self.anchored or self.zdrop is None:
            raise AttributeError("swept_steps: not a z-drop plan")
        if getattr(self, "swept", None) is None:
            self.swept = self.torch.zeros(max(self.P, 1), dtype=self.torch.int32, device=self.dev)
        r = lib().ta_anchored_plan_swept_steps(self._h, self.swept.data_ptr(), self._stream())
        if r != TA_OK:
            _raise(r, self._ctx)
        return self.swept

    def swept_steps(self):
        """Z-drop plans, after run() or the fills: uint32 numpy array [P]."""
        s = self.swept_steps_async()
        self.torch.cuda.synchronize(self.dev)
        return s[:self.P].cpu().numpy().view(np.uint32)

    def ends_async(self):
        """Anchored plans: enqueue the copy of the last run()'s goal cells on the
        current stream (ta_anchored_plan_ends) -> (query_end, target_end)
        int32 device tensors, allocated on first use."""
        if not self.anchored:
            raise AttributeError("ends: not an anchored plan")
        torch = self.torch
        if getattr(self, "query_end", None) is None:
            self.query_end = torch.zeros(max(self.P, 1), dtype=torch.int32, device=self.dev)
            self.target_end = torch.zeros(max(self.P, 1), dtype=torch.int32, device=self.dev)
        r = lib().ta_anchored_plan_ends(self._h, self.query_end.data_ptr(), self.target_end.data_ptr(),
                                        self._stream())
        if r != TA_OK:
            _raise(r, self._ctx)
        return self.query_end, self.target_end

    def ends(self):
        """Anchored plans, after run() or the fills: (query_end, target_end) uint32 numpy arrays [P]."""
        qe, te = self.ends_async()
        self.torch.cuda.synchronize(self.dev)
        return qe[:self.P].cpu().numpy().view(np.uint32), te[:self.P].cpu().numpy().view(np.uint32)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    @property
    def band_cells(self) -> int:
        """Banded plans: the in-band interior cells of all pairs (ta_banded_plan_band_cells)."""
        if not self.banded:
            raise AttributeError("band_cells: not a banded plan")
        return int(self._fn("ta_plan_band_cells")(self._h))

    @property
    def swept_cells(self) -> int:
        """Banded plans: the cells the kernels sweep (ta_banded_plan_swept_cells)."""
        if not self.banded:
            raise AttributeError("swept_cells: not a banded plan")
        return int(self._fn("ta_plan_swept_cells")(self._h))

    def set_inputs(self, inputs):
        """Point the plan at another batch of the same shapes already in HBM:
        (query bytes, query offsets, target bytes, target offsets) tensors --
        pair p must keep its planned lengths.  Takes effect for the launches
        enqueued after the call; the caller keeps the tensors unmodified until
        those launches are done."""
        q, qo, t, to = inputs
        assert q.device == self.dev and t.device == self.dev and qo.numel() >= self.P and to.numel() >= self.P
        self.qbytes, self.qoff, self.tbytes, self.toff = q, qo, t, to
        self.io.query_bytes, self.io.query_off = q.data_ptr(), qo.data_ptr()
        self.io.target_bytes, self.io.target_off = t.data_ptr(), to.data_ptr()

    def run(self):
        r = self._fn("ta_plan_execute")(self._h, C.byref(self.io), self._stream())
        if r != TA_OK:
            _raise(r, self._ctx)

    def run_fill(self, chunk: int = 0):
        r = self._fn("ta_plan_execute_fill")(self._h, C.byref(self.io), self._stream(), chunk)
        if r != TA_OK:
            _raise(r, self._ctx)

    def run_traceback(self, chunk: int = 0):
        r = self._fn("ta_plan_execute_traceback")(self._h, C.byref(self.io), self._stream(), chunk)
        if r != TA_OK:
            _raise(r, self._ctx)

    def check(self):
        """ta_plan_check after synchronising: raises DeviceError if a kernel reported an internal failure."""
        self.torch.cuda.synchronize(self.dev)
        r = self._fn("ta_plan_check")(self._h)
        if r != TA_OK:
            _raise(r, self._ctx)

    def certify_async(self):
        """Banded plans: enqueue the certificate of the last run() on the
        current stream (ta_banded[_affine]_plan_certify) -> (exact uint8,
        band_needed int32) device tensors, allocated on first use."""
        if not self.banded:
            raise AttributeError("certify: not a banded plan")
        if self.anchored:
            raise AttributeError("certify: certification does not cover anchored plans")
        torch = self.torch
        if getattr(self, "exact", None) is None:
            self.exact = torch.zeros(max(self.P, 1), dtype=torch.uint8, device=self.dev)
            self.band_needed = torch.zeros(max(self.P, 1), dtype=torch.int32, device=self.dev)
        r = self._fn("ta_plan_certify")(self._h, C.byref(self.io), self.exact.data_ptr(),
                                        self.band_needed.data_ptr(), self._stream())
        if r != TA_OK:
            _raise(r, self._ctx)
        return self.exact, self.band_needed

    def certify(self):
        """Banded plans, after run(): (exact, band_needed) numpy arrays [P].
        exact[p] = 1: pair p's score, target_begin and CIGAR are the unbanded
        ones; else band_needed[p] is the band at which they will be (where
        exact, the pair's own clamped band)."""
        ex, need = self.certify_async()
        self.torch.cuda.synchronize(self.dev)
        return ex[:self.P].cpu().numpy(), need[:self.P].cpu().numpy().view(np.uint32)

    def annotate(self, eqx: bool = True):
        """Enqueue the annotate pass (ta_plan_annotate) on the current stream,
        after the run() it annotates: per-pair info records and, with ``eqx``,
        the =/X CIGARs.  The tensors are allocated on first use."""
        torch = self.torch
        if getattr(self, "info", None) is None:
            self.info = torch.zeros((self.P, 10), dtype=torch.int32, device=self.dev)
        if eqx and getattr(self, "eqx_slots", None) is None:
            self.eqx_slots = torch.zeros(max(self.slots_bytes, 1), dtype=torch.uint8, device=self.dev)
            self.eqx_start = torch.zeros(self.P, dtype=torch.int64, device=self.dev)
            self.eqx_len = torch.zeros(self.P, dtype=torch.int32, device=self.dev)
        self._annotated_eqx = bool(eqx)
        aio = _AnnotateIO(self.info.data_ptr(), self.eqx_slots.data_ptr() if eqx else None,
                          self.eqx_start.data_ptr() if eqx else None, self.eqx_len.data_ptr() if eqx else None)
        r = self._fn("ta_plan_annotate")(self._h, C.byref(self.io), C.byref(aio), self._stream())
        if r != TA_OK:
            _raise(r, self._ctx)

    def annotation(self) -> Annotation:
        """Synchronise, check and copy the last annotate()'s outputs to the host."""
        if getattr(self, "info", None) is None:
            raise RuntimeError("annotation(): no annotate() was enqueued")
        self.check()
        info = np.ascontiguousarray(self.info.cpu().numpy()).view(np.uint32).reshape(self.P, 10)
        info = info.view(PAIR_INFO_DTYPE).reshape(self.P)
        if not self._annotated_eqx:
            return Annotation(info, None, None, None)
        return Annotation(info, self.eqx_start.cpu().numpy().view(np.uint64),
                          self.eqx_len.cpu().numpy().view(np.uint32), self.eqx_slots.cpu().numpy())

    def compact_cigars(self, out=None):
        """The CIGARs packed back to back on the device (ta_compact_cigars on
        the current stream): returns (bytes uint8 tensor, int64 offsets
        tensor [P+1]) -- what a rank hands to an RCCL gather.  ``out``: a
        (bytes, offsets) pair from compact_buffers() to fill instead of fresh
        tensors (a pipeline reusing them per slot)."""
        torch = self.torch
        lens = self.cigar_len.to(torch.int64)
        if out is None:
            off = torch.zeros(self.P + 1, dtype=torch.int64, device=self.dev)
            # a device-side bound keeps this free of host syncs: every CIGAR fits its slot
            dst = torch.empty(max(self.slots_bytes, 1), dtype=torch.uint8, device=self.dev)
        else:
            dst, off = out
        torch.cumsum(lens, 0, out=off[1:])
        r = lib().ta_compact_cigars(self._ctx, self.P, self.slots.data_ptr(), self.cigar_start.data_ptr(),
                                    self.cigar_len.data_ptr(), off.data_ptr(), dst.data_ptr(), self._stream())
        if r != TA_OK:
            _raise(r, self._ctx)
        return dst, off

    def compact_buffers(self):
        """Buffers for compact_cigars(out=...): (bytes, offsets with offsets[0] = 0)."""
        torch = self.torch
        return (torch.empty(max(self.slots_bytes, 1), dtype=torch.uint8, device=self.dev),
                torch.zeros(self.P + 1, dtype=torch.int64, device=self.dev))

    def pair_chunks(self) -> np.ndarray:
        """uint32 [P]: the chunk each pair ran in (ta_plan_pair_chunks)."""
        out = np.zeros(max(self.P, 1), np.uint32)
        r = self._fn("ta_plan_pair_chunks")(self._h, _p(out, C.c_uint32))
        if r != TA_OK:
            _raise(r, self._ctx)
        return out[: self.P]

    def results_at(self, indices) -> BatchResult:
        """Synchronise, check and copy the results of the pairs ``indices`` only
        (the stratified parity checks of a stated-size run): a BatchResult whose
        k-th entry is pair indices[k]."""
        torch = self.torch
        self.check()
        idx = torch.as_tensor(np.asarray(indices, np.int64), device=self.dev)
        sc = self.score[idx].cpu().numpy()
        tb = self.target_begin[idx].cpu().numpy().view(np.uint32)
        if not self.want_cigar:
            return BatchResult(sc, tb, None, None, None)
        start = self.cigar_start[idx].cpu().numpy()
        ln = self.cigar_len[idx].cpu().numpy().view(np.uint32)
        parts, offs, o = [], np.zeros(len(ln), np.uint64), 0
        for k in range(len(ln)):
            parts.append(self.slots[int(start[k]):int(start[k]) + int(ln[k])].cpu().numpy())
            offs[k] = o
            o += int(ln[k])
        arena = np.concatenate(parts) if parts else np.zeros(1, np.uint8)
        return BatchResult(sc, tb, offs, ln, arena)

    def results(self) -> BatchResult:
        """Synchronise, check and copy results to host (CIGARs unpacked from slots)."""
        self.check()
        return _results(self)

    def close(self):
        if getattr(self, "_h", None):
            self._fn("ta_plan_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePipeline:
    """Device-resident batches aligned back to back with batch k's traceback
    running beside batch k+1's fill.

    The traceback of a batch is one long serial walk per pair -- latency-bound,
    about one wave per SIMD -- while the fill is VALU-bound with
    many waves per SIMD, so the two overlap well on one GPU.  Each slot is a
    DevicePlan on its own Aligner context: the context owns the workspace the
    fill writes and the walk reads, and ta_plan_execute_fill / _traceback order
    one context's launches across streams (a slot's traceback waits for its
    fill, its next fill for that traceback).  The streams, events and
    dependencies are the library's (ta_pipeline_* of team_align_c.h,
    csrc/ta_pipeline.cpp): each slot's fills run on a fill stream of the slot's
    own, so a fill also overlaps the tail of the fill before it; tracebacks on
    a high-priority walk stream -- where a traceback is a walk kernel and a run
    formatter (checkpoint and band walks, one chunk) only the walk, and the
    formatter on the caller's stream beside the next walk (``format_split``);
    and the caller's
    current stream waits for each step's traceback, so whatever the caller
    enqueues after step() on its stream (a compaction, a gather, the next
    upload into this step's input buffers) follows it; a slot's next fill also
    waits for that.

    Inputs: every step may align another batch of the planned shapes
    (step(inputs=...), tensors in HBM); the step's fill waits for the
    ``ready`` event (recorded after the batch's upload, e.g. on a copy stream).
    Without ``ready`` the inputs must already be resident (written before the
    pipeline was built, or synchronised): waiting on the caller's stream would
    also wait for the previous step's traceback and serialise the pipeline.  A
    step without inputs realigns the slot's last batch (at construction: the
    shared first batch).  Memory: ``depth`` workspaces (3 by default)."""

    def __init__(self, device: int, batch, type, match, mismatch, gap, want_cigar=True, depth: int = 3,
                 workspace_budget: int = 0, gap_open=None, flags: int = 0, inputs=None, first=None,
                 walk_streams=None, format_stream=None):
        """first: an existing DevicePlan (on its own Aligner) to use as slot 0;
        the other slots then start on its inputs.  depth: the slots (>= 2).
        At 2, fill k+2 waits for walk k, which ends only shortly before fill
        k+1 does, and every other step leaves the chip without a fill; at 3
        a fill is always queued behind the running one (DESIGN 3.12 has the
        measurements; 4 was slower).  A caller that rotates its batches to
        check the pipeline wants a count coprime with the depth, or every
        slot realigns the batch it held last.  walk_streams: the walk streams
        (1 .. depth; step k's traceback runs on stream k % walk_streams, so
        consecutive walks may overlap); None: the library's default, which
        depends on GPU_MAX_HW_QUEUES (ta_pipeline_create_ex in
        team_align_c.h).  ``self.walk_streams`` is the count in use.
        format_stream: None or 0, the library's default -- the run formatter
        on the caller's stream where the plans allow it; 1 keeps it on the
        walk stream behind its walk.  ``self.format_split`` is what is in use
        (True: formatters on the caller's stream)."""
        import torch

        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.aligners, self.plans, self.k = [], [], 0
        for k in range(depth):
            if k == 0 and first is not None:
                self.plans.append(first)
                continue
            al = Aligner(device)
            self.aligners.append(al)
            shared = inputs if not self.plans else (self.plans[0].qbytes, self.plans[0].qoff,
                                                    self.plans[0].tbytes, self.plans[0].toff)
            self.plans.append(DevicePlan(al, batch, type, match, mismatch, gap, want_cigar,
                                         workspace_budget=workspace_budget, gap_open=gap_open, flags=flags,
                                         inputs=shared))
        L = lib()
        handles = (C.c_void_p * len(self.plans))(*[p._h for p in self.plans])
        h = C.c_void_p()
        create = L.ta_pipeline_create_affine_ex if self.plans[0].affine else L.ta_pipeline_create_ex
        # ta_pipeline_options: size, walk_streams, format_stream
        opts = (C.c_uint32 * 3)(12, int(walk_streams or 0), int(format_stream or 0))
        r = create(handles, len(self.plans), opts, C.byref(h))
        if r != TA_OK:
            msg = L.ta_last_error(self.plans[0]._ctx).decode()
            for p in self.plans[1 if first is not None else 0:]:  # (a caller's ``first`` stays open)
                p.close()
            for al in self.aligners:
                al.close()
            if r == TA_ERR_ARG:
                raise ValueError(msg or "ta_pipeline_create: invalid argument")
            raise DeviceError(f"{L.ta_status_string(r).decode()}: {msg}")
        self._h = h
        self.walk_streams = L.ta_pipeline_walk_streams(h)
        self.format_split = bool(L.ta_pipeline_format_split(h))

    @property
    def chunks(self):
        return self.plans[0].chunks

    def step(self, inputs=None, ready=None):
        """Enqueue one batch (ta_pipeline_step): its fill on the slot's fill
        stream, its traceback on the walk stream (the current stream waits for
        it; with ``format_split`` the run formatter is enqueued on the current
        stream itself).  inputs: this batch's
        (query bytes, query offsets, target bytes, target offsets) tensors in
        HBM, same shapes as planned; ready: an event the fill waits for first
        (None: the inputs are resident); ``ready`` without ``inputs`` is a
        ValueError.  Returns the slot's
        DevicePlan (its results are ready on the current stream after the call;
        the inputs may be overwritten by work enqueued on it after the call)."""
        if ready is not None and inputs is None:
            raise ValueError("DevicePipeline.step: ready without inputs (the event belongs to an upload of inputs)")
        plan = self.plans[self.k % len(self.plans)]  # (the library's rotation: step k on slot k % depth)
        if inputs is not None:
            plan.set_inputs(inputs)
        cur = self.torch.cuda.current_stream(self.dev)
        slot = C.c_uint32()
        ev = C.c_void_p(ready.cuda_event) if ready is not None else None
        r = lib().ta_pipeline_step(self._h, C.byref(plan.io), ev, C.c_void_p(cur.cuda_stream), C.byref(slot))
        if r != TA_OK:
            _raise(r, plan._ctx)
        assert self.plans[slot.value] is plan
        self.k += 1
        return plan

    def check(self):
        for p in self.plans:
            p.check()

    def close(self):
        if getattr(self, "_h", None):  # (before the plans and contexts it refers to)
            lib().ta_pipeline_destroy(self._h)
            self._h = None
        for p in self.plans:
            p.close()
        for al in self.aligners:
            al.close()


class HostBatchRunner:
    """Repeated host-memory batches (ta_align_batch) over one batch whose
    inputs and outputs live in pinned host memory (torch pin_memory, i.e.
    hipHostMalloc): what a caller that keeps its reads in pinned buffers gets
    host-to-host.  run() is one call: upload, kernels, download, sync."""

    def __init__(self, aligner: Aligner, batch, type, match, mismatch, gap, want_cigar=True):
        import torch

        self.t = _check_type(type)
        self.sc = (match, mismatch, gap)
        self.want_cigar = bool(want_cigar)
        self.aligner = aligner
        self.P = P = batch.n_pairs

        def pinned(a):
            a = np.ascontiguousarray(a)
            t = torch.empty(max(a.nbytes, 1), dtype=torch.uint8, pin_memory=True)
            v = t.numpy()[: a.nbytes].view(a.dtype)
            v[...] = a.reshape(-1)
            return t, v

        self._keep = []
        for name, a in (("qb", batch.qbytes if batch.qbytes.size else np.zeros(1, np.uint8)), ("qoff", batch.qoff),
                        ("qlen", batch.qlen), ("tb", batch.tbytes if batch.tbytes.size else np.zeros(1, np.uint8)),
                        ("toff", batch.toff), ("tlen", batch.tlen), ("score", np.zeros(P, np.int32)),
                        ("tbeg", np.zeros(P, np.uint32)), ("coff", np.zeros(P, np.uint64)),
                        ("clen", np.zeros(P, np.uint32))):
            t, v = pinned(a)
            self._keep.append(t)
            setattr(self, name, v)
        cap = int((2 * (batch.qlen.astype(np.uint64) + batch.tlen.astype(np.uint64)) + 2).sum()) if P else 1
        t, self.arena = pinned(np.zeros(max(cap, 1), np.uint8))
        self._keep.append(t)
        self.cap = cap

    def run(self):
        L = lib()
        r = L.ta_align_batch(
            self.aligner.handle, self.P, self.qb.ctypes.data, _p(self.qoff, C.c_uint64), _p(self.qlen, C.c_uint32),
            self.tb.ctypes.data, _p(self.toff, C.c_uint64), _p(self.tlen, C.c_uint32), self.t, *self.sc,
            int(self.want_cigar), _p(self.score, C.c_int32), _p(self.tbeg, C.c_uint32), self.arena.ctypes.data,
            self.cap, _p(self.coff, C.c_uint64), _p(self.clen, C.c_uint32))
        if r != TA_OK:
            _raise(r, self.aligner.handle)

    def results(self) -> BatchResult:
        if not self.want_cigar:
            return BatchResult(self.score.copy(), self.tbeg.copy(), None, None, None)
        return BatchResult(self.score.copy(), self.tbeg.copy(), self.coff.copy(), self.clen.copy(), self.arena.copy())


class HostPipeline:
    """Host-resident batches aligned back to back with the PCIe transfers hidden:
    batch k's upload runs on an upload stream and batch k-1's download on a
    download stream while the kernels run on the compute stream.  Inputs are the
    batch's bytes in pinned host memory; every step uploads them, runs the plan,
    compacts the CIGARs on the device and brings the records and the compacted
    CIGAR bytes back into pinned host memory (host inputs to host
    results).

    Two DevicePlans alternate (double-buffered device inputs and outputs), each
    on an Aligner context of its own (the given one and a second), so that, as
    in DevicePipeline, batch k's traceback (high-priority walk stream) runs
    beside batch k+1's fill (fill stream).  Step k enqueues its upload and
    kernels, then waits for step k-1's kernels and downloads step k-1's records
    (12 bytes per pair) and exactly its CIGAR bytes.  Every copy is posted only
    once its data is ready: a copy enqueued ahead of its data (waiting on an
    event) holds its DMA engine, and an upload queued behind it then waits for
    a whole plan (measured: a 0.45 ms bubble every other step)."""

    def __init__(self, aligner: Aligner, batch, type, match, mismatch, gap, want_cigar=True, workspace_budget=0,
                 overlap: bool = True):
        """overlap=False: both slots on ``aligner``'s context, one stream for
        the kernels (each batch's fill after the previous traceback)."""
        import torch

        self.torch = torch
        self.P = P = batch.n_pairs
        self.want_cigar = bool(want_cigar)
        dev = torch.device("cuda", aligner.device)
        self.dev = dev
        qb = batch.qbytes if batch.qbytes.size else np.zeros(1, np.uint8)
        tb = batch.tbytes if batch.tbytes.size else np.zeros(1, np.uint8)
        # query and target bytes in one pinned buffer and one device buffer per
        # slot: one H2D copy per step
        nq = int(qb.size)
        self.h_qt = torch.from_numpy(np.concatenate([np.ascontiguousarray(qb), np.ascontiguousarray(tb)])).pin_memory()
        qoff = torch.from_numpy(batch.qoff.view(np.int64).copy()).to(dev)
        toff = torch.from_numpy(batch.toff.view(np.int64).copy()).to(dev)
        self.d_qt = [torch.empty_like(self.h_qt, device=dev) for _ in range(2)]
        self.d_q = [self.d_qt[i][:nq] for i in range(2)]
        self.d_t = [self.d_qt[i][nq:] for i in range(2)]
        # per slot: scores, target_begins, CIGAR lengths (written there by the plan) + the CIGAR byte total
        self.d_rec = [torch.zeros(3 * P + 1, dtype=torch.int32, device=dev) for _ in range(2)]
        self.second = Aligner(aligner.device) if overlap else None
        self.plans = [DevicePlan(al, batch, type, match, mismatch, gap, want_cigar,
                                 workspace_budget=workspace_budget, inputs=(self.d_q[i], qoff, self.d_t[i], toff),
                                 records=self.d_rec[i])
                      for i, al in enumerate((aligner, self.second or aligner))]
        self.fill, self.up, self.down = (torch.cuda.Stream(dev) for _ in range(3))
        # tracebacks + compaction (DevicePipeline.walk); without overlap the fills run there too
        self.compute = torch.cuda.Stream(dev, priority=-1) if overlap else self.fill
        self.h_rec = [torch.empty(3 * P + 1, dtype=torch.int32, pin_memory=True) for _ in range(2)]
        cap = max(self.plans[0].slots_bytes, 1)
        self.h_cig = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        E = lambda: [torch.cuda.Event() for _ in range(2)]  # noqa: E731
        self.ev_in, self.ev_done, self.ev_rec, self.ev_cig = E(), E(), E(), E()
        # per slot: the compacted CIGAR bytes and offsets, allocated once
        self.cbuf = [self.plans[i].compact_buffers() for i in range(2)] if self.want_cigar else [None, None]
        self.used = [False, False]  # slot has a step in flight (its downloads may still run)
        self.prev = None            # (slot, device CIGAR bytes) of the previous step
        self.last = None
        self.k = 0

    def _download(self, i, dst):
        """Slot i's step, once its kernels are done: the records, then exactly
        its CIGAR bytes (posted only now that their data is ready)."""
        torch = self.torch
        self.ev_done[i].synchronize()  # the step's kernels are done
        with torch.cuda.stream(self.down):
            self.h_rec[i].copy_(self.d_rec[i], non_blocking=True)
            self.ev_rec[i].record(self.down)
        if self.want_cigar:
            self.ev_rec[i].synchronize()
            nbytes = int(self.h_rec[i][3 * self.P])
            with torch.cuda.stream(self.down):
                if nbytes:
                    self.h_cig[i][:nbytes].copy_(dst[:nbytes], non_blocking=True)
                self.ev_cig[i].record(self.down)
        else:
            self.ev_cig[i] = self.ev_rec[i]
        self.last = i

    def step(self):
        torch, P = self.torch, self.P
        i = self.k % 2
        self.k += 1
        # inputs of this step: the kernels of two steps ago (slot i) are done (the
        # host saw them finish during the previous step)
        with torch.cuda.stream(self.up):
            self.d_qt[i].copy_(self.h_qt, non_blocking=True)
            self.ev_in[i].record(self.up)
        plan = self.plans[i]
        with torch.cuda.stream(self.fill):
            self.fill.wait_event(self.ev_in[i])
            if self.used[i]:  # the slot's results of two steps ago are down (a wait on the device)
                self.fill.wait_event(self.ev_cig[i])
            for c in range(plan.chunks):
                plan.run_fill(c)
                with torch.cuda.stream(self.compute):
                    plan.run_traceback(c)  # (after its fill: the slot's context orders them)
        with torch.cuda.stream(self.compute):
            rec = self.d_rec[i]
            dst = None
            if self.want_cigar:
                dst, off = plan.compact_cigars(out=self.cbuf[i])
                rec[3 * P:].copy_(off[-1:], non_blocking=True)
            self.ev_done[i].record(self.compute)
        self.used[i] = True
        if self.prev is not None:  # the previous step's results (its kernels end as this step's begin)
            self._download(*self.prev)
        self.prev = (i, dst)

    def drain(self):
        if self.prev is not None:
            self._download(*self.prev)
            self.prev = None
        self.torch.cuda.synchronize(self.dev)

    def results(self) -> BatchResult:
        """The last drained step's results (host copies)."""
        i, P = self.last, self.P
        rec = self.h_rec[i].numpy()
        sc = rec[:P].copy()
        tb = rec[P:2 * P].copy().view(np.uint32)
        if not self.want_cigar:
            return BatchResult(sc, tb, None, None, None)
        ln = rec[2 * P:3 * P].copy().view(np.uint32)
        off = np.zeros(P, np.uint64)
        if P:
            off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        return BatchResult(sc, tb, off, ln, self.h_cig[i].numpy()[:int(rec[3 * P])].copy())

    def close(self):
        for p in self.plans:
            p.close()
        if self.second:
            self.second.close()
