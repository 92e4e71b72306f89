// bioinfo1_amd/csrc/ta_anchored.h -- what the anchored family's driver
// (ta_anchored.cpp) needs from the two banded families: their plans built in
// Mode kAnchored, the goal cells of an execution, and the host-memory batch.
// The public banded entries keep rejecting every type but the reference's
// three; kAnchored is reached only through these hidden functions.
//
// The plans they make are ordinary ta_banded_plan / ta_banded_affine_plan
// objects: everything else (execute, chunks, annotate, destroy) goes through
// the families' extern "C" entries.
#pragma once

#include <stdint.h>

#include "../../include/team_align_c.h"

#define TA_ANCHORED_LOCAL __attribute__((visibility("hidden")))

namespace ta_host {

// As ta_banded_plan_create / ta_banded_affine_plan_create without `type` and `flags`.
// zdrop >= 0: a z-drop plan (the DROP fills); zdrop < 0: the plain anchored plan.
// zdrop_rule: TA_ZDROP_SEGMENT or TA_ZDROP_STRIPE (checked by the caller), which fills a z-drop plan runs.
TA_ANCHORED_LOCAL int anchored_linear_create(ta_context* ctx, uint32_t n_pairs, const uint32_t* qlen,
                                             const uint32_t* tlen, const uint32_t* band, int match, int mismatch,
                                             int gap, int want_cigar, uint64_t budget, int32_t zdrop,
                                             int zdrop_rule, ta_banded_plan** out);
TA_ANCHORED_LOCAL int anchored_affine_create(ta_context* ctx, uint32_t n_pairs, const uint32_t* qlen,
                                             const uint32_t* tlen, const uint32_t* band, int match, int mismatch,
                                             int gap_open, int gap_extend, int want_cigar, uint64_t budget,
                                             int32_t zdrop, int zdrop_rule, ta_banded_affine_plan** out);
// Enqueue the copy of the plan's goal cells (the last execution's) on `stream`.
TA_ANCHORED_LOCAL int anchored_linear_ends(ta_banded_plan* pl, uint32_t* query_end_dev, uint32_t* target_end_dev,
                                           void* stream);
TA_ANCHORED_LOCAL int anchored_affine_ends(ta_banded_affine_plan* pl, uint32_t* query_end_dev,
                                           uint32_t* target_end_dev, void* stream);
// Z-drop plans: enqueue the copy of the per-pair step counts (the last execution's or fills') on `stream`.
TA_ANCHORED_LOCAL int anchored_linear_swept_steps(ta_banded_plan* pl, uint32_t* steps_dev, void* stream);
TA_ANCHORED_LOCAL int anchored_affine_swept_steps(ta_banded_affine_plan* pl, uint32_t* steps_dev, void* stream);
// As ta_align_batch_banded / _banded_affine without `type`; the goal cells instead of target_begin.
// zdrop as above; swept_steps (z-drop only, may be null): the per-pair step counts.
TA_ANCHORED_LOCAL int anchored_linear_batch(ta_context* ctx, uint32_t n_pairs, const char* qb, const uint64_t* qoff,
                                            const uint32_t* qlen, const char* tbytes, const uint64_t* toff,
                                            const uint32_t* tlen, const uint32_t* band, int match, int mismatch,
                                            int gap, int want_cigar, int32_t* score, uint32_t* query_end,
                                            uint32_t* target_end, char* arena, uint64_t arena_bytes,
                                            uint64_t* cigar_off, uint32_t* cigar_len, int32_t zdrop,
                                            int zdrop_rule, uint32_t* swept_steps);
TA_ANCHORED_LOCAL int anchored_affine_batch(ta_context* ctx, uint32_t n_pairs, const char* qb, const uint64_t* qoff,
                                            const uint32_t* qlen, const char* tbytes, const uint64_t* toff,
                                            const uint32_t* tlen, const uint32_t* band, int match, int mismatch,
                                            int gap_open, int gap_extend, int want_cigar, int32_t* score,
                                            uint32_t* query_end, uint32_t* target_end, char* arena,
                                            uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len,
                                            int32_t zdrop, int zdrop_rule, uint32_t* swept_steps);

}  // namespace ta_host
