// bioinfo1_amd/csrc/ta_anchored.cpp -- the ta_anchored_* family of
// include/team_align_c.h: anchored (free-end) alignment, the path fixed at
// (0, 0) and ended where the score is best.
//
// An anchored plan is a banded plan (gap_open == 0: the 2-bit linear kernels)
// or a banded affine plan run in Mode kAnchored (ta_anchored.h); this file only
// chooses between the two and forwards.  The kernels are ta_banded.hip's and
// ta_banded_affine.hip's kAnchored instantiations.
#include "../../include/team_align_c.h"
#include "ta_anchored.h"
#include "ta_context.h"

struct ta_anchored_plan {
    ta_context* ctx = nullptr;
    ta_banded_plan* lin = nullptr;         // exactly one of the two is set
    ta_banded_affine_plan* aff = nullptr;
};

// Forward one entry to whichever family the plan holds.
#define TA_ANCHORED_FWD(pl, none, call_lin, call_aff) \
    (!(pl) ? (none) : (pl)->lin ? (call_lin) : (call_aff))

extern "C" {

int ta_anchored_plan_create(ta_context* ctx, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen,
                            const uint32_t* band, int match, int mismatch, int gap_open, int gap_extend,
                            int want_cigar, uint64_t budget, uint32_t flags, ta_anchored_plan** out) {
    return ta_anchored_plan_create_zdrop(ctx, n_pairs, qlen, tlen, band, match, mismatch, gap_open, gap_extend,
                                         want_cigar, budget, flags, -1, out);
}

int ta_anchored_plan_create_zdrop(ta_context* ctx, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen,
                                  const uint32_t* band, int match, int mismatch, int gap_open, int gap_extend,
                                  int want_cigar, uint64_t budget, uint32_t flags, int32_t zdrop,
                                  ta_anchored_plan** out) {
    return ta_anchored_plan_create_zdrop_rule(ctx, n_pairs, qlen, tlen, band, match, mismatch, gap_open, gap_extend,
                                              want_cigar, budget, flags, zdrop, TA_ZDROP_SEGMENT, out);
}

int ta_anchored_plan_create_zdrop_rule(ta_context* ctx, uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen,
                                       const uint32_t* band, int match, int mismatch, int gap_open, int gap_extend,
                                       int want_cigar, uint64_t budget, uint32_t flags, int32_t zdrop, int rule,
                                       ta_anchored_plan** out) {
    if (!out) return TA_ERR_ARG;
    *out = nullptr;
    if (!ctx) return TA_ERR_ARG;
    if (flags & ~TA_ANCHORED_AFFINE_KERNELS)
        return ta_host::fail(ctx, TA_ERR_ARG, "ta_anchored_plan_create: unknown flag bits");
    if (rule != TA_ZDROP_SEGMENT && rule != TA_ZDROP_STRIPE)
        return ta_host::fail(ctx, TA_ERR_ARG, "ta_anchored_plan_create: unknown z-drop rule");
    auto* pl = new ta_anchored_plan();
    pl->ctx = ctx;
    const bool affine = gap_open != 0 || (flags & TA_ANCHORED_AFFINE_KERNELS);
    const int r = affine ? ta_host::anchored_affine_create(ctx, n_pairs, qlen, tlen, band, match, mismatch, gap_open,
                                                           gap_extend, want_cigar, budget, zdrop, rule, &pl->aff)
                         : ta_host::anchored_linear_create(ctx, n_pairs, qlen, tlen, band, match, mismatch,
                                                           gap_extend, want_cigar, budget, zdrop, rule, &pl->lin);
    if (r != TA_OK) {
        delete pl;
        return r;
    }
    *out = pl;
    return TA_OK;
}

void ta_anchored_plan_destroy(ta_anchored_plan* pl) {
    if (!pl) return;
    ta_banded_plan_destroy(pl->lin);
    ta_banded_affine_plan_destroy(pl->aff);
    delete pl;
}

uint64_t ta_anchored_plan_cigar_slots_bytes(const ta_anchored_plan* pl) {
    return TA_ANCHORED_FWD(pl, 0, ta_banded_plan_cigar_slots_bytes(pl->lin),
                           ta_banded_affine_plan_cigar_slots_bytes(pl->aff));
}
uint64_t ta_anchored_plan_workspace_bytes(const ta_anchored_plan* pl) {
    return TA_ANCHORED_FWD(pl, 0, ta_banded_plan_workspace_bytes(pl->lin),
                           ta_banded_affine_plan_workspace_bytes(pl->aff));
}
uint32_t ta_anchored_plan_chunks(const ta_anchored_plan* pl) {
    return TA_ANCHORED_FWD(pl, 0, ta_banded_plan_chunks(pl->lin), ta_banded_affine_plan_chunks(pl->aff));
}
int ta_anchored_plan_pair_chunks(const ta_anchored_plan* pl, uint32_t* chunk_of_pair) {
    return TA_ANCHORED_FWD(pl, TA_ERR_ARG, ta_banded_plan_pair_chunks(pl->lin, chunk_of_pair),
                           ta_banded_affine_plan_pair_chunks(pl->aff, chunk_of_pair));
}
uint64_t ta_anchored_plan_band_cells(const ta_anchored_plan* pl) {
    return TA_ANCHORED_FWD(pl, 0, ta_banded_plan_band_cells(pl->lin), ta_banded_affine_plan_band_cells(pl->aff));
}
uint64_t ta_anchored_plan_swept_cells(const ta_anchored_plan* pl) {
    return TA_ANCHORED_FWD(pl, 0, ta_banded_plan_swept_cells(pl->lin), ta_banded_affine_plan_swept_cells(pl->aff));
}
int ta_anchored_plan_execute(ta_anchored_plan* pl, const ta_device_io* io, void* stream) {
    return TA_ANCHORED_FWD(pl, TA_ERR_ARG, ta_banded_plan_execute(pl->lin, io, stream),
                           ta_banded_affine_plan_execute(pl->aff, io, stream));
}
int ta_anchored_plan_execute_fill(ta_anchored_plan* pl, const ta_device_io* io, void* stream, uint32_t chunk) {
    return TA_ANCHORED_FWD(pl, TA_ERR_ARG, ta_banded_plan_execute_fill(pl->lin, io, stream, chunk),
                           ta_banded_affine_plan_execute_fill(pl->aff, io, stream, chunk));
}
int ta_anchored_plan_execute_traceback(ta_anchored_plan* pl, const ta_device_io* io, void* stream, uint32_t chunk) {
    return TA_ANCHORED_FWD(pl, TA_ERR_ARG, ta_banded_plan_execute_traceback(pl->lin, io, stream, chunk),
                           ta_banded_affine_plan_execute_traceback(pl->aff, io, stream, chunk));
}
int ta_anchored_plan_check(ta_anchored_plan* pl) {
    return TA_ANCHORED_FWD(pl, TA_ERR_ARG, ta_banded_plan_check(pl->lin), ta_banded_affine_plan_check(pl->aff));
}
int ta_anchored_plan_annotate(ta_anchored_plan* pl, const ta_device_io* io, const ta_annotate_io* out, void* stream) {
    return TA_ANCHORED_FWD(pl, TA_ERR_ARG, ta_banded_plan_annotate(pl->lin, io, out, stream),
                           ta_banded_affine_plan_annotate(pl->aff, io, out, stream));
}
int ta_anchored_plan_ends(ta_anchored_plan* pl, uint32_t* query_end_dev, uint32_t* target_end_dev, void* stream) {
    return TA_ANCHORED_FWD(pl, TA_ERR_ARG,
                           ta_host::anchored_linear_ends(pl->lin, query_end_dev, target_end_dev, stream),
                           ta_host::anchored_affine_ends(pl->aff, query_end_dev, target_end_dev, stream));
}

int ta_anchored_plan_swept_steps(ta_anchored_plan* pl, uint32_t* steps_dev, void* stream) {
    return TA_ANCHORED_FWD(pl, TA_ERR_ARG, ta_host::anchored_linear_swept_steps(pl->lin, steps_dev, stream),
                           ta_host::anchored_affine_swept_steps(pl->aff, steps_dev, stream));
}

int ta_align_batch_anchored(ta_context* ctx, uint32_t n_pairs, const char* qb, const uint64_t* qoff,
                            const uint32_t* qlen, const char* tbytes, const uint64_t* toff, const uint32_t* tlen,
                            const uint32_t* band, int match, int mismatch, int gap_open, int gap_extend,
                            int want_cigar, int32_t* score, uint32_t* query_end, uint32_t* target_end, char* arena,
                            uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len) {
    return ta_align_batch_anchored_zdrop(ctx, n_pairs, qb, qoff, qlen, tbytes, toff, tlen, band, match, mismatch,
                                         gap_open, gap_extend, want_cigar, score, query_end, target_end, arena,
                                         arena_bytes, cigar_off, cigar_len, -1, nullptr);
}

int ta_align_batch_anchored_zdrop(ta_context* ctx, uint32_t n_pairs, const char* qb, const uint64_t* qoff,
                                  const uint32_t* qlen, const char* tbytes, const uint64_t* toff,
                                  const uint32_t* tlen, const uint32_t* band, int match, int mismatch, int gap_open,
                                  int gap_extend, int want_cigar, int32_t* score, uint32_t* query_end,
                                  uint32_t* target_end, char* arena, uint64_t arena_bytes, uint64_t* cigar_off,
                                  uint32_t* cigar_len, int32_t zdrop, uint32_t* swept_steps) {
    return ta_align_batch_anchored_zdrop_rule(ctx, n_pairs, qb, qoff, qlen, tbytes, toff, tlen, band, match, mismatch,
                                              gap_open, gap_extend, want_cigar, score, query_end, target_end, arena,
                                              arena_bytes, cigar_off, cigar_len, zdrop, TA_ZDROP_SEGMENT, swept_steps);
}

int ta_align_batch_anchored_zdrop_rule(ta_context* ctx, uint32_t n_pairs, const char* qb, const uint64_t* qoff,
                                       const uint32_t* qlen, const char* tbytes, const uint64_t* toff,
                                       const uint32_t* tlen, const uint32_t* band, int match, int mismatch,
                                       int gap_open, int gap_extend, int want_cigar, int32_t* score,
                                       uint32_t* query_end, uint32_t* target_end, char* arena, uint64_t arena_bytes,
                                       uint64_t* cigar_off, uint32_t* cigar_len, int32_t zdrop, int rule,
                                       uint32_t* swept_steps) {
    if (!ctx) return TA_ERR_ARG;
    if (rule != TA_ZDROP_SEGMENT && rule != TA_ZDROP_STRIPE)
        return ta_host::fail(ctx, TA_ERR_ARG, "ta_align_batch_anchored: unknown z-drop rule");
    if (gap_open != 0)
        return ta_host::anchored_affine_batch(ctx, n_pairs, qb, qoff, qlen, tbytes, toff, tlen, band, match, mismatch,
                                              gap_open, gap_extend, want_cigar, score, query_end, target_end, arena,
                                              arena_bytes, cigar_off, cigar_len, zdrop, rule, swept_steps);
    return ta_host::anchored_linear_batch(ctx, n_pairs, qb, qoff, qlen, tbytes, toff, tlen, band, match, mismatch,
                                          gap_extend, want_cigar, score, query_end, target_end, arena, arena_bytes,
                                          cigar_off, cigar_len, zdrop, rule, swept_steps);
}

}  // extern "C"
