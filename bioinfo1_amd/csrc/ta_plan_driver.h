// bioinfo1_amd/csrc/ta_plan_driver.h -- what the host drivers of the plan
// families share (linear gap: ta_api.hip, affine gap: ta_affine.hip, banded:
// ta_banded.hip, banded affine: ta_banded_affine.hip): device-resident create / destroy, the argument
// checks of an execution, the chunk loop, pair_chunks, annotate and the error
// word's check.  The extern "C" entries of include/team_align_c.h forward here.
//
// PL is a family's opaque plan struct.  It derives from the family's device
// arrays (ta_plan_block.h) and holds
//     ta_context* ctx;  <host plan> h;  void* own_block;
//     static int exec_chunk(PL*, const ta_device_io*, hipStream_t, uint32_t c, bool fill, ta::TraceParts trace);
//         (trace: the parts of the traceback to enqueue, or kNoTrace.  A family whose walks write the
//         CIGAR text themselves runs its traceback for kTraceWalk and nothing for kTraceFormat alone.)
//     uint32_t* err_word() const;  // the device word this plan's kernels report errors in, or null
//     static const char* err_message(uint32_t err);  // what a nonzero error word means
// exec_chunk (which kernels a chunk launches, on which streams) is the
// family's own code, as are its planner call and its messages.  The struct is
// defined TA_PLAN_LOCAL: neither its members nor the instantiations below
// belong in the library's dynamic symbol table (the C ABI is the boundary).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "ta_context.h"
#include "ta_internal.h"
#include "ta_plan_block.h"

#define TA_PLAN_LOCAL __attribute__((visibility("hidden")))

namespace ta_host {

inline bool valid_type(int t) { return t == TA_GLOBAL || t == TA_LOCAL || t == TA_SEMI_GLOBAL; }

// The range rule of include/team_align_c.h (the affine oracle's
// oracle_affine_in_range): every |value| < 2^26.  max_step = the largest
// magnitude one step can add (affine: |open| + |extend| among them).
inline bool in_range(uint32_t n_pairs, const uint32_t* qlen, const uint32_t* tlen, long long max_step) {
    uint64_t maxn = 0, maxm = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        maxn = std::max<uint64_t>(maxn, qlen[p]);
        maxm = std::max<uint64_t>(maxm, tlen[p]);
    }
    return (long long)(maxn + maxm + 2) * max_step < (1ll << 26);
}

template <class PL>
void plan_destroy(PL* pl) {
    if (!pl) return;
    if (pl->own_block) {
        (void)hipSetDevice(pl->ctx->device);
        (void)hipFree(pl->own_block);
    }
    delete pl;
}

// Second half of a family's create: pl (new, its host plan built) gets all its
// per-pair arrays in one device allocation, uploaded in one copy.  Owns pl:
// *out on success, destroyed on failure.  who = "ta_..._plan_create: ".
template <class PL>
int plan_create_block(PL* pl, const char* who, PL** out) {
    const ta::BlockSpan span = ta::layout_block(pl->h, *pl);
    std::vector<uint8_t> host(span.upload);
    ta::pack_block(pl->h, *pl, host.data());
    hipError_t e = hipMalloc(&pl->own_block, std::max<uint64_t>(span.bytes, 256));
    if (e == hipSuccess && span.upload) e = hipMemcpy(pl->own_block, host.data(), span.upload, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ta_context* ctx = pl->ctx;
        plan_destroy(pl);
        return fail(ctx, TA_ERR_DEVICE, std::string(who) + hipGetErrorString(e));
    }
    ta::bind_block(pl->h, *pl, static_cast<uint8_t*>(pl->own_block), span);
    *out = pl;
    return TA_OK;
}

template <class PL>
int check_io(PL* pl, const ta_device_io* io) {
    if (!pl || !io) return TA_ERR_ARG;
    if (pl->h.n_pairs && (!io->query_off || !io->target_off || !io->score || !io->target_begin))
        return fail(pl->ctx, TA_ERR_ARG, "null device pointer");
    if (pl->h.want_cigar && pl->h.n_pairs && (!io->cigar_slots || !io->cigar_start || !io->cigar_len))
        return fail(pl->ctx, TA_ERR_ARG, "null cigar device pointer");
    return TA_OK;
}

constexpr ta::TraceParts kNoTrace = ta::TraceParts(0);  // an execution of the fill alone

// chunk == UINT32_MAX: every chunk.  trace: the parts of the traceback to enqueue (an enum, so
// that no caller's `true` arrives as the walk alone).  Called with ctx->mu held.
template <class PL>
int exec(PL* pl, const ta_device_io* io, hipStream_t s, uint32_t chunk, bool fill, ta::TraceParts trace) {
    ta_context* ctx = pl->ctx;
    TA_HIP(ctx, hipSetDevice(ctx->device));
    if (int r = stream_enter(ctx, s)) return r;
    const uint32_t c0 = chunk == UINT32_MAX ? 0 : chunk;
    const uint32_t c1 = chunk == UINT32_MAX ? (uint32_t)pl->h.chunks.size() : chunk + 1;
    for (uint32_t c = c0; c < c1; ++c)
        if (int r = PL::exec_chunk(pl, io, s, c, fill, trace)) return r;
    return stream_leave(ctx, s);
}

template <class PL>
int plan_execute(PL* pl, const ta_device_io* io, void* stream) {
    if (int r = check_io(pl, io)) return r;
    std::lock_guard<std::mutex> lock(pl->ctx->mu);
    return exec(pl, io, (hipStream_t)stream, UINT32_MAX, true, ta::kTraceAll);
}

// One chunk's fill (fill) or traceback (!fill; parts: all of it, or its walk or
// its run formatter alone).  A chunk beyond the last is an error, except on a
// plan of no pairs (which has no chunk to run).
template <class PL>
int plan_execute_chunk(PL* pl, const ta_device_io* io, void* stream, uint32_t chunk, bool fill,
                       ta::TraceParts parts = ta::kTraceAll) {
    if (int r = check_io(pl, io)) return r;
    if (chunk >= pl->h.chunks.size()) return pl->h.n_pairs ? TA_ERR_ARG : TA_OK;
    std::lock_guard<std::mutex> lock(pl->ctx->mu);
    return exec(pl, io, (hipStream_t)stream, chunk, fill, fill ? kNoTrace : parts);
}

template <class PL>
int plan_pair_chunks(const PL* pl, uint32_t* chunk_of_pair) {
    if (!pl || !chunk_of_pair) return TA_ERR_ARG;
    for (uint32_t c = 0; c < (uint32_t)pl->h.chunks.size(); ++c) {
        const auto& ch = pl->h.chunks[c];
        for (uint32_t k = ch.begin; k < ch.begin + ch.count; ++k) chunk_of_pair[pl->h.order[k]] = c;
    }
    return TA_OK;
}

// Reads and clears the kernels' error word (plans whose kernels have one).
template <class PL>
int plan_check(PL* pl) {
    if (!pl) return TA_ERR_ARG;
    uint32_t* d_err = pl->err_word();
    if (!d_err) return TA_OK;
    uint32_t err = 0;
    TA_HIP(pl->ctx, hipSetDevice(pl->ctx->device));
    TA_HIP(pl->ctx, hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost));
    if (!err) return TA_OK;
    TA_HIP(pl->ctx, hipMemset(d_err, 0, 4));
    return fail(pl->ctx, TA_ERR_DEVICE, PL::err_message(err));
}

template <class PL>
int plan_annotate(PL* pl, const ta_device_io* io, const ta_annotate_io* out, void* stream) {
    if (!pl || !io || !out) return TA_ERR_ARG;
    ta_context* ctx = pl->ctx;
    if (!pl->h.want_cigar) return fail(ctx, TA_ERR_ARG, "annotate: the plan has no CIGARs");
    if (out->eqx_slots && (!out->eqx_start || !out->eqx_len))
        return fail(ctx, TA_ERR_ARG, "annotate: eqx_slots without eqx_start / eqx_len");
    if (int r = check_io(pl, io)) return r;
    if (!pl->h.n_pairs) return TA_OK;
    std::lock_guard<std::mutex> lock(ctx->mu);
    TA_HIP(ctx, hipSetDevice(ctx->device));
    ta::AnnotateArgs a{pl->h.n_pairs, pl->h.type, pl->d_qlen, pl->d_tlen, pl->d_goal_i, pl->d_goal_j, pl->d_slot_off,
                       reinterpret_cast<const uint8_t*>(io->query_bytes), io->query_off,
                       reinterpret_cast<const uint8_t*>(io->target_bytes), io->target_off, io->cigar_slots,
                       io->cigar_start, io->cigar_len, out->info, out->eqx_slots, out->eqx_start, out->eqx_len};
    TA_HIP(ctx, ta::launch_annotate(a, (hipStream_t)stream));
    return TA_OK;
}

// Banded plans (PL derives from ta::BandArrays): enqueue the certificate of the
// execution that wrote io->score, after it on the same stream.  Reads the
// plan's arrays, io->score and the sequences; writes exact[P], band_needed[P].
template <class PL>
int plan_certify(PL* pl, const ta_device_io* io, int gap_open, int gap_extend, uint8_t* exact,
                 uint32_t* band_needed, void* stream) {
    if (!pl || !io) return TA_ERR_ARG;
    ta_context* ctx = pl->ctx;
    if (!pl->h.n_pairs) return TA_OK;
    if (!exact || !band_needed) return fail(ctx, TA_ERR_ARG, "certify: null output");
    if (!io->query_off || !io->target_off || !io->score) return fail(ctx, TA_ERR_ARG, "null device pointer");
    std::lock_guard<std::mutex> lock(ctx->mu);
    TA_HIP(ctx, hipSetDevice(ctx->device));
    ta::BandCertifyArgs a{pl->h.n_pairs, pl->h.type, pl->h.match, pl->h.mismatch, gap_open, gap_extend,
                          pl->d_qlen, pl->d_tlen, pl->d_band,
                          reinterpret_cast<const uint8_t*>(io->query_bytes), io->query_off,
                          reinterpret_cast<const uint8_t*>(io->target_bytes), io->target_off, io->score,
                          exact, band_needed};
    TA_HIP(ctx, ta::launch_band_certify(a, (hipStream_t)stream));
    return TA_OK;
}

// Anchored plans (a banded family's plan built in Mode kAnchored): enqueue the
// copy of the last execution's goal cells, after it on the same stream.
template <class PL>
int plan_ends(PL* pl, uint32_t* query_end_dev, uint32_t* target_end_dev, void* stream) {
    if (!pl) return TA_ERR_ARG;
    ta_context* ctx = pl->ctx;
    if (!pl->h.n_pairs) return TA_OK;
    if (!query_end_dev || !target_end_dev) return fail(ctx, TA_ERR_ARG, "ends: null output");
    std::lock_guard<std::mutex> lock(ctx->mu);
    TA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = 4ull * pl->h.n_pairs;
    TA_HIP(ctx, hipMemcpyAsync(query_end_dev, pl->d_goal_i, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    TA_HIP(ctx, hipMemcpyAsync(target_end_dev, pl->d_goal_j, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TA_OK;
}

// Z-drop plans (an anchored plan with zdrop >= 0): enqueue the copy of the last
// execution's per-pair step counts, after it (or its fills) on the same stream.
template <class PL>
int plan_swept_steps(PL* pl, uint32_t* steps_dev, void* stream) {
    if (!pl) return TA_ERR_ARG;
    ta_context* ctx = pl->ctx;
    if (pl->h.zdrop < 0) return fail(ctx, TA_ERR_ARG, "swept_steps: not a z-drop plan");
    if (!pl->h.n_pairs) return TA_OK;
    if (!steps_dev) return fail(ctx, TA_ERR_ARG, "swept_steps: null output");
    std::lock_guard<std::mutex> lock(ctx->mu);
    TA_HIP(ctx, hipSetDevice(ctx->device));
    TA_HIP(ctx, hipMemcpyAsync(steps_dev, pl->d_swept, 4ull * pl->h.n_pairs, hipMemcpyDeviceToDevice,
                               (hipStream_t)stream));
    return TA_OK;
}

// ... and after a host batch (its stream drained, ctx->mu still held): the goal cells to host arrays.
// swept_steps: z-drop plans only (else it must be null).
template <class PL>
int batch_ends(ta_context* ctx, const PL& pl, uint32_t* query_end, uint32_t* target_end,
               uint32_t* swept_steps = nullptr) {
    const size_t bytes = 4ull * pl.h.n_pairs;
    hipStream_t s = ctx->stream;
    if (query_end) TA_HIP(ctx, hipMemcpyAsync(query_end, pl.d_goal_i, bytes, hipMemcpyDeviceToHost, s));
    if (target_end) TA_HIP(ctx, hipMemcpyAsync(target_end, pl.d_goal_j, bytes, hipMemcpyDeviceToHost, s));
    if (swept_steps && pl.h.zdrop >= 0)
        TA_HIP(ctx, hipMemcpyAsync(swept_steps, pl.d_swept, bytes, hipMemcpyDeviceToHost, s));
    TA_HIP(ctx, hipStreamSynchronize(s));
    return TA_OK;
}

}  // namespace ta_host
