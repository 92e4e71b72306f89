// bioinfo1_amd/csrc/ta_pipeline.cpp -- ta_pipeline_* of include/team_align_c.h:
// the dependency structure of batches aligned back to back.
//
// Host C++ over the C ABI and the HIP runtime's streams and events only: no
// kernel, no device-side polling.  What it relies on from the plans' drivers:
// an execution on another stream than its context's previous one first waits
// for that one (ta_context.h stream_enter / stream_leave), so a slot's
// traceback on the walk stream follows its fill on the slot's fill stream, and
// a chunk's fill the traceback of the chunk before it (one workspace).
//
// Streams: ONE FILL STREAM PER SLOT.  Fill k+2 (slot s) waits for slot s's
// done event only -- walk k and what the caller queued after it -- never for
// fill k+1, which runs on another slot's stream: when fill k+1's last blocks
// run alone on a mostly idle chip (they could not become resident while walk
// k held registers), fill k+2's blocks take the free CUs.
//
// WALK STREAMS: ta_pipeline_create keeps one, so walks run back to back (with
// their formatters between them in the combined order, below).  With
// walk_streams = w (ta_pipeline_create_ex) step k's
// traceback goes to walk stream k % w -- the step index, not the slot's, so
// consecutive steps alternate whatever the depth -- and walk k+1 may start
// beside walk k's tail and its formatter.  Nothing else changes: a walk still
// follows its own fill through the slot's context, the caller's stream waits
// for every step's walk in step order, and a fill for its slot's done event.
//
// THE RUN FORMATTER OFF THE WALK STREAM.  With one walk stream the step period
// is that stream's chain: walk, formatter, the launch gap to the next walk.
// Walk k+1 needs its own fill and the walk stream, nothing the formatter of
// step k writes; only the caller's stream and the slot's next fill need that.
// So where a slot's traceback is a walk kernel and a formatter kernel
// (ta_plan_format_is_split: checkpoint and band walks) and the plan has one
// chunk, a step enqueues the walk alone on the walk stream
// (ta_plan_execute_walk), records walked[i] after it, lets the caller's stream
// wait for that and enqueues the formatter on the CALLER'S stream
// (ta_plan_execute_format): formatter k runs beside walk k+1, what the caller
// enqueues afterwards follows it by stream order, and done[i], recorded on the
// caller's stream at the next step, makes the slot's next fill follow it too.
// No further stream, so no further hardware queue.  Plans of several chunks
// (one workspace: a chunk's fill follows the formatter before it anyway),
// affine slots and format_stream = 1 keep the combined traceback call.
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/team_align_c.h"
#define TA_PIPELINE_WEAK_REFS 1  // ta_plan_execute_walk / _format / _format_is_split may be absent (stand-in builds)
#include "ta_pipeline_internal.h"

namespace {

// The plan family's entry points behind a slot (linear-gap or affine plans).
struct Ops {
    ta_context* (*context)(const void*);
    uint32_t (*chunks)(const void*);
    int (*fill)(void*, const ta_device_io*, void*, uint32_t);
    int (*walk)(void*, const ta_device_io*, void*, uint32_t);  // the whole traceback: walk and formatter
    // the traceback in two executions, where the library has them and the plan's traceback is
    // two kernels (split); null: the family has only the combined call
    bool (*split)(const void*);
    int (*walk_only)(void*, const ta_device_io*, void*, uint32_t);
    int (*format)(void*, const ta_device_io*, void*, uint32_t);
};

const Ops kLinear = {
    [](const void* p) { return ta_plan_context(static_cast<const ta_plan*>(p)); },
    [](const void* p) { return ta_plan_chunks(static_cast<const ta_plan*>(p)); },
    [](void* p, const ta_device_io* io, void* s, uint32_t c) {
        return ta_plan_execute_fill(static_cast<ta_plan*>(p), io, s, c);
    },
    [](void* p, const ta_device_io* io, void* s, uint32_t c) {
        return ta_plan_execute_traceback(static_cast<ta_plan*>(p), io, s, c);
    },
    // (weak references, ta_pipeline_internal.h: absent in a build against stand-ins that lack them)
    [](const void* p) {
        const ta_plan* pl = static_cast<const ta_plan*>(p);
        return ta_plan_execute_walk && ta_plan_execute_format && ta_plan_format_is_split && ta_plan_chunks(pl) == 1 &&
               ta_plan_format_is_split(pl, 0) != 0;
    },
    [](void* p, const ta_device_io* io, void* s, uint32_t c) {
        return ta_plan_execute_walk(static_cast<ta_plan*>(p), io, s, c);
    },
    [](void* p, const ta_device_io* io, void* s, uint32_t c) {
        return ta_plan_execute_format(static_cast<ta_plan*>(p), io, s, c);
    },
};

const Ops kAffine = {
    [](const void* p) { return ta_affine_plan_context(static_cast<const ta_affine_plan*>(p)); },
    [](const void* p) { return ta_affine_plan_chunks(static_cast<const ta_affine_plan*>(p)); },
    [](void* p, const ta_device_io* io, void* s, uint32_t c) {
        return ta_affine_plan_execute_fill(static_cast<ta_affine_plan*>(p), io, s, c);
    },
    [](void* p, const ta_device_io* io, void* s, uint32_t c) {
        return ta_affine_plan_execute_traceback(static_cast<ta_affine_plan*>(p), io, s, c);
    },
    nullptr,
    nullptr,
    nullptr,
};

int fail(ta_context* ctx, int code, const std::string& msg) {
    ta_context_set_error(ctx, msg.c_str());
    return code;
}

#define TP_HIP(ctx, expr)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((ctx), TA_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

}  // namespace

struct ta_pipeline {
    const Ops* ops = nullptr;
    int device = 0;
    std::vector<void*> slots;
    std::vector<ta_context*> ctxs;
    // created at the first step (each stream takes one of the process's few hardware queues)
    std::vector<hipStream_t> fill;  // one per slot
    std::vector<hipStream_t> walk;  // step k's traceback on walk[k % size]; high priority: hardware queues beside the fills'
    // done[s]: recorded on the caller's stream at the step after slot s's, so it covers
    // slot s's traceback (its formatter on the caller's stream included) and what the caller
    // queued after it; walked[s]: slot s's traceback (split: its walk);
    // start: the caller's stream at the first step (a slot's first fill follows it)
    std::vector<hipEvent_t> done, walked;
    hipEvent_t start = nullptr;
    std::vector<bool> used;
    bool split = false;  // every step: the walk on the walk stream, the formatter on the caller's
    uint64_t k = 0;
    int last = -1;
};

namespace {

// GPU_MAX_HW_QUEUES as the HIP runtime reads it: unset (or not a number) is its default, 4.
uint32_t hw_queues() {
    const char* v = std::getenv("GPU_MAX_HW_QUEUES");
    if (!v || !*v) return 4;
    char* end = nullptr;
    const long n = std::strtol(v, &end, 10);
    return (*end || n <= 0) ? 4u : (uint32_t)n;
}

// walk_streams 0: the library's default where every stream of the pipeline and the caller's
// get a hardware queue of their own (streams sharing a queue run one after the other, and a
// walk behind a fill on its queue would be worse than the one walk stream); else one.
uint32_t resolve_walk_streams(uint32_t asked, uint32_t depth) {
    if (asked) return asked;
    const uint32_t w = TA_PIPELINE_WALK_STREAMS_DEFAULT < depth ? TA_PIPELINE_WALK_STREAMS_DEFAULT : depth;
    return hw_queues() >= depth + w + 1 ? w : 1;
}

int create(const Ops& ops, void* const* slots, uint32_t depth, const ta_pipeline_options* opt, ta_pipeline** out) {
    if (!out) return TA_ERR_ARG;
    *out = nullptr;
    if (!slots || !depth || !slots[0]) return TA_ERR_ARG;
    ta_context* c0 = ops.context(slots[0]);
    if (!c0) return TA_ERR_ARG;
    if (depth < 2) return fail(c0, TA_ERR_ARG, "ta_pipeline_create: depth must be at least 2");
    for (uint32_t a = 0; a < depth; ++a) {
        ta_context* ca = slots[a] ? ops.context(slots[a]) : nullptr;
        if (!ca) return fail(c0, TA_ERR_ARG, "ta_pipeline_create: null slot");
        if (ta_context_device(ca) != ta_context_device(c0))
            return fail(c0, TA_ERR_ARG, "ta_pipeline_create: slots on different devices");
        for (uint32_t b = 0; b < a; ++b)
            if (ops.context(slots[b]) == ca)
                return fail(c0, TA_ERR_ARG, "ta_pipeline_create: two slots share a context (each needs its own workspace)");
    }
    // (fields beyond the caller's `size` read as 0; no options: ta_pipeline_create's one walk stream)
    uint32_t w = 1, format_stream = 0;
    if (opt) {
        const bool has = opt->size >= offsetof(ta_pipeline_options, walk_streams) + sizeof(opt->walk_streams);
        w = resolve_walk_streams(has ? opt->walk_streams : 0, depth);
        if (opt->size >= offsetof(ta_pipeline_options, format_stream) + sizeof(opt->format_stream))
            format_stream = opt->format_stream;
    }
    if (format_stream > 1)
        return fail(c0, TA_ERR_ARG, "ta_pipeline_create: format_stream must be 0 or 1 (" + std::to_string(format_stream) + ")");
    if (w > depth)
        return fail(c0, TA_ERR_ARG, "ta_pipeline_create: walk_streams exceeds depth (" + std::to_string(w) + " > " +
                                        std::to_string(depth) + ")");
    auto* p = new ta_pipeline();
    p->ops = &ops;
    p->device = ta_context_device(c0);
    p->slots.assign(slots, slots + depth);
    for (uint32_t a = 0; a < depth; ++a) p->ctxs.push_back(ops.context(slots[a]));
    p->fill.assign(depth, nullptr);
    p->walk.assign(w, nullptr);
    p->done.assign(depth, nullptr);
    p->walked.assign(depth, nullptr);
    p->used.assign(depth, false);
    p->split = format_stream == 0 && ops.split;
    for (uint32_t a = 0; p->split && a < depth; ++a) p->split = ops.split(slots[a]);
    *out = p;
    return TA_OK;
}

int lazy_stream(ta_context* ctx, hipStream_t& s, int priority) {
    if (s) return TA_OK;
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority) != hipSuccess) {
        s = nullptr;
        return fail(ctx, TA_ERR_DEVICE, "ta_pipeline_step: hipStreamCreateWithPriority failed");
    }
    return TA_OK;
}

int lazy_event(ta_context* ctx, hipEvent_t& e) {
    if (e) return TA_OK;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
        e = nullptr;
        return fail(ctx, TA_ERR_DEVICE, "ta_pipeline_step: hipEventCreateWithFlags failed");
    }
    return TA_OK;
}

}  // namespace

extern "C" {

int ta_pipeline_create(ta_plan* const* slots, uint32_t depth, ta_pipeline** out) {
    return create(kLinear, reinterpret_cast<void* const*>(slots), depth, nullptr, out);
}

int ta_pipeline_create_ex(ta_plan* const* slots, uint32_t depth, const ta_pipeline_options* options,
                          ta_pipeline** out) {
    const ta_pipeline_options defaults = {sizeof(ta_pipeline_options), 0, 0};
    return create(kLinear, reinterpret_cast<void* const*>(slots), depth, options ? options : &defaults, out);
}

int ta_pipeline_create_affine(ta_affine_plan* const* slots, uint32_t depth, ta_pipeline** out) {
    return create(kAffine, reinterpret_cast<void* const*>(slots), depth, nullptr, out);
}

int ta_pipeline_create_affine_ex(ta_affine_plan* const* slots, uint32_t depth, const ta_pipeline_options* options,
                                 ta_pipeline** out) {
    const ta_pipeline_options defaults = {sizeof(ta_pipeline_options), 0, 0};
    return create(kAffine, reinterpret_cast<void* const*>(slots), depth, options ? options : &defaults, out);
}

uint32_t ta_pipeline_walk_streams(const ta_pipeline* p) { return p ? (uint32_t)p->walk.size() : 0; }
int ta_pipeline_format_split(const ta_pipeline* p) { return p && p->split ? 1 : 0; }

int ta_pipeline_step(ta_pipeline* p, const ta_device_io* io, void* ready_event, void* caller_stream,
                     uint32_t* slot_out) {
    if (!p) return TA_ERR_ARG;
    const uint32_t depth = (uint32_t)p->slots.size();
    const uint32_t i = (uint32_t)(p->k % depth);
    ta_context* ctx = p->ctxs[i];
    if (!io) return fail(ctx, TA_ERR_ARG, "ta_pipeline_step: null io");
    hipStream_t cur = static_cast<hipStream_t>(caller_stream);
    TP_HIP(ctx, hipSetDevice(p->device));
    if (!p->walk.back()) {  // every walk stream at the first step
        int least = 0, greatest = 0;
        TP_HIP(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        for (hipStream_t& s : p->walk)
            if (int r = lazy_stream(ctx, s, greatest)) return r;
    }
    hipStream_t walk = p->walk[p->k % p->walk.size()];
    if (int r = lazy_stream(ctx, p->fill[i], 0)) return r;
    if (int r = lazy_event(ctx, p->done[i])) return r;
    if (int r = lazy_event(ctx, p->walked[i])) return r;
    if (!p->start) {
        if (int r = lazy_event(ctx, p->start)) return r;
        TP_HIP(ctx, hipEventRecord(p->start, cur));
    }
    // the previous slot's traceback and what the caller queued after it
    if (p->last >= 0) TP_HIP(ctx, hipEventRecord(p->done[p->last], cur));
    if (slot_out) *slot_out = i;
    void* plan = p->slots[i];
    TP_HIP(ctx, hipStreamWaitEvent(p->fill[i], p->used[i] ? p->done[i] : p->start, 0));
    if (ready_event) TP_HIP(ctx, hipStreamWaitEvent(p->fill[i], static_cast<hipEvent_t>(ready_event), 0));
    if (p->split) {  // (one chunk) the walk stream's chain is walk -> walk: the formatter runs beside the next walk
        if (int r = p->ops->fill(plan, io, p->fill[i], 0)) return r;
        if (int r = p->ops->walk_only(plan, io, walk, 0)) return r;  // (after the fill: the slot's context orders them)
        TP_HIP(ctx, hipEventRecord(p->walked[i], walk));
        TP_HIP(ctx, hipStreamWaitEvent(cur, p->walked[i], 0));
        if (int r = p->ops->format(plan, io, cur, 0)) return r;
    } else {
        const uint32_t chunks = p->ops->chunks(plan);
        for (uint32_t c = 0; c < chunks; ++c) {
            if (int r = p->ops->fill(plan, io, p->fill[i], c)) return r;
            if (int r = p->ops->walk(plan, io, walk, c)) return r;  // (after the fill: the slot's context orders them)
        }
        TP_HIP(ctx, hipEventRecord(p->walked[i], walk));
        TP_HIP(ctx, hipStreamWaitEvent(cur, p->walked[i], 0));
    }
    p->used[i] = true;
    p->last = (int)i;
    ++p->k;
    return TA_OK;
}

void ta_pipeline_destroy(ta_pipeline* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    // (destroying a stream or an event with work pending is deferred by the runtime until it is done)
    for (hipStream_t s : p->fill)
        if (s) (void)hipStreamDestroy(s);
    for (hipStream_t s : p->walk)
        if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : p->done)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->walked)
        if (e) (void)hipEventDestroy(e);
    if (p->start) (void)hipEventDestroy(p->start);
    delete p;
}

}  // extern "C"
