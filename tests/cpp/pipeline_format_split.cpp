// tests/cpp/pipeline_format_split.cpp -- the dependency structure
// ta_pipeline_step enqueues when the slots' tracebacks are split into a walk
// and a run formatter (ta_plan_execute_walk / _format, ta_plan_format_is_split;
// bioinfo1_amd/csrc/ta_pipeline.cpp), on the CPU.  As tests/cpp/pipeline_order.cpp:
// the file is linked against stub_ta.cpp's contexts and the recording stand-ins
// below for the HIP runtime's streams and events and the plans' entry points,
// which model what the real ones promise (a stream runs its work in order, an
// event carries what its stream held when recorded, a wait adds that to the
// waiting stream, an execution on another stream than its context's previous
// one first waits for that one).  Every launch then knows the set of launches
// that must have finished before it.  Ops: 'F' fill, 'W' walk, 'R' format, 'T'
// the combined traceback, 'C' the caller's work after a step, 'U' an upload.
// main() asserts, for depth 2 and 3 over 8 steps with and without a ready
// event: the split order (walk k after fill k and walk k - 1 on the one walk
// stream and after no format younger than step k - depth; format k on the
// caller's stream after walk k; the caller after format k; fill k after format
// k - depth and nothing of the steps in between), and the combined order of
// pipeline_order.cpp where the split does not apply: two chunks, format_stream
// = 1, affine slots, plans without a formatter kernel
// (tests/test_pipeline_format_split.py runs it).
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "team_align_c.h"

struct ta_context {  // as in stub_ta.cpp
    std::string last_error;
    int device = 0;
};
struct ta_plan {
    ta_context* ctx;
    uint32_t chunks;
    bool formatter;  // its walks leave runs for a formatter kernel
};
struct ta_affine_plan {
    ta_context* ctx;
};

namespace {

using Set = std::set<int>;
struct Op {
    char kind;
    int step, chunk;
    const void* stream;
    Set before;  // every op that must have finished first
};
std::vector<Op> g_ops;
std::map<const void*, Set> g_stream;  // what a stream's next op follows
std::map<const void*, Set> g_event;   // what a recorded event carries
struct CtxLast {
    bool used = false;
    const void* stream = nullptr;
    Set held;
};
std::map<const ta_context*, CtxLast> g_ctx;
std::set<const void*> g_live_streams, g_high_streams;
int g_events = 0, g_step = 0;
uintptr_t g_next_handle = 0x1000;

int launch(char kind, int chunk, const void* stream) {
    const int id = (int)g_ops.size();
    g_ops.push_back({kind, g_step, chunk, stream, g_stream[stream]});
    g_stream[stream].insert(id);
    return id;
}

// kind 0: an execution that enqueues nothing (it still takes its place in the context's order)
int execute(ta_context* ctx, char kind, uint32_t chunk, void* stream) {
    CtxLast& c = g_ctx[ctx];
    if (c.used && c.stream != stream) g_stream[stream].insert(c.held.begin(), c.held.end());
    if (kind) launch(kind, (int)chunk, stream);
    c.held = g_stream[stream];
    c.stream = stream;
    c.used = true;
    return TA_OK;
}

int find(char kind, int step, int chunk = 0) {
    for (size_t i = 0; i < g_ops.size(); ++i)
        if (g_ops[i].kind == kind && g_ops[i].step == step && g_ops[i].chunk == chunk) return (int)i;
    return -1;
}

int count(char kind) {
    int n = 0;
    for (const Op& o : g_ops) n += o.kind == kind;
    return n;
}

Set steps_of(const Set& before, char kind) {
    Set s;
    for (int id : before)
        if (g_ops[id].kind == kind) s.insert(g_ops[id].step);
    return s;
}

Set upto(int last) {
    Set s;
    for (int k = 0; k <= last; ++k) s.insert(k);
    return s;
}

int g_fails = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            ++g_fails;                         \
            std::printf("FAIL %s: ", #cond);   \
            std::printf(__VA_ARGS__);          \
            std::printf("\n");                 \
        }                                      \
    } while (0)

void reset() {
    g_ops.clear();
    g_stream.clear();
    g_event.clear();
    g_ctx.clear();
    g_live_streams.clear();
    g_high_streams.clear();
    g_events = g_step = 0;
}

}  // namespace

extern "C" {

// ---- the HIP runtime's streams and events
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) {
    *least = 1;
    *greatest = -1;
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int flags, int priority) {
    if (flags != hipStreamNonBlocking) return hipErrorInvalidValue;  // (a blocking stream would join the null stream)
    *s = reinterpret_cast<hipStream_t>(g_next_handle += 16);
    g_live_streams.insert(*s);
    if (priority < 0) g_high_streams.insert(*s);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    g_live_streams.erase(s);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned int) {
    *e = reinterpret_cast<hipEvent_t>(g_next_handle += 16);
    ++g_events;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) {
    --g_events;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    g_event[e] = g_stream[s];
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) {
    const Set& held = g_event[e];
    g_stream[s].insert(held.begin(), held.end());
    return hipSuccess;
}

// ---- the plans' side of the C ABI that ta_pipeline.cpp calls
ta_context* ta_plan_context(const ta_plan* p) { return p ? p->ctx : nullptr; }
uint32_t ta_plan_chunks(const ta_plan* p) { return p->chunks; }
int ta_context_device(const ta_context* c) { return c->device; }
void ta_context_set_error(ta_context* c, const char* m) { c->last_error = m; }
int ta_plan_execute_fill(ta_plan* p, const ta_device_io*, void* s, uint32_t c) { return execute(p->ctx, 'F', c, s); }
int ta_plan_execute_traceback(ta_plan* p, const ta_device_io*, void* s, uint32_t c) { return execute(p->ctx, 'T', c, s); }
// (a plan without a formatter kernel: _walk is the whole traceback, _format enqueues nothing)
int ta_plan_execute_walk(ta_plan* p, const ta_device_io*, void* s, uint32_t c) {
    return execute(p->ctx, p->formatter ? 'W' : 'T', c, s);
}
int ta_plan_execute_format(ta_plan* p, const ta_device_io*, void* s, uint32_t c) {
    return execute(p->ctx, p->formatter ? 'R' : 0, c, s);
}
int ta_plan_format_is_split(const ta_plan* p, uint32_t c) { return p && c < p->chunks && p->formatter ? 1 : 0; }
ta_context* ta_affine_plan_context(const ta_affine_plan* p) { return p ? p->ctx : nullptr; }
uint32_t ta_affine_plan_chunks(const ta_affine_plan*) { return 1; }
int ta_affine_plan_execute_fill(ta_affine_plan* p, const ta_device_io*, void* s, uint32_t c) { return execute(p->ctx, 'F', c, s); }
int ta_affine_plan_execute_traceback(ta_affine_plan* p, const ta_device_io*, void* s, uint32_t c) { return execute(p->ctx, 'T', c, s); }

}  // extern "C"

namespace {

void* const kCaller = reinterpret_cast<void*>(0x10);
void* const kCopy = reinterpret_cast<void*>(0x20);
const hipEvent_t kReady = reinterpret_cast<hipEvent_t>(0x30);

struct Slots {
    std::vector<ta_context*> ctxs;
    std::vector<ta_plan> plans;
    std::vector<ta_plan*> slots;
    std::vector<ta_affine_plan> aplans;
    std::vector<ta_affine_plan*> aslots;
    Slots(uint32_t depth, uint32_t chunks, bool formatter) : ctxs(depth), plans(depth), slots(depth), aplans(depth), aslots(depth) {
        for (uint32_t s = 0; s < depth; ++s) {
            ta_context_create(0, &ctxs[s]);
            plans[s] = {ctxs[s], chunks, formatter};
            slots[s] = &plans[s];
            aplans[s] = {ctxs[s]};
            aslots[s] = &aplans[s];
        }
    }
    ~Slots() {
        for (ta_context* c : ctxs) ta_context_destroy(c);
    }
};

void run_steps(ta_pipeline* pipe, uint32_t depth, int steps, bool with_ready) {
    const ta_device_io io{};
    for (g_step = 0; g_step < steps; ++g_step) {
        if (with_ready) {
            launch('U', 0, kCopy);
            hipEventRecord(kReady, static_cast<hipStream_t>(kCopy));
        }
        uint32_t slot = ~0u;
        CHECK(ta_pipeline_step(pipe, &io, with_ready ? kReady : nullptr, kCaller, &slot) == TA_OK, "step %d", g_step);
        CHECK(slot == (uint32_t)g_step % depth, "step %d on slot %u", g_step, slot);
        launch('C', 0, kCaller);  // what the caller queues after the step (a snapshot of its results)
    }
    CHECK(g_live_streams.size() == depth + 1 && g_high_streams.size() == 1, "%zu streams, %zu of high priority",
          g_live_streams.size(), g_high_streams.size());
}

// The split order.  opt: null (ta_pipeline_create), or the options of ta_pipeline_create_ex.
void run_split(uint32_t depth, int steps, bool with_ready, const ta_pipeline_options* opt, const char* what) {
    reset();
    Slots S(depth, 1, true);
    ta_pipeline* pipe = nullptr;
    const int r = opt ? ta_pipeline_create_ex(S.slots.data(), depth, opt, &pipe) : ta_pipeline_create(S.slots.data(), depth, &pipe);
    CHECK(r == TA_OK && pipe, "%s depth %u", what, depth);
    if (!pipe) return;
    CHECK(ta_pipeline_format_split(pipe) == 1, "%s depth %u", what, depth);
    CHECK(g_live_streams.empty() && g_events == 0, "streams are created at the first step");
    run_steps(pipe, depth, steps, with_ready);
    CHECK(count('T') == 0 && count('W') == steps && count('R') == steps, "%s: %d T, %d W, %d R", what, count('T'), count('W'),
          count('R'));
    const int d = (int)depth;
    const void* walk_stream = g_ops[find('W', 0)].stream;
    CHECK(g_high_streams.count(walk_stream) == 1, "%s: the walk stream is the one of high priority", what);
    for (int k = 0; k < steps; ++k) {
        const int f = find('F', k), w = find('W', k), r = find('R', k), c = find('C', k);
        CHECK(f >= 0 && w >= 0 && r >= 0 && c >= 0, "%s step %d", what, k);
        if (f < 0 || w < 0 || r < 0 || c < 0) continue;
        const Op &fill = g_ops[f], &walk = g_ops[w], &fmt = g_ops[r], &call = g_ops[c];
        // walk k: on the one walk stream, after its fill and the walk before it; of the formats only
        // those its fill followed (steps 0 .. k - depth) -- not R_{k-1}, which runs beside it
        CHECK(walk.stream == walk_stream && walk.stream != fill.stream && walk.stream != kCaller, "%s walk %d", what, k);
        CHECK(walk.before.count(f) == 1, "%s walk %d follows its fill", what, k);
        if (k) CHECK(walk.before.count(find('W', k - 1)) == 1, "%s walk %d follows walk %d", what, k, k - 1);
        CHECK(steps_of(walk.before, 'R') == upto(k - d), "%s walk %d depth %d", what, k, d);
        CHECK(steps_of(walk.before, 'C') == upto(k - d), "%s walk %d depth %d", what, k, d);
        if (k) CHECK(walk.before.count(find('R', k - 1)) == 0, "%s walk %d does not follow format %d", what, k, k - 1);
        // format k: on the caller's stream, after walk k (and so after format k - 1, stream order)
        CHECK(fmt.stream == kCaller, "%s format %d on the caller's stream", what, k);
        CHECK(fmt.before.count(w) == 1, "%s format %d follows walk %d", what, k, k);
        CHECK(steps_of(fmt.before, 'W') == upto(k), "%s format %d", what, k);
        // the caller's work after the step follows the format
        CHECK(call.before.count(r) == 1, "%s caller after format %d", what, k);
        // fill k follows slot k % depth's previous use -- format k - depth included -- and nothing
        // of steps k - depth + 1 .. k - 1
        for (char kind : {'F', 'W', 'R', 'C'})
            CHECK(steps_of(fill.before, kind) == upto(k - d), "%s fill %d depth %d kind %c", what, k, d, kind);
        if (k >= d) CHECK(fill.before.count(find('R', k - d)) == 1, "%s fill %d follows format %d", what, k, k - d);
        if (with_ready) CHECK(steps_of(fill.before, 'U').count(k) == 1, "%s fill %d follows its upload", what, k);
        CHECK(g_high_streams.count(fill.stream) == 0 && fill.stream != kCaller, "%s fill %d", what, k);
        for (int j = 0; j < k; ++j)  // a fill stream per slot
            CHECK((g_ops[find('F', j)].stream == fill.stream) == (j % d == k % d), "%s fill streams of steps %d, %d", what, j, k);
    }
    ta_pipeline_destroy(pipe);
    CHECK(g_live_streams.empty() && g_events == 0, "destroy: %zu streams, %d events left", g_live_streams.size(), g_events);
}

// The combined order (what pipeline_order.cpp asserts): 'T' on the walk stream, no 'W', no 'R'.
void check_combined(uint32_t depth, uint32_t chunks, int steps, bool with_ready, const char* what) {
    CHECK(count('W') == 0 && count('R') == 0 && count('T') == steps * (int)chunks, "%s: %d W, %d R, %d T", what, count('W'),
          count('R'), count('T'));
    const int d = (int)depth, last_chunk = (int)chunks - 1;
    if (find('T', 0, 0) < 0) return;
    const void* walk_stream = g_ops[find('T', 0, 0)].stream;
    CHECK(g_high_streams.count(walk_stream) == 1, "%s: the walk stream is the one of high priority", what);
    for (int k = 0; k < steps; ++k) {
        const int f0 = find('F', k, 0), c = find('C', k);
        CHECK(f0 >= 0 && c >= 0, "%s step %d", what, k);
        if (f0 < 0 || c < 0) continue;
        const Op& fill = g_ops[f0];
        for (char kind : {'F', 'T', 'C'})
            CHECK(steps_of(fill.before, kind) == upto(k - d), "%s fill %d depth %d kind %c", what, k, d, kind);
        if (k >= d) CHECK(fill.before.count(find('T', k - d, last_chunk)) == 1, "%s fill %d", what, k);
        if (with_ready) CHECK(steps_of(fill.before, 'U').count(k) == 1, "%s fill %d follows its upload", what, k);
        for (int ch = 0; ch < (int)chunks; ++ch) {
            const int f = find('F', k, ch), t = find('T', k, ch);
            CHECK(f >= 0 && t >= 0 && g_ops[t].before.count(f) == 1, "%s walk %d.%d follows its fill", what, k, ch);
            if (f < 0 || t < 0) continue;
            CHECK(g_ops[f].stream == fill.stream && g_ops[t].stream == walk_stream, "%s step %d.%d", what, k, ch);
            if (ch) CHECK(g_ops[f].before.count(find('T', k, ch - 1)) == 1, "%s fill %d.%d", what, k, ch);
        }
        for (int j = 0; j < k; ++j)
            CHECK((g_ops[find('F', j, 0)].stream == fill.stream) == (j % d == k % d), "%s fill streams of steps %d, %d", what, j, k);
        CHECK(g_ops[c].before.count(find('T', k, last_chunk)) == 1, "%s caller after step %d", what, k);
    }
}

enum Combined { kTwoChunks, kFormatStream1, kAffine, kNoFormatter };

void run_combined(Combined which, uint32_t depth, int steps, bool with_ready) {
    reset();
    const char* what = which == kTwoChunks ? "two chunks" : which == kFormatStream1 ? "format_stream 1" : which == kAffine ? "affine" : "no formatter";
    const uint32_t chunks = which == kTwoChunks ? 2 : 1;
    Slots S(depth, chunks, which != kNoFormatter);
    ta_pipeline* pipe = nullptr;
    const ta_pipeline_options keep = {sizeof(ta_pipeline_options), 0, 1}, defaults = {sizeof(ta_pipeline_options), 0, 0};
    int r;
    if (which == kAffine)
        r = ta_pipeline_create_affine_ex(S.aslots.data(), depth, &defaults, &pipe);
    else
        r = ta_pipeline_create_ex(S.slots.data(), depth, which == kFormatStream1 ? &keep : &defaults, &pipe);
    CHECK(r == TA_OK && pipe, "%s depth %u", what, depth);
    if (!pipe) return;
    CHECK(ta_pipeline_format_split(pipe) == 0, "%s depth %u", what, depth);
    run_steps(pipe, depth, steps, with_ready);
    check_combined(depth, chunks, steps, with_ready, what);
    ta_pipeline_destroy(pipe);
    CHECK(g_live_streams.empty() && g_events == 0, "destroy: %zu streams, %d events left", g_live_streams.size(), g_events);
}

void run_options() {
    reset();
    Slots S(3, 1, true);
    ta_pipeline* pipe = reinterpret_cast<ta_pipeline*>(1);
    const ta_pipeline_options bad = {sizeof(ta_pipeline_options), 0, 2};
    CHECK(ta_pipeline_create_ex(S.slots.data(), 3, &bad, &pipe) == TA_ERR_ARG && !pipe, "format_stream 2");
    CHECK(std::string(ta_last_error(S.ctxs[0])).find("format_stream") != std::string::npos, "%s", ta_last_error(S.ctxs[0]));
    CHECK(ta_pipeline_format_split(nullptr) == 0, "null pipeline");
    CHECK(g_ops.empty() && g_live_streams.empty() && g_events == 0, "argument errors enqueue nothing");
}

}  // namespace

int main() {
    const ta_pipeline_options defaults = {sizeof(ta_pipeline_options), 0, 0};
    // a caller compiled before format_stream existed: the field lies beyond its `size` and reads as 0
    const ta_pipeline_options older = {(uint32_t)offsetof(ta_pipeline_options, format_stream), 1, 1};
    for (uint32_t depth : {2u, 3u})
        for (bool ready : {false, true}) {
            run_split(depth, 8, ready, nullptr, "ta_pipeline_create");
            run_split(depth, 8, ready, &defaults, "format_stream 0");
            run_split(depth, 8, ready, &older, "format_stream beyond size");
            for (Combined which : {kTwoChunks, kFormatStream1, kAffine, kNoFormatter}) run_combined(which, depth, 8, ready);
        }
    run_options();
    std::printf("pipeline format split: fails %d\n", g_fails);
    return g_fails ? 1 : 0;
}
