// tests/cpp/pipeline_order.cpp -- the dependency structure ta_pipeline_step
// enqueues (bioinfo1_amd/csrc/ta_pipeline.cpp), on the CPU: the file is linked
// against stub_ta.cpp's contexts and against the recording stand-ins below for
// the HIP runtime's streams and events and for the plans' fill / traceback
// entry points.  The stand-ins model what the real ones promise: a stream runs
// its work in order, an event carries what its stream held when it was
// recorded, a wait adds that to the waiting stream, and an execution on
// another stream than its context's previous one first waits for that one
// (ta_context.h stream_enter / stream_leave).  Every launch then knows the set
// of launches that must have finished before it, and main() asserts that set
// for depth 2 and 3 over 8 steps (tests/test_pipeline_order.py runs it).
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

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
};
struct ta_affine_plan {
    ta_context* ctx;
};

namespace {

using Set = std::set<int>;
struct Op {
    char kind;  // 'F' fill, 'T' traceback, 'C' the caller's own work, 'U' an upload
    int step, chunk;
    const void* stream;
    Set before;  // every op that must have finished first
};
std::vector<Op> g_ops;
std::map<const void*, Set> g_stream;             // what a stream's next op follows
std::map<const void*, Set> g_event;              // what a recorded event carries
struct CtxLast {
    bool used = false;
    const void* stream = nullptr;
    Set held;
};
std::map<const ta_context*, CtxLast> g_ctx;
int g_streams = 0, g_events = 0, g_high_priority = 0, g_step = 0;
uintptr_t g_next_handle = 0x1000;

int launch(char kind, int chunk, const void* stream) {
    const int id = (int)g_ops.size();
    g_ops.push_back({kind, g_step, chunk, stream, g_stream[stream]});
    g_stream[stream].insert(id);
    return id;
}

int execute(ta_context* ctx, char kind, uint32_t chunk, void* stream) {
    CtxLast& c = g_ctx[ctx];
    if (c.used && c.stream != stream) g_stream[stream].insert(c.held.begin(), c.held.end());
    launch(kind, (int)chunk, stream);
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
    g_streams = g_events = g_high_priority = g_step = 0;
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
    ++g_streams;
    if (priority < 0) ++g_high_priority;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) {
    --g_streams;
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
ta_context* ta_affine_plan_context(const ta_affine_plan* p) { return p ? p->ctx : nullptr; }
uint32_t ta_affine_plan_chunks(const ta_affine_plan*) { return 1; }
int ta_affine_plan_execute_fill(ta_affine_plan* p, const ta_device_io*, void* s, uint32_t c) { return execute(p->ctx, 'F', c, s); }
int ta_affine_plan_execute_traceback(ta_affine_plan* p, const ta_device_io*, void* s, uint32_t c) { return execute(p->ctx, 'T', c, s); }

}  // extern "C"

namespace {

// depth slots of `chunks` chunks over `steps` steps; with_ready: every step's
// inputs are "uploaded" on a copy stream whose event is passed as ready
void run_case(uint32_t depth, uint32_t chunks, int steps, bool with_ready) {
    reset();
    std::vector<ta_context*> ctxs(depth);
    std::vector<ta_plan> plans(depth);
    std::vector<ta_plan*> slots(depth);
    for (uint32_t s = 0; s < depth; ++s) {
        ta_context_create(0, &ctxs[s]);
        plans[s] = {ctxs[s], chunks};
        slots[s] = &plans[s];
    }
    ta_pipeline* pipe = nullptr;
    CHECK(ta_pipeline_create(slots.data(), depth, &pipe) == TA_OK && pipe, "depth %u", depth);
    CHECK(g_streams == 0 && g_events == 0, "streams are created at the first step");
    const ta_device_io io{};
    void* caller = reinterpret_cast<void*>(0x10);
    void* copy = reinterpret_cast<void*>(0x20);
    hipEvent_t ready = reinterpret_cast<hipEvent_t>(0x30);
    for (g_step = 0; g_step < steps; ++g_step) {
        if (with_ready) {
            launch('U', 0, copy);
            hipEventRecord(ready, static_cast<hipStream_t>(copy));
        }
        uint32_t slot = ~0u;
        CHECK(ta_pipeline_step(pipe, &io, with_ready ? ready : nullptr, caller, &slot) == TA_OK, "step %d", g_step);
        CHECK(slot == (uint32_t)g_step % depth, "step %d on slot %u", g_step, slot);
        launch('C', 0, caller);  // what the caller queues after the step (a snapshot of its results)
    }
    CHECK(g_streams == (int)depth + 1 && g_high_priority == 1, "%d streams, %d of high priority", g_streams, g_high_priority);
    const int d = (int)depth, last_chunk = (int)chunks - 1;
    for (int k = 0; k < steps; ++k) {
        const int f0 = find('F', k, 0), c = find('C', k);
        CHECK(f0 >= 0 && c >= 0, "step %d", k);
        const Op& fill = g_ops[f0];
        // fill k follows slot k % depth's previous use -- its fills, its tracebacks and what the
        // caller queued after them -- and through that everything older; nothing of steps
        // k - depth + 1 .. k - 1 (the other slots' fills and walks still in flight)
        CHECK(steps_of(fill.before, 'F') == upto(k - d), "fill %d depth %d", k, d);
        CHECK(steps_of(fill.before, 'T') == upto(k - d), "fill %d depth %d", k, d);
        CHECK(steps_of(fill.before, 'C') == upto(k - d), "fill %d depth %d", k, d);
        if (k >= d) CHECK(fill.before.count(find('T', k - d, last_chunk)) == 1, "fill %d", k);
        if (with_ready) CHECK(steps_of(fill.before, 'U').count(k) == 1, "fill %d follows its upload", k);
        for (int ch = 0; ch < (int)chunks; ++ch) {
            const int f = find('F', k, ch), t = find('T', k, ch);
            CHECK(f >= 0 && t >= 0 && g_ops[t].before.count(f) == 1, "walk %d.%d follows its fill", k, ch);
            CHECK(g_ops[f].stream != g_ops[t].stream, "step %d: fill and walk streams", k);
            CHECK(g_ops[f].stream == fill.stream && g_ops[t].stream == g_ops[find('T', 0, 0)].stream, "step %d", k);
            // one workspace: a chunk's fill follows the walk of the chunk before it
            if (ch) CHECK(g_ops[f].before.count(find('T', k, ch - 1)) == 1, "fill %d.%d", k, ch);
        }
        // a fill stream per slot
        for (int j = 0; j < k; ++j)
            CHECK((g_ops[find('F', j, 0)].stream == fill.stream) == (j % d == k % d), "fill streams of steps %d, %d", j, k);
        // the caller's stream waited for walk k
        CHECK(g_ops[c].before.count(find('T', k, last_chunk)) == 1, "caller after step %d", k);
    }
    ta_pipeline_destroy(pipe);
    CHECK(g_streams == 0 && g_events == 0, "destroy: %d streams, %d events left", g_streams, g_events);
    for (ta_context* c : ctxs) ta_context_destroy(c);
}

void run_errors() {
    reset();
    ta_context *a = nullptr, *b = nullptr, *other = nullptr;
    ta_context_create(0, &a);
    ta_context_create(0, &b);
    ta_context_create(1, &other);
    ta_plan pa{a, 1}, pa2{a, 1}, pb{b, 1}, po{other, 1};
    ta_pipeline* pipe = reinterpret_cast<ta_pipeline*>(1);
    ta_plan* one[] = {&pa};
    CHECK(ta_pipeline_create(one, 1, &pipe) == TA_ERR_ARG && !pipe, "depth 1");
    CHECK(std::string(ta_last_error(a)).find("depth") != std::string::npos, "%s", ta_last_error(a));
    ta_plan* shared[] = {&pa, &pb, &pa2};
    CHECK(ta_pipeline_create(shared, 3, &pipe) == TA_ERR_ARG && !pipe, "shared context");
    CHECK(std::string(ta_last_error(a)).find("context") != std::string::npos, "%s", ta_last_error(a));
    ta_plan* mixed[] = {&pa, &po};
    CHECK(ta_pipeline_create(mixed, 2, &pipe) == TA_ERR_ARG && !pipe, "mixed devices");
    CHECK(std::string(ta_last_error(a)).find("device") != std::string::npos, "%s", ta_last_error(a));
    ta_plan* null_slot[] = {&pa, nullptr};
    CHECK(ta_pipeline_create(null_slot, 2, &pipe) == TA_ERR_ARG && !pipe, "null slot");
    CHECK(ta_pipeline_create(nullptr, 2, &pipe) == TA_ERR_ARG, "null slots");
    ta_plan* good[] = {&pa, &pb};
    CHECK(ta_pipeline_create(good, 2, &pipe) == TA_OK, "two contexts");
    CHECK(ta_pipeline_step(pipe, nullptr, nullptr, nullptr, nullptr) == TA_ERR_ARG, "null io");
    CHECK(ta_pipeline_step(nullptr, nullptr, nullptr, nullptr, nullptr) == TA_ERR_ARG, "null pipeline");
    CHECK(g_ops.empty() && g_streams == 0 && g_events == 0, "argument errors enqueue nothing");
    ta_pipeline_destroy(pipe);
    ta_pipeline_destroy(nullptr);
    for (ta_context* c : {a, b, other}) ta_context_destroy(c);
}

}  // namespace

int main() {
    for (uint32_t depth : {2u, 3u})
        for (uint32_t chunks : {1u, 2u})
            for (bool ready : {false, true}) run_case(depth, chunks, 8, ready);
    run_errors();
    std::printf("pipeline order: fails %d\n", g_fails);
    return g_fails ? 1 : 0;
}
