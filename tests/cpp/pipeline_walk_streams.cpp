// tests/cpp/pipeline_walk_streams.cpp -- the dependency structure
// ta_pipeline_step enqueues for a pipeline made by ta_pipeline_create_ex with
// `walk_streams` walk streams (bioinfo1_amd/csrc/ta_pipeline.cpp), on the CPU.
// As tests/cpp/pipeline_order.cpp: the file is linked against stub_ta.cpp's
// contexts and the recording stand-ins below for the HIP runtime's streams and
// events and the plans' fill / traceback entry points, which model what the
// real ones promise (a stream runs its work in order, an event carries what
// its stream held when recorded, a wait adds that to the waiting stream, an
// execution on another stream than its context's previous one first waits for
// that one).  Every launch then knows the set of launches that must have
// finished before it.  main() asserts that set for depth 2, 3, 4 x
// walk_streams 1, 2, depth (one and two chunks, with and without a ready
// event), the argument errors, and how walk_streams = 0 resolves against
// GPU_MAX_HW_QUEUES (tests/test_pipeline_walk_streams.py runs it).
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <algorithm>
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
ta_context* ta_affine_plan_context(const ta_affine_plan* p) { return p ? p->ctx : nullptr; }
uint32_t ta_affine_plan_chunks(const ta_affine_plan*) { return 1; }
int ta_affine_plan_execute_fill(ta_affine_plan* p, const ta_device_io*, void* s, uint32_t c) { return execute(p->ctx, 'F', c, s); }
int ta_affine_plan_execute_traceback(ta_affine_plan* p, const ta_device_io*, void* s, uint32_t c) { return execute(p->ctx, 'T', c, s); }

}  // extern "C"

namespace {

struct Slots {
    std::vector<ta_context*> ctxs;
    std::vector<ta_plan> plans;
    std::vector<ta_plan*> slots;
    Slots(uint32_t depth, uint32_t chunks) : ctxs(depth), plans(depth), slots(depth) {
        for (uint32_t s = 0; s < depth; ++s) {
            ta_context_create(0, &ctxs[s]);
            plans[s] = {ctxs[s], chunks};
            slots[s] = &plans[s];
        }
    }
    ~Slots() {
        for (ta_context* c : ctxs) ta_context_destroy(c);
    }
};

// depth slots of `chunks` chunks over `steps` steps on w walk streams; with_ready: every
// step's inputs are "uploaded" on a copy stream whose event is passed as ready
void run_case(uint32_t depth, uint32_t w, uint32_t chunks, int steps, bool with_ready) {
    reset();
    Slots S(depth, chunks);
    const ta_pipeline_options opt = {sizeof(ta_pipeline_options), w};
    ta_pipeline* pipe = nullptr;
    CHECK(ta_pipeline_create_ex(S.slots.data(), depth, &opt, &pipe) == TA_OK && pipe, "depth %u w %u", depth, w);
    if (!pipe) return;
    CHECK(ta_pipeline_walk_streams(pipe) == w, "depth %u w %u", depth, w);
    CHECK(g_live_streams.empty() && g_events == 0, "streams are created at the first step");
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
        if (g_step == 0)  // every walk stream exists after the first step, and one fill stream so far
            CHECK(g_high_streams.size() == w && g_live_streams.size() == w + 1, "first step: %zu streams, %zu high",
                  g_live_streams.size(), g_high_streams.size());
        launch('C', 0, caller);  // what the caller queues after the step (a snapshot of its results)
    }
    CHECK(g_live_streams.size() == depth + w && g_high_streams.size() == w, "%zu streams, %zu of high priority",
          g_live_streams.size(), g_high_streams.size());
    const int d = (int)depth, last_chunk = (int)chunks - 1;
    // the walk streams: those of the first w steps, all different and all of high priority
    std::vector<const void*> walk_stream;
    for (int j = 0; j < (int)w; ++j) walk_stream.push_back(g_ops[find('T', j, 0)].stream);
    CHECK(std::set<const void*>(walk_stream.begin(), walk_stream.end()).size() == w, "w %u: walk streams differ", w);
    for (const void* s : walk_stream) CHECK(g_high_streams.count(s) == 1, "a walk stream of high priority");
    for (int k = 0; k < steps; ++k) {
        const int f0 = find('F', k, 0), c = find('C', k);
        CHECK(f0 >= 0 && c >= 0, "step %d", k);
        const Op& fill = g_ops[f0];
        // fill k follows slot k % depth's previous use -- its fills, its tracebacks and what the
        // caller queued after them -- and through that everything older; nothing of steps
        // k - depth + 1 .. k - 1, whatever the walk streams
        CHECK(steps_of(fill.before, 'F') == upto(k - d), "fill %d depth %d w %u", k, d, w);
        CHECK(steps_of(fill.before, 'T') == upto(k - d), "fill %d depth %d w %u", k, d, w);
        CHECK(steps_of(fill.before, 'C') == upto(k - d), "fill %d depth %d w %u", k, d, w);
        if (k >= d) CHECK(fill.before.count(find('T', k - d, last_chunk)) == 1, "fill %d", k);
        if (with_ready) CHECK(steps_of(fill.before, 'U').count(k) == 1, "fill %d follows its upload", k);
        if (with_ready) CHECK(steps_of(fill.before, 'U').count(k + 1) == 0, "fill %d", k);
        CHECK(g_high_streams.count(fill.stream) == 0, "fill %d on a stream of default priority", k);
        for (int ch = 0; ch < (int)chunks; ++ch) {
            const int f = find('F', k, ch), t = find('T', k, ch);
            CHECK(f >= 0 && t >= 0 && g_ops[t].before.count(f) == 1, "walk %d.%d follows its fill", k, ch);
            // walk k (every chunk) on walk stream k % w: the step's index, not the slot's
            CHECK(g_ops[t].stream == walk_stream[k % (int)w], "walk %d.%d on walk stream %d", k, ch, k % (int)w);
            CHECK(g_ops[f].stream == fill.stream, "fill %d.%d", k, ch);
            // one workspace: a chunk's fill follows the walk of the chunk before it
            if (ch) CHECK(g_ops[f].before.count(find('T', k, ch - 1)) == 1, "fill %d.%d", k, ch);
            if (k >= 1) {
                const bool chained = g_ops[t].before.count(find('T', k - 1, last_chunk)) == 1;
                // w >= 2: walk k does not wait for walk k - 1; one walk stream: it does
                CHECK(chained == (w == 1), "walk %d.%d %s walk %d (w %u)", k, ch, chained ? "follows" : "does not follow",
                      k - 1, w);
            }
            // ... but for the walk before it on its own stream
            if (k >= (int)w) CHECK(g_ops[t].before.count(find('T', k - (int)w, last_chunk)) == 1, "walk %d.%d", k, ch);
        }
        // a fill stream per slot
        for (int j = 0; j < k; ++j)
            CHECK((g_ops[find('F', j, 0)].stream == fill.stream) == (j % d == k % d), "fill streams of steps %d, %d", j, k);
        // the caller's stream waited for walk k, and for every walk before it (step order)
        CHECK(g_ops[c].before.count(find('T', k, last_chunk)) == 1, "caller after step %d", k);
        CHECK(steps_of(g_ops[c].before, 'T') == upto(k), "caller after step %d", k);
    }
    ta_pipeline_destroy(pipe);
    CHECK(g_live_streams.empty() && g_events == 0, "destroy: %zu streams, %d events left", g_live_streams.size(), g_events);
}

void run_errors() {
    reset();
    Slots S(3, 1);
    ta_context* a = S.ctxs[0];
    ta_pipeline* pipe = reinterpret_cast<ta_pipeline*>(1);
    ta_pipeline_options opt = {sizeof(ta_pipeline_options), 4};
    CHECK(ta_pipeline_create_ex(S.slots.data(), 3, &opt, &pipe) == TA_ERR_ARG && !pipe, "walk_streams 4 at depth 3");
    CHECK(std::string(ta_last_error(a)).find("walk_streams") != std::string::npos, "%s", ta_last_error(a));
    opt.walk_streams = 3;
    pipe = reinterpret_cast<ta_pipeline*>(1);
    CHECK(ta_pipeline_create_ex(S.slots.data(), 2, &opt, &pipe) == TA_ERR_ARG && !pipe, "walk_streams 3 at depth 2");
    CHECK(std::string(ta_last_error(a)).find("walk_streams") != std::string::npos, "%s", ta_last_error(a));
    // the checks of ta_pipeline_create hold for the _ex entry too
    opt.walk_streams = 1;
    CHECK(ta_pipeline_create_ex(S.slots.data(), 1, &opt, &pipe) == TA_ERR_ARG && !pipe, "depth 1");
    CHECK(std::string(ta_last_error(a)).find("depth") != std::string::npos, "%s", ta_last_error(a));
    CHECK(ta_pipeline_create_ex(nullptr, 2, &opt, &pipe) == TA_ERR_ARG, "null slots");
    CHECK(ta_pipeline_create_ex(S.slots.data(), 2, &opt, nullptr) == TA_ERR_ARG, "null out");
    ta_affine_plan fa{S.ctxs[0]}, fb{S.ctxs[1]};
    ta_affine_plan* affine[] = {&fa, &fb};
    opt.walk_streams = 3;
    CHECK(ta_pipeline_create_affine_ex(affine, 2, &opt, &pipe) == TA_ERR_ARG && !pipe, "affine: walk_streams 3 at depth 2");
    opt.walk_streams = 2;
    CHECK(ta_pipeline_create_affine_ex(affine, 2, &opt, &pipe) == TA_OK && ta_pipeline_walk_streams(pipe) == 2, "affine");
    CHECK(ta_pipeline_step(pipe, nullptr, nullptr, nullptr, nullptr) == TA_ERR_ARG, "null io");
    CHECK(g_ops.empty() && g_live_streams.empty() && g_events == 0, "argument errors enqueue nothing");
    ta_pipeline_destroy(pipe);
    CHECK(ta_pipeline_walk_streams(nullptr) == 0, "null pipeline");
}

// what walk_streams = 0 becomes at `depth` under GPU_MAX_HW_QUEUES = env (null: unset)
uint32_t resolved(uint32_t depth, const char* env, const ta_pipeline_options* opt, bool plain = false) {
    if (env)
        setenv("GPU_MAX_HW_QUEUES", env, 1);
    else
        unsetenv("GPU_MAX_HW_QUEUES");
    Slots S(depth, 1);
    ta_pipeline* pipe = nullptr;
    const int r = plain ? ta_pipeline_create(S.slots.data(), depth, &pipe)
                        : ta_pipeline_create_ex(S.slots.data(), depth, opt, &pipe);
    CHECK(r == TA_OK && pipe, "depth %u under %s", depth, env ? env : "(unset)");
    const uint32_t w = ta_pipeline_walk_streams(pipe);
    ta_pipeline_destroy(pipe);
    return w;
}

// The queue rule: 0 resolves to w = min(TA_PIPELINE_WALK_STREAMS_DEFAULT, depth) when the
// process has at least depth + w + 1 hardware queues (unset: 4), else to 1.
void run_queue_rule() {
    reset();
    const ta_pipeline_options zero = {sizeof(ta_pipeline_options), 0};
    const ta_pipeline_options size_only = {sizeof(uint32_t), 7};  // (walk_streams lies beyond `size`: reads as 0)
    for (uint32_t depth : {2u, 3u, 4u}) {
        const uint32_t best = std::min<uint32_t>(TA_PIPELINE_WALK_STREAMS_DEFAULT, depth);
        const std::string enough = std::to_string(depth + best + 1), short_by_one = std::to_string(depth + best);
        for (const ta_pipeline_options* opt : {&zero, &size_only, (const ta_pipeline_options*)nullptr}) {
            CHECK(resolved(depth, nullptr, opt) == 1, "unset counts as 4 queues: depth %u", depth);
            CHECK(resolved(depth, "4", opt) == 1, "4 queues: depth %u", depth);
            CHECK(resolved(depth, "", opt) == 1, "empty counts as 4: depth %u", depth);
            CHECK(resolved(depth, "many", opt) == 1, "not a number counts as 4: depth %u", depth);
            CHECK(resolved(depth, "16", opt) == best, "16 queues: depth %u", depth);
            CHECK(resolved(depth, enough.c_str(), opt) == best, "%s queues: depth %u", enough.c_str(), depth);
            CHECK(resolved(depth, short_by_one.c_str(), opt) == 1, "%s queues: depth %u", short_by_one.c_str(), depth);
        }
        // an explicit count is the caller's, whatever the queues; ta_pipeline_create keeps one walk stream
        const ta_pipeline_options two = {sizeof(ta_pipeline_options), 2};
        CHECK(resolved(depth, "4", &two) == 2, "explicit 2 at 4 queues: depth %u", depth);
        CHECK(resolved(depth, "16", nullptr, true) == 1, "ta_pipeline_create at 16 queues: depth %u", depth);
    }
    unsetenv("GPU_MAX_HW_QUEUES");
}

}  // namespace

int main() {
    for (uint32_t depth : {2u, 3u, 4u})
        for (uint32_t w : std::set<uint32_t>{1u, 2u, depth})
            for (uint32_t chunks : {1u, 2u})
                for (bool ready : {false, true}) run_case(depth, w, chunks, 9, ready);
    run_errors();
    run_queue_rule();
    std::printf("pipeline walk streams: fails %d\n", g_fails);
    return g_fails ? 1 : 0;
}
