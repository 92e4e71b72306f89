/*
 * include/team_align_c.h -- extern "C" batch ABI of the MI355X team_alignment
 * engine (libteam_alignment.so).
 *
 * This is the boundary the reference's Align() path is replaced behind.  The
 * reference exposes one C++ entry, team::Align
 * (/root/reference/team_alignment/team_alignment.hpp:14-23, implemented at
 * team_alignment.cpp:49-350), called once per read by team_mapper.cpp:666,
 * 674, 755, 763.  Each function below states which part of that interface it
 * replaces.  Plain pointers and sizes only; no C++ or torch types; nothing
 * throws.  Every function returns a TA_* status.
 *
 * Semantics per pair are exactly team::Align's:
 *   score        -- the int the reference returns
 *   target_begin -- what the reference writes to *target_begin
 *                   (0 for global/semiGlobal, end column + 1 for local)
 *   CIGAR        -- the bytes the reference assigns to *cigar: decimal run
 *                   lengths of M / I (consumes target) / D (consumes query);
 *                   an empty alignment is the 2-byte string "1\0".
 */
#ifndef TEAM_ALIGN_C_H
#define TEAM_ALIGN_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* team::AlignmentType values (team_alignment.hpp:8-12). */
#define TA_GLOBAL 0
#define TA_LOCAL 1
#define TA_SEMI_GLOBAL 2

/* Status codes. */
#define TA_OK 0
#define TA_ERR_BAD_TYPE 1 /* reference: std::invalid_argument("Unknown AlignmentType provided.") */
#define TA_ERR_CIGAR 2    /* reference: std::invalid_argument("Unknown error in determining cigar string.") */
#define TA_ERR_ARG 3      /* null pointer / inconsistent sizes */
#define TA_ERR_DEVICE 4   /* no usable gfx950 device or a HIP runtime failure (see ta_last_error) */
#define TA_ERR_CAPACITY 5 /* caller-provided CIGAR arena too small */

typedef struct ta_context ta_context; /* device + stream + cached buffers; one per host thread */
typedef struct ta_plan ta_plan;       /* a batch's lengths, scoring and device workspace layout */

/* Message for a status code (static storage). */
const char* ta_status_string(int status);
/* Last error detail recorded on this context (e.g. the HIP error string). */
const char* ta_last_error(const ta_context* ctx);

/* Create a context on HIP device `device` (gfx950 required).  Replaces nothing
 * in the reference (which has no device state); team::Align keeps one per
 * calling thread so concurrent callers (team_mapper.cpp:596 OpenMP) are safe. */
int ta_context_create(int device, ta_context** out);
void ta_context_destroy(ta_context* ctx);
/* Free the context's cached device workspace and staging buffers (they are
 * grow-only: a large batch keeps its traceback-code workspace for the next
 * one).  Waits for the context's last execution.  The context stays usable. */
void ta_context_release(ta_context* ctx);

/* Device bytes the context holds in its grow-only traceback-code and
 * pass-boundary workspace -- the memory a plan's chunks reuse.  A caller sizing
 * ta_plan_create's workspace budget from hipMemGetInfo adds this back: the free
 * figure does not count memory the context will reuse.  (Staging and output
 * buffers are not included: a plan cannot reuse them.) */
uint64_t ta_context_held_bytes(const ta_context* ctx);

/* ---- Low-latency single pairs (the drop-in team::Align's path for calls that
 * fit).  Replaces team::Align's per-call synchronous computation
 * (team_alignment.cpp:49-56) as called by team_mapper.cpp:666-678 / 755-767:
 * a persistent kernel (one wave per slot) serves pairs posted in pinned host
 * memory, so a call costs no kernel launch and no copy.  One server per
 * (device, alignment type); its kernel starts with the first call and stops
 * after ~200 ms without calls.  Thread-safe: concurrent callers take
 * different slots. */
typedef struct ta_server ta_server;
int ta_server_create(int device, int type, uint32_t slots, ta_server** out); /* slots 1..64 */
void ta_server_destroy(ta_server* server);
/* 1 when an n x m pair with these scores runs on the server (n <= 4096,
 * m <= 16384; local mode: (n + m) * max|score| < 2^25). */
int ta_server_fits(const ta_server* server, uint32_t query_len, uint32_t target_len, int match, int mismatch,
                   int gap);
/* One pair, synchronous, team::Align's results (score, target_begin, the CIGAR
 * bytes when want_cigar).  TA_ERR_UNSERVED when the pair does not fit or no
 * slot is free: use ta_align_batch instead. */
int ta_server_align(ta_server* server, const char* query, uint32_t query_len, const char* target,
                    uint32_t target_len, int match, int mismatch, int gap, int want_cigar, int32_t* score,
                    uint32_t* target_begin, char* cigar, uint64_t cigar_capacity, uint32_t* cigar_len);
/* 1 while the server's kernel is resident. */
int ta_server_running(const ta_server* server);
/* Pause / resume (counted).  While paused, ta_server_align returns
 * TA_ERR_UNSERVED at once; ta_server_pause waits for the calls in flight and
 * stops the kernel, so that work on other streams of the device never queues
 * behind the persistent kernel on a shared hardware queue (a batch on the same
 * device pauses the server around its launches).  Pausing a server that is not
 * running only counts; the drop-in shim pauses its own servers around each
 * combined batch.  Work submitted outside the shim (ta_align_batch, plans, the
 * mapper) does not pause anything: a caller that mixes it with a live server on
 * one device pauses the server itself for the duration. */
int ta_server_pause(ta_server* server);
int ta_server_resume(ta_server* server);
/* Diagnostics: the device-side phase times (microseconds) of the last request
 * served in `slot`: [0] request + bytes into HBM, [1] fill + walk, [2] results
 * and CIGAR into the slot, [3] 0 (the release store of `done` is the fence). */
int ta_server_last_times(const ta_server* server, uint32_t slot, double* us_out4);

/* The drop-in team::Align (include/team_alignment.hpp) runs each call on:
 * the device set here (device >= 0; -1 clears the choice), else the device
 * named by the TEAM_ALIGN_DEVICE environment variable (read once), else the
 * calling thread's current HIP device (hipSetDevice) as of that thread's first
 * call (a thread keeps it: hipGetDevice per call would cost more than a small
 * pair's alignment).  TA_ERR_ARG for a device that does not exist. */
int ta_set_default_device(int device);
/* The calling thread's own choice, ahead of the three above: its drop-in calls
 * run on `device` (>= 0).  -1 drops the choice and makes the thread's next
 * call read its current HIP device again -- the call to make after a
 * hipSetDevice that should move the thread's team::Align calls with it.
 * TA_ERR_ARG for a device that does not exist. */
int ta_set_thread_device(int device);
/* The calling thread's current HIP device (0 when it has none) and the number of devices. */
int ta_current_device(void);
int ta_device_count(void);

/* Bytes of the per-pair CIGAR slot for an n x m pair: 2*(n+m)+2, an upper
 * bound on any run-length CIGAR of that pair (team_alignment.cpp:145-160). */
uint64_t ta_cigar_slot_bytes(uint32_t query_len, uint32_t target_len);

/*
 * Host-memory batch: the batched form of team::Align
 * (team_alignment.hpp:14-23), n_pairs independent calls with shared
 * type/match/mismatch/gap.  Inputs are SoA: concatenated bytes + per-pair
 * offset + length (length-delimited, not NUL-terminated, as Align takes them).
 * Outputs (host memory, n_pairs each): score[], target_begin[] (either may be
 * NULL, like Align's optional pointer), and when want_cigar != 0 the CIGARs
 * packed back to back into cigar_arena (capacity cigar_arena_bytes; at most
 * the sum of ta_cigar_slot_bytes is ever needed), pair p's bytes at
 * cigar_arena[cigar_off[p] .. cigar_off[p]+cigar_len[p]).
 * want_cigar == 0 is the reference's cigar == nullptr mode: no traceback.
 * Returns TA_ERR_BAD_TYPE for an unknown type (no pair is computed).
 * No device allocation per call once the context's grow-only buffers fit the
 * batch: per call one pinned upload of the plan arrays, offsets and (up to
 * 4 MB) sequences, the kernels, the downloads, one or two synchronisations.
 * Caller buffers may be pageable or pinned (pinned ones, e.g. allocated with
 * hipHostMalloc, transfer at full PCIe rate).
 */
int ta_align_batch(ta_context* ctx, uint32_t n_pairs, const char* query_bytes, const uint64_t* query_off,
                   const uint32_t* query_len, const char* target_bytes, const uint64_t* target_off,
                   const uint32_t* target_len, int type, int match, int mismatch, int gap, int want_cigar,
                   int32_t* score, uint32_t* target_begin, char* cigar_arena, uint64_t cigar_arena_bytes,
                   uint64_t* cigar_off, uint32_t* cigar_len);

/* ta_align_batch with plan flags (TA_PLAN_* below: kernel selection, e.g.
 * TA_PLAN_INT32_ONLY for one int32 wave per pair with its walk inside the
 * fill kernel).  Results are identical for every flag value. */
int ta_align_batch_flags(ta_context* ctx, uint32_t n_pairs, const char* query_bytes, const uint64_t* query_off,
                         const uint32_t* query_len, const char* target_bytes, const uint64_t* target_off,
                         const uint32_t* target_len, int type, int match, int mismatch, int gap, int want_cigar,
                         int32_t* score, uint32_t* target_begin, char* cigar_arena, uint64_t cigar_arena_bytes,
                         uint64_t* cigar_off, uint32_t* cigar_len, uint32_t flags);

/*
 * Device-resident batches (the mapper-side batching of SURVEY §8f and the
 * benchmark path).  A plan fixes the lengths (host arrays, copied) and the
 * scoring, lays out the device workspace (2-bit traceback pointers, pass
 * boundary rows) and chunks the batch when the pointer matrices exceed
 * workspace_budget bytes (0 = library default: half the free HBM, at most
 * 64 GiB).  flags: 0, or TA_PLAN_* below (kernel selection for tests and
 * measurements; results are identical either way).
 */
#define TA_PLAN_INT32_ONLY 1u /* no packed two-pairs-per-wave int16 kernels */
#define TA_PLAN_NO_FLEX 2u    /* no rebased couples of different shapes */
#define TA_PLAN_UNFUSED 4u    /* int32-only plans: traceback as its own kernel, not inside the fill */
#define TA_PLAN_WALK1 8u      /* local tracebacks: one pair per wave (run walk) */
#define TA_PLAN_WALK2 16u     /* local tracebacks: two pairs per wave (run walk), not one lane per pair */
#define TA_PLAN_SERIAL_PASSES 32u /* int32 fill: one wave sweeps all of a pair's passes (no pass pipelining) */
#define TA_PLAN_PASS_MAJOR 64u    /* pass-pipelined fills: tickets start-aligned (every pass 0 first), not end-aligned */
#define TA_PLAN_NO_BLK 128u       /* local plans of equal-shape couples: keep the [step][lane] code layout and the
                                     lane walks instead of the blocked layout and the band walks */
#define TA_PLAN_NO_CK 256u        /* those plans: the fill writes blocked codes walked by the band walks, never
                                     checkpoints walked by the recomputing walks (the default for large batches) */
#define TA_PLAN_CK 512u           /* those plans: checkpoints and recomputing walks at any batch size */
#define TA_PLAN_NO_FLEX_CK 1024u  /* plans with couples of different shapes: codes and the code walks, not checkpoints */
int ta_plan_create(ta_context* ctx, uint32_t n_pairs, const uint32_t* query_len_host,
                   const uint32_t* target_len_host, int type, int match, int mismatch, int gap, int want_cigar,
                   uint64_t workspace_budget, uint32_t flags, ta_plan** out);
void ta_plan_destroy(ta_plan* plan);
/* Total bytes of the device CIGAR slot arena the caller must provide. */
uint64_t ta_plan_cigar_slots_bytes(const ta_plan* plan);
/* Device workspace a plan's execution grows in its context (codes or checkpoints,
 * pass-boundary rows and the walks' event words), and the number of launch chunks. */
uint64_t ta_plan_workspace_bytes(const ta_plan* plan);
uint32_t ta_plan_chunks(const ta_plan* plan);
/* Pairs the plan runs in the packed two-pairs-per-wave int16 kernels (equal
 * shapes with scores provably within int16, or -- global / semi-global --
 * couples of different shapes in the rebased kernel); the rest use the int32
 * kernel. */
uint32_t ta_plan_dual_pairs(const ta_plan* plan);
/* Of those, the pairs in couples of different shapes / beyond int16 (ta_flex.hip). */
uint32_t ta_plan_flex_pairs(const ta_plan* plan);
/* 1 when the fill kernel walks its own pair (int32-only plans with CIGAR on). */
int ta_plan_fused(const ta_plan* plan);
/* The plan's walk (diagnostics, tests): local walk kind in bits 7:0 (64 band walks,
 * one lane per pair; 32 two pairs per wave; 16 lane walks; 0 one pair per wave),
 * bit 8 set when the codes use the blocked layout, bit 9 when the fill leaves
 * checkpoints instead and the walk recomputes codes around its path. */
int ta_plan_walk(const ta_plan* plan);
/* chunk_of_pair[p] = the chunk (0 .. ta_plan_chunks-1) whose launches align pair p
 * (caller-allocated, n_pairs entries).  Diagnostics: which chunk a checked pair ran in. */
int ta_plan_pair_chunks(const ta_plan* plan, uint32_t* chunk_of_pair);

/* Device pointers for one execution of a plan. */
typedef struct ta_device_io {
    const char* query_bytes;      /* device */
    const uint64_t* query_off;    /* device, n_pairs */
    const char* target_bytes;     /* device */
    const uint64_t* target_off;   /* device, n_pairs */
    int32_t* score;               /* device, n_pairs */
    uint32_t* target_begin;       /* device, n_pairs */
    char* cigar_slots;            /* device, ta_plan_cigar_slots_bytes(); unused when !want_cigar */
    uint64_t* cigar_start;        /* device, n_pairs: pair p's CIGAR starts at cigar_slots[cigar_start[p]] */
    uint32_t* cigar_len;          /* device, n_pairs */
} ta_device_io;

/* Enqueue the whole batch on `hip_stream` (a hipStream_t; NULL = the HIP
 * null stream, as everywhere in HIP).  Asynchronous: returns after enqueueing.
 * Plans of one context share its workspace: an execution on a different
 * stream than the context's previous one waits for that one first. */
int ta_plan_execute(ta_plan* plan, const ta_device_io* io, void* hip_stream);

/* After the plan's executions have completed (stream synchronised): TA_OK, or
 * TA_ERR_DEVICE when a kernel reported an internal failure since the last
 * check (the flexible fill's bounded pass hand-off poll gave up; see
 * ta_last_error).  Clears the flag.  ta_align_batch checks it itself. */
int ta_plan_check(ta_plan* plan);

/* Enqueue only the DP fill (scores/target_begin; traceback pointers into the
 * workspace) or only the traceback, for profiling the two kernels. */
int ta_plan_execute_fill(ta_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);
int ta_plan_execute_traceback(ta_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);

/* The traceback in two executions, for a caller that wants the two on
 * different streams (ta_pipeline_step below).  The traceback of checkpoint
 * plans and of band-walk plans is a walk kernel, which leaves each pair's runs
 * in the context's workspace, and a run formatter, which writes the CIGAR
 * text: ta_plan_format_is_split returns 1 for such a chunk (0 otherwise, and
 * for a chunk beyond the last).  There _walk enqueues the walk alone and
 * _format the formatter alone; _format belongs after _walk and before the
 * context's next fill, which the context's own ordering gives on any streams
 * (an execution on another stream than the previous one waits for it first).
 * For every other plan _walk is ta_plan_execute_traceback and _format
 * enqueues nothing.  Arguments, errors and the bytes written are those of
 * ta_plan_execute_traceback, which stays walk and formatter on one stream. */
int ta_plan_execute_walk(ta_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);
int ta_plan_execute_format(ta_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);
int ta_plan_format_is_split(const ta_plan* plan, uint32_t chunk);

/* The context a plan was created on, and a context's device. */
ta_context* ta_plan_context(const ta_plan* plan);
int ta_context_device(const ta_context* ctx);

/*
 * Batches back to back, batch k's traceback beside batch k+1's fill, and a
 * fill beside the tail of the fill before it.  The slots are `depth` (>= 2)
 * plans of the same shapes, each on a context of its own (a context owns the
 * workspace the fill writes and the walk reads) and all on one device;
 * TA_ERR_ARG otherwise, with the reason in ta_last_error of the first slot's
 * context.  The pipeline owns one fill stream per slot, one high-priority
 * walk stream and its events, all created at the first step; the plans and
 * contexts stay the caller's and outlive the pipeline.
 *
 * ta_pipeline_step enqueues the next batch on the next slot in turn (step k
 * uses slot k % depth; *slot_out, when not NULL, receives it) and returns:
 *   - on the slot's fill stream: a wait for whatever the caller had enqueued
 *     on `caller_stream` up to the step after this slot's previous one (its
 *     previous traceback included), a wait for `ready_event` (a hipEvent_t
 *     recorded after the upload of this batch's inputs; NULL: the inputs were
 *     resident before the pipeline's first step, or the host waited for them)
 *     and every chunk's fill;
 *   - on the walk stream: every chunk's traceback (after its fill);
 *   - on `caller_stream`: a wait for that traceback, so what the caller
 *     enqueues there after the call sees this step's results, and may
 *     overwrite its inputs.
 * Where every slot is a linear plan of one chunk whose traceback is split
 * (ta_plan_format_is_split) the walk stream gets the walk alone and
 * `caller_stream`, after its wait for the walk, the run formatter
 * (ta_plan_execute_format): the formatter of step k then runs beside the walk
 * of step k+1 instead of between the two, the caller's later work follows it
 * by stream order and the slot's next fill follows that (format_stream below;
 * ta_pipeline_format_split tells).  Results are the same bytes either way.
 * No fill waits for another slot's fill.  Errors (TA_ERR_ARG for a null
 * argument, TA_ERR_DEVICE) leave their message in ta_last_error of the slot's
 * context; argument errors enqueue nothing.  One thread at a time per pipeline.
 */
typedef struct ta_pipeline ta_pipeline;
int ta_pipeline_create(ta_plan* const* slots, uint32_t depth, ta_pipeline** out);
int ta_pipeline_step(ta_pipeline* pipe, const ta_device_io* io, void* ready_event, void* caller_stream,
                     uint32_t* slot_out);
void ta_pipeline_destroy(ta_pipeline* pipe);

/*
 * ta_pipeline_create with options.  `size` is sizeof(ta_pipeline_options) as
 * the caller was compiled (fields beyond it read as 0); a NULL `options` is
 * every field 0.  A field of 0 means the library's default.
 *
 * walk_streams = w (1 <= w <= depth; larger: TA_ERR_ARG, the message names
 * walk_streams): the pipeline owns w walk streams, all of high priority and
 * created at the first step, and step k's traceback (every chunk) runs on walk
 * stream k % w -- consecutive steps on different streams, so walk k+1 may
 * start beside walk k's tail and its run formatter instead of behind them.
 * Everything else is as above: a walk follows its own fill, the caller's
 * stream waits for every step's traceback in step order, a fill for its
 * slot's previous use only.  Results are the same bytes for every w.
 *
 * Hardware queues: the HIP runtime maps streams onto GPU_MAX_HW_QUEUES
 * hardware queues (environment variable; 4 when unset) and two streams on one
 * queue run one after the other.  walk_streams = 0 therefore resolves, when
 * the pipeline is created, to min(TA_PIPELINE_WALK_STREAMS_DEFAULT, depth)
 * only if GPU_MAX_HW_QUEUES (read then; unset counts as 4) is at least
 * depth + w + 1 -- the fill streams, the walk streams and the caller's --
 * and to 1 otherwise.  ta_pipeline_walk_streams returns the resolved count.
 * ta_pipeline_create / _create_affine keep one walk stream whatever the
 * environment.  The default is 1: on an MI355X two streams measured not
 * steadily faster than one for 10,000 pairs of 1 kb and three slower (DESIGN
 * 3.12), so the rule only matters to a build that defines another default.
 *
 * format_stream: 0, the default, puts the run formatter on the caller's stream
 * where the slots allow it (above; no further stream or hardware queue); 1
 * keeps it on the walk stream behind its walk, the order of
 * ta_plan_execute_traceback (for comparisons, and as a way back); anything
 * else is TA_ERR_ARG, the message names format_stream.  ta_pipeline_create /
 * _create_affine take the default.  ta_pipeline_format_split returns 1 when
 * the pipeline's steps enqueue walk and formatter apart, else 0.
 */
#ifndef TA_PIPELINE_WALK_STREAMS_DEFAULT
#define TA_PIPELINE_WALK_STREAMS_DEFAULT 1u
#endif
typedef struct ta_pipeline_options {
    uint32_t size;         /* sizeof(ta_pipeline_options) */
    uint32_t walk_streams; /* 0: the default (above) */
    uint32_t format_stream; /* 0: the default (above); 1: the formatter stays on the walk stream */
} ta_pipeline_options;
int ta_pipeline_create_ex(ta_plan* const* slots, uint32_t depth, const ta_pipeline_options* options,
                          ta_pipeline** out);
uint32_t ta_pipeline_walk_streams(const ta_pipeline* pipe);
int ta_pipeline_format_split(const ta_pipeline* pipe);

/* Pack n_pairs CIGARs from their slots (device: cigar_slots, cigar_start,
 * cigar_len as written by an execution) back to back into dst (device):
 * pair p's bytes go to dst[dst_off[p] ..).  Enqueued on hip_stream.  For a
 * caller that gathers CIGAR bytes between GPUs (bench.py's RCCL gather) or
 * downloads them.  The reference has no counterpart (one std::string per
 * team::Align call, team_alignment.cpp:160). */
int ta_compact_cigars(ta_context* ctx, uint32_t n_pairs, const char* cigar_slots, const uint64_t* cigar_start,
                      const uint32_t* cigar_len, const uint64_t* dst_off, char* dst, void* hip_stream);

/*
 * ---- Annotate: per-pair alignment coordinates, column counts and extended
 * '=' / 'X' CIGARs, computed on the device from a finished execution.  The
 * reference has no counterpart (team::Align returns a score, an M/I/D CIGAR
 * and target_begin only).
 *
 * The alignment columns are the ops of the pair's CIGAR in order.  An M
 * column at (i, j) is '=' when query[i] == target[j] as raw bytes
 * (match_func, team_alignment.cpp:20-23) and 'X' otherwise.  The extended
 * CIGAR is the same path with every M run split into maximal '=' / 'X' runs,
 * in the same decimal run-length form ("1\0" for the empty op string); it
 * never needs more than ta_cigar_slot_bytes(n, m) bytes, so its arena is
 * ta_plan_cigar_slots_bytes() again, and pair p's text lies in the same byte
 * range of that arena as its base CIGAR slot does in cigar_slots.
 *
 * The scored part of the path: global -- all of it; local -- all of it, ending
 * at the goal cell (query_end, target_end = target_begin_out - 1), the begins
 * being the ends minus the consumption; semi-global -- without the free first
 * run (I along row 0 or D along column 0) and without the run appended after
 * the goal cell (team_alignment.cpp:305-315): both are counted in n_free, the
 * begins are the cell after the leading run and the ends the goal cell.
 * Always n_eq + n_x + n_ins + n_del + n_free == the number of CIGAR columns.
 */
typedef struct ta_pair_info {
    uint32_t query_begin, query_end;   /* scored part of the path, 0-based half-open */
    uint32_t target_begin, target_end;
    uint32_t n_eq, n_x, n_ins, n_del;  /* columns of each class inside the scored part */
    uint32_t n_gap_runs;               /* maximal I runs + maximal D runs inside the scored part */
    uint32_t n_free;                   /* columns outside it (semi-global free ends), else 0 */
} ta_pair_info;                        /* 40 bytes */

typedef struct ta_annotate_io {
    ta_pair_info* info;    /* device, n_pairs; NULL = no records */
    char* eqx_slots;       /* device, ta_plan_cigar_slots_bytes(), not the execution's cigar_slots; NULL = no extended CIGAR */
    uint64_t* eqx_start;   /* device, n_pairs (with eqx_slots): pair p's text starts at eqx_slots[eqx_start[p]] */
    uint32_t* eqx_len;     /* device, n_pairs (with eqx_slots) */
} ta_annotate_io;

/* Enqueue the annotate pass over all pairs (of all chunks) on hip_stream:
 * asynchronous.  Enqueue it on the stream of the execution it annotates,
 * after that execution and before the plan's next one: it reads the plan's
 * goal cells and io's sequences, CIGAR slots, starts and lengths.
 * ta_compact_cigars packs the extended CIGARs like the base ones.
 * TA_ERR_ARG for a plan created with want_cigar == 0, a null io or out, and
 * eqx_slots without eqx_start / eqx_len. */
int ta_plan_annotate(ta_plan* plan, const ta_device_io* io, const ta_annotate_io* out, void* hip_stream);

/*
 * ---- Affine-gap extension (BASELINE config 5: "affine gaps + full CIGAR
 * traceback").  The reference has NO counterpart: team::Align is linear-gap
 * only (team_alignment.cpp:25-28, 102-116; the "Gotoh" of
 * team_alignment.hpp:11 is a label).  The semantics are defined in
 * oracle/affine_oracle.c (Gotoh E/F/H, the reference's tie order, boundaries,
 * goals, traceback and CIGAR format); a gap of length L costs
 * gap_open + L * gap_extend and a '-' byte makes its gap step free.  With
 * gap_open == 0 the results are byte-identical to team::Align with
 * gap = gap_extend (that part of parity is pinned to the reference goldens;
 * gap_open != 0 is unpinned).
 * Range: (max qlen + max tlen + 2) * max(|match|, |mismatch|,
 * |gap_open| + |gap_extend|) must be < 2^26, else TA_ERR_RANGE.
 */
#define TA_ERR_RANGE 6 /* affine scoring x lengths outside the int32-safe range */
#define TA_ERR_UNSERVED 7 /* ta_server_align: the pair is outside the server's limits, or every slot is busy */

typedef struct ta_affine_plan ta_affine_plan;

/* As ta_plan_create, with the affine scoring.  Traceback codes take 4 bits per
 * cell (source M/I/D/STOP + the E and F extension bits).  flags:
 * TA_PLAN_INT32_ONLY or 0. */
int ta_affine_plan_create(ta_context* ctx, uint32_t n_pairs, const uint32_t* query_len_host,
                          const uint32_t* target_len_host, int type, int match, int mismatch, int gap_open,
                          int gap_extend, int want_cigar, uint64_t workspace_budget, uint32_t flags,
                          ta_affine_plan** out);
void ta_affine_plan_destroy(ta_affine_plan* plan);
uint64_t ta_affine_plan_cigar_slots_bytes(const ta_affine_plan* plan);
uint64_t ta_affine_plan_workspace_bytes(const ta_affine_plan* plan);
uint32_t ta_affine_plan_chunks(const ta_affine_plan* plan);
/* Pairs the plan runs in the packed two-pairs-per-wave int16 affine fill
 * (global / semi-global couples of equal shape whose values provably fit). */
uint32_t ta_affine_plan_dual_pairs(const ta_affine_plan* plan);
int ta_affine_plan_pair_chunks(const ta_affine_plan* plan, uint32_t* chunk_of_pair);
/* Enqueue the whole batch / one chunk's fill / one chunk's traceback on hip_stream. */
int ta_affine_plan_execute(ta_affine_plan* plan, const ta_device_io* io, void* hip_stream);
int ta_affine_plan_execute_fill(ta_affine_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);
int ta_affine_plan_execute_traceback(ta_affine_plan* plan, const ta_device_io* io, void* hip_stream,
                                     uint32_t chunk);
/* As ta_plan_check: TA_ERR_DEVICE when a pass hand-off poll of the packed
 * affine fill (one wave per couple and pass) gave up; clears the flag. */
int ta_affine_plan_check(ta_affine_plan* plan);
/* As ta_plan_context; and a ta_pipeline (above) whose slots are affine plans. */
ta_context* ta_affine_plan_context(const ta_affine_plan* plan);
int ta_pipeline_create_affine(ta_affine_plan* const* slots, uint32_t depth, ta_pipeline** out);
/* As ta_pipeline_create_ex (its options, its walk-stream default and queue rule). */
int ta_pipeline_create_affine_ex(ta_affine_plan* const* slots, uint32_t depth, const ta_pipeline_options* options,
                                 ta_pipeline** out);
/* As ta_plan_annotate, for an affine plan's execution. */
int ta_affine_plan_annotate(ta_affine_plan* plan, const ta_device_io* io, const ta_annotate_io* out,
                            void* hip_stream);

/* Host-memory batch with affine gaps: ta_align_batch with gap -> (gap_open, gap_extend). */
int ta_align_batch_affine(ta_context* ctx, uint32_t n_pairs, const char* query_bytes, const uint64_t* query_off,
                          const uint32_t* query_len, const char* target_bytes, const uint64_t* target_off,
                          const uint32_t* target_len, int type, int match, int mismatch, int gap_open,
                          int gap_extend, int want_cigar, int32_t* score, uint32_t* target_begin,
                          char* cigar_arena, uint64_t cigar_arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len);

/*
 * ---- Banded extension: only the cells within a per-pair band of diagonals
 * are computed, so work and code workspace grow with n * band instead of
 * n * m.  The reference has NO counterpart (team::Align fills the whole
 * matrix); like the affine extension this is a plan family of its own and
 * nothing above changes behaviour.
 *
 * Definition, for a pair of lengths n (query) and m (target) and its band w:
 *   The band.  Cell (i, j), 0 <= i <= n, 0 <= j <= m, is in band iff
 *     lo <= j - i <= hi,  lo = min(0, m - n) - w,  hi = max(0, m - n) + w.
 *   (0, 0) and (n, m) are always in band; w >= max(n, m) puts every cell in
 *   band; boundary cells (row 0, column 0) obey the same rule.
 *   The recurrence is team::Align's (oracle/align_oracle.c restates it) with
 *   out-of-band cells not existing: for an in-band interior cell MATCH is
 *   always a candidate (its predecessor lies on the same diagonal), INSERT
 *   (left) and DELETE (up) only when their predecessor cell is in band.  Tie
 *   order (strict '>', M, then I, then D), free gap steps at '-' bytes, the
 *   local clamp and its "parent kept" rule are unchanged.
 *   Goals.  Global: (n, m).  Local: the first strict row-major maximum over
 *   the in-band interior cells ((1, 1) is always one); target_begin = gj + 1.
 *   Semi-global: the reference's scan over in-band cells only -- column m
 *   with i ascending, then row n, strict '>' -- and the trailing I / D run to
 *   (n, m) as today.  Traceback, reversal, RLE and "1\0" are unchanged.
 *   Degenerate pairs (n == 0 or m == 0): today's closed forms.
 * With every cell the unbanded walk visits in band, the results equal the
 * unbanded ones; a banded score is never above the unbanded score.
 * Range: (max qlen + max tlen + 2) * max(|match|, |mismatch|, |gap|) must be
 * < 2^26, else TA_ERR_RANGE (the affine extension's rule).
 */
typedef struct ta_banded_plan ta_banded_plan;

/* As ta_plan_create, with band[n_pairs] (host array, copied).  Codes are kept
 * only for the columns each 1024-row pass sweeps.  flags: 0. */
int ta_banded_plan_create(ta_context* ctx, uint32_t n_pairs, const uint32_t* query_len_host,
                          const uint32_t* target_len_host, const uint32_t* band_host, int type, int match,
                          int mismatch, int gap, int want_cigar, uint64_t workspace_budget, uint32_t flags,
                          ta_banded_plan** out);
void ta_banded_plan_destroy(ta_banded_plan* plan);
uint64_t ta_banded_plan_cigar_slots_bytes(const ta_banded_plan* plan);
uint64_t ta_banded_plan_workspace_bytes(const ta_banded_plan* plan);
uint32_t ta_banded_plan_chunks(const ta_banded_plan* plan);
int ta_banded_plan_pair_chunks(const ta_banded_plan* plan, uint32_t* chunk_of_pair);
/* Diagnostics: the in-band interior cells of all pairs (the numerator of a
 * cell-update rate) and the cells the kernels sweep (each pass's column range
 * times its rows). */
uint64_t ta_banded_plan_band_cells(const ta_banded_plan* plan);
uint64_t ta_banded_plan_swept_cells(const ta_banded_plan* plan);
/* Enqueue the whole batch / one chunk's fill / one chunk's traceback on hip_stream. */
int ta_banded_plan_execute(ta_banded_plan* plan, const ta_device_io* io, void* hip_stream);
int ta_banded_plan_execute_fill(ta_banded_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);
int ta_banded_plan_execute_traceback(ta_banded_plan* plan, const ta_device_io* io, void* hip_stream,
                                     uint32_t chunk);
/* As ta_plan_check (the banded kernels have no failure to report: TA_OK). */
int ta_banded_plan_check(ta_banded_plan* plan);
/* As ta_plan_annotate, for a banded plan's execution. */
int ta_banded_plan_annotate(ta_banded_plan* plan, const ta_device_io* io, const ta_annotate_io* out,
                            void* hip_stream);

/* Host-memory batch with a band per pair: ta_align_batch plus band[n_pairs]. */
int ta_align_batch_banded(ta_context* ctx, uint32_t n_pairs, const char* query_bytes, const uint64_t* query_off,
                          const uint32_t* query_len, const char* target_bytes, const uint64_t* target_off,
                          const uint32_t* target_len, const uint32_t* band, int type, int match, int mismatch,
                          int gap, int want_cigar, int32_t* score, uint32_t* target_begin, char* cigar_arena,
                          uint64_t cigar_arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len);

/*
 * ---- Banded affine extension: the affine-gap extension inside the banded
 * extension's band.  Work and code workspace grow with n * band (4 bits of
 * traceback code per swept cell) instead of n * m.  Neither the reference nor
 * the two extensions above have a counterpart; it is a plan family of its own
 * and nothing above changes behaviour.
 *
 * Definition, for a pair of lengths n (query) and m (target) and its band w:
 *   The band is the banded extension's: cell (i, j), 0 <= i <= n, 0 <= j <= m,
 *   exists iff lo <= j - i <= hi, lo = min(0, m - n) - w, hi = max(0, m - n) + w;
 *   boundary cells (row 0, column 0) obey the same rule.
 *   The recurrence is oracle/affine_oracle.c's Gotoh H/E/F with the cells
 *   outside the band not existing (go_t = gap_open + gap_extend and
 *   ge_t = gap_extend, both 0 at a '-' byte of the sequence the step consumes):
 *     E(i, j) = max(H(i, j-1) + go_t, E(i, j-1) + ge_t) when (i, j-1) is in
 *       band, else -inf; its extension bit is "2nd > 1st", strict.
 *     F(i, j) the same over (i-1, j).
 *     MATCH (the diagonal, whose predecessor lies on the same diagonal) is
 *     always a candidate of an in-band interior cell; INSERT wins iff
 *     E > diag, DELETE iff F > max(diag, E), both strict.  The local clamp
 *     keeps the source.
 *   Boundaries: H(i, 0) and H(0, j) are gap_open + L * gap_extend (global; 0
 *   at (0, 0)) or 0, where in band; E(i, 0) = F(0, j) = -inf.
 *   Goals are the banded extension's.  Global: (n, m).  Local: the first
 *   strict row-major maximum over the in-band interior cells, target_begin =
 *   gj + 1.  Semi-global: column m with i ascending, then row n, strict '>',
 *   over in-band cells only.
 *   The three-state walk, the reversal, the semi-global trailing run, the RLE
 *   and "1\0" are the affine oracle's.
 *   Degenerate pairs (n == 0 or m == 0): the affine closed forms (global:
 *   gap_open + L * gap_extend for L > 0, 0 for the empty pair).
 * With gap_open == 0 the results equal the banded extension's with gap =
 * gap_extend, at every band; with w >= max(n, m) they equal the affine
 * extension's; with every cell the unbanded affine walk visits in band they
 * equal the unbanded affine ones; a banded score is never above the unbanded
 * affine score.
 * Range: (max qlen + max tlen + 2) * max(|match|, |mismatch|,
 * |gap_open| + |gap_extend|) must be < 2^26, else TA_ERR_RANGE.
 */
typedef struct ta_banded_affine_plan ta_banded_affine_plan;

/* As ta_banded_plan_create, with gap -> (gap_open, gap_extend).  Codes take
 * 8 bytes per (pass, swept step, lane).  flags must be 0 (TA_ERR_ARG). */
int ta_banded_affine_plan_create(ta_context* ctx, uint32_t n_pairs, const uint32_t* query_len_host,
                                 const uint32_t* target_len_host, const uint32_t* band_host, int type, int match,
                                 int mismatch, int gap_open, int gap_extend, int want_cigar,
                                 uint64_t workspace_budget, uint32_t flags, ta_banded_affine_plan** out);
void ta_banded_affine_plan_destroy(ta_banded_affine_plan* plan);
uint64_t ta_banded_affine_plan_cigar_slots_bytes(const ta_banded_affine_plan* plan);
uint64_t ta_banded_affine_plan_workspace_bytes(const ta_banded_affine_plan* plan);
uint32_t ta_banded_affine_plan_chunks(const ta_banded_affine_plan* plan);
int ta_banded_affine_plan_pair_chunks(const ta_banded_affine_plan* plan, uint32_t* chunk_of_pair);
/* As ta_banded_plan_band_cells / _swept_cells. */
uint64_t ta_banded_affine_plan_band_cells(const ta_banded_affine_plan* plan);
uint64_t ta_banded_affine_plan_swept_cells(const ta_banded_affine_plan* plan);
/* Enqueue the whole batch / one chunk's fill / one chunk's traceback on hip_stream. */
int ta_banded_affine_plan_execute(ta_banded_affine_plan* plan, const ta_device_io* io, void* hip_stream);
int ta_banded_affine_plan_execute_fill(ta_banded_affine_plan* plan, const ta_device_io* io, void* hip_stream,
                                       uint32_t chunk);
int ta_banded_affine_plan_execute_traceback(ta_banded_affine_plan* plan, const ta_device_io* io, void* hip_stream,
                                            uint32_t chunk);
/* As ta_plan_check (these kernels have no failure to report: TA_OK). */
int ta_banded_affine_plan_check(ta_banded_affine_plan* plan);
/* As ta_plan_annotate, for a banded affine plan's execution. */
int ta_banded_affine_plan_annotate(ta_banded_affine_plan* plan, const ta_device_io* io, const ta_annotate_io* out,
                                   void* hip_stream);

/* Host-memory batch: ta_align_batch_banded with gap -> (gap_open, gap_extend). */
int ta_align_batch_banded_affine(ta_context* ctx, uint32_t n_pairs, const char* query_bytes,
                                 const uint64_t* query_off, const uint32_t* query_len, const char* target_bytes,
                                 const uint64_t* target_off, const uint32_t* target_len, const uint32_t* band,
                                 int type, int match, int mismatch, int gap_open, int gap_extend, int want_cigar,
                                 int32_t* score, uint32_t* target_begin, char* cigar_arena,
                                 uint64_t cigar_arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len);

/*
 * ---- Exact banded alignment: a banded execution certifies, pair by pair,
 * that its band held every optimal path -- its results are then the unbanded
 * ones byte for byte -- and an uncertified pair names the band that will.
 * Nothing above changes behaviour.
 *
 * Definition, for a pair of lengths n, m, its band w (clamped to max(n, m)),
 * the scoring, and hs = max(match, mismatch).  Linear gaps read gap_open = 0,
 * gap_extend = gap below.
 *   Full band.  If w >= min(n, m) every cell is in band; the same holds for a
 *     degenerate pair (n == 0 or m == 0).  The pair is exact.
 *   Uncertifiable scoring.  If gap > 0 (affine: gap_open > 0 or
 *     gap_extend > 0) nothing is certified short of the full band.
 *   Bound.  Every path that leaves the band crosses diagonal hi + 1 or lo - 1,
 *     and such a path takes at most k = min(n, m) - w - 1 diagonal steps.
 *       Local and semi-global:  U(w) = max(hs, 0) * k.
 *       Global linear:  U(w) = max(hs, 0) * k
 *                              + gap * max(0, |m - n| + 2 (w + 1) - dashes):
 *         such a path takes at least |m - n| + 2 (w + 1) gap steps; dashes is
 *         the number of '-' bytes in both sequences, and at most that many
 *         gap steps are free.
 *       Global affine:  gap -> gap_extend, plus 2 * gap_open when dashes == 0
 *         (the path needs at least one I run and one D run).
 *   Certified means score_banded(w) > U(w); the comparison is strict.
 *   Needed band.  needed(w, s) is the smallest w' > w with U(w') < s; if there
 *     is none below min(n, m), it is min(n, m).  U does not increase with w.
 *   Two rounds always suffice: a banded score never falls when the band grows,
 *     so the pair run at needed(w0, score(w0)) is certified.
 * ta_layout.h band_exact_bound / band_exact_needed evaluate the rule on the
 * host and in the kernel; tests/band_exact_ref.py restates it.
 */

/* After an execution of `plan` into io, on the same stream: exact_dev[p] = 1
 * when pair p is certified (its score, target_begin and CIGAR are the unbanded
 * ones) else 0; band_needed_dev[p] = the pair's clamped band where exact, else
 * needed(band, score).  Reads the plan's arrays, io->score and the sequences. */
int ta_banded_plan_certify(ta_banded_plan* plan, const ta_device_io* io, uint8_t* exact_dev,
                           uint32_t* band_needed_dev, void* hip_stream);
int ta_banded_affine_plan_certify(ta_banded_affine_plan* plan, const ta_device_io* io, uint8_t* exact_dev,
                                  uint32_t* band_needed_dev, void* hip_stream);

/* Host-memory batches with the unbanded results at banded cost:
 * ta_align_batch_banded[_affine] run at band_start[p] (NULL: the start rule
 * max(64, ceil(min(n, m) / 16)) -- a choice, not a measurement), certified,
 * and the uncertified pairs run once more at their needed band, as one banded
 * batch over gathered offsets into the same byte buffers.  For every pair the
 * score, target_begin and CIGAR equal ta_align_batch's (linear) or
 * ta_align_batch_affine's; the outputs are laid out as ta_align_batch_banded
 * lays them out (CIGARs back to back in pair order).  band_used (optional):
 * the clamped band each result was computed at; rounds (optional): 1 or 2.
 * Errors are the banded entries'. */
int ta_align_batch_banded_exact(ta_context* ctx, uint32_t n_pairs, const char* query_bytes,
                                const uint64_t* query_off, const uint32_t* query_len, const char* target_bytes,
                                const uint64_t* target_off, const uint32_t* target_len, const uint32_t* band_start,
                                int type, int match, int mismatch, int gap, int want_cigar, int32_t* score,
                                uint32_t* target_begin, char* cigar_arena, uint64_t cigar_arena_bytes,
                                uint64_t* cigar_off, uint32_t* cigar_len, uint32_t* band_used, uint8_t* rounds);
int ta_align_batch_banded_affine_exact(ta_context* ctx, uint32_t n_pairs, const char* query_bytes,
                                       const uint64_t* query_off, const uint32_t* query_len,
                                       const char* target_bytes, const uint64_t* target_off,
                                       const uint32_t* target_len, const uint32_t* band_start, int type, int match,
                                       int mismatch, int gap_open, int gap_extend, int want_cigar, int32_t* score,
                                       uint32_t* target_begin, char* cigar_arena, uint64_t cigar_arena_bytes,
                                       uint64_t* cigar_off, uint32_t* cigar_len, uint32_t* band_used,
                                       uint8_t* rounds);

/*
 * ---- Anchored (free-end) alignment: the path starts at the known cell (0, 0)
 * and the score chooses where it stops -- the alignment a seed-and-extend
 * mapper runs at the two ends of a chain.  Neither the reference nor the
 * extensions above have a counterpart; it is a plan family of its own, reached
 * only through the entries below, and nothing above changes behaviour (type 3
 * stays "Unknown AlignmentType provided." everywhere else).
 *
 * Definition, for a pair of lengths n (query) and m (target) and its band w
 * (tests/anchored_ref.py restates it):
 *   The band is the banded extension's: cell (i, j) exists iff
 *   lo <= j - i <= hi, lo = min(0, m - n) - w, hi = max(0, m - n) + w;
 *   w >= max(n, m) holds every cell.
 *   Boundaries are global's, where in band: H(i, 0) = i * gap, H(0, j) =
 *   j * gap, whatever the bytes ('-' included); affine: gap_open + L *
 *   gap_extend, 0 at (0, 0), E(i, 0) = F(0, j) = -inf.
 *   The interior recurrence is the banded extension's global one (linear:
 *   strict '>' in the order M, I, D, free gap steps at '-' bytes) or the
 *   banded affine extension's global H/E/F.  No clamp.
 *   Goal: (0, 0) with score 0, unless some in-band interior cell (i, j >= 1)
 *   has H > 0; then the first strict row-major maximum over the in-band
 *   interior cells.  Boundary cells other than (0, 0) are never goals.
 *   score = H(goal) >= 0.
 *   Walk: the global walk from the goal (gi, gj) to (0, 0) (row 0 emits I x j,
 *   column 0 D x i; affine: the three-state walk from H-state); reversal, RLE
 *   and "1\0" for the empty op string are the reference's.  The CIGAR consumes
 *   exactly gi query and gj target bytes.
 *   Outputs per pair: score, query_end = gi, target_end = gj, CIGAR.  The
 *   target_begin array of ta_device_io is written 0.
 *   Degenerate pairs (n == 0 or m == 0): goal (0, 0), score 0, "1\0".
 * With a full band and gi, gj > 0, score and CIGAR are those of the global
 * alignment of query[0, gi) against target[0, gj), and no pair of prefixes has
 * a higher global score.  With gap_open == 0 the affine kernels give the linear
 * kernels' results at every band.  A banded score is never above the full-band
 * score.
 * Range: the banded families' rule ((max qlen + max tlen + 2) * max(|match|,
 * |mismatch|, |gap_open| + |gap_extend|) < 2^26), else TA_ERR_RANGE.
 * Certification (ta_*_plan_certify, the *_exact batches) does not cover this
 * mode.
 */
typedef struct ta_anchored_plan ta_anchored_plan;

#define TA_ANCHORED_AFFINE_KERNELS 1u /* run the affine kernels even at gap_open == 0 (same results) */

/* As ta_banded_affine_plan_create without `type`.  gap_open == 0 runs the
 * linear kernels (2-bit codes, gap = gap_extend) unless flags holds
 * TA_ANCHORED_AFFINE_KERNELS; any other gap_open the affine kernels.  Other
 * flag bits: TA_ERR_ARG. */
int ta_anchored_plan_create(ta_context* ctx, uint32_t n_pairs, const uint32_t* query_len_host,
                            const uint32_t* target_len_host, const uint32_t* band_host, int match, int mismatch,
                            int gap_open, int gap_extend, int want_cigar, uint64_t workspace_budget,
                            uint32_t flags, ta_anchored_plan** out);
void ta_anchored_plan_destroy(ta_anchored_plan* plan);
uint64_t ta_anchored_plan_cigar_slots_bytes(const ta_anchored_plan* plan);
uint64_t ta_anchored_plan_workspace_bytes(const ta_anchored_plan* plan);
uint32_t ta_anchored_plan_chunks(const ta_anchored_plan* plan);
int ta_anchored_plan_pair_chunks(const ta_anchored_plan* plan, uint32_t* chunk_of_pair);
/* As ta_banded_plan_band_cells / _swept_cells. */
uint64_t ta_anchored_plan_band_cells(const ta_anchored_plan* plan);
uint64_t ta_anchored_plan_swept_cells(const ta_anchored_plan* plan);
/* Enqueue the whole batch / one chunk's fill / one chunk's traceback on hip_stream. */
int ta_anchored_plan_execute(ta_anchored_plan* plan, const ta_device_io* io, void* hip_stream);
int ta_anchored_plan_execute_fill(ta_anchored_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);
int ta_anchored_plan_execute_traceback(ta_anchored_plan* plan, const ta_device_io* io, void* hip_stream,
                                       uint32_t chunk);
/* As ta_plan_check (these kernels have no failure to report: TA_OK). */
int ta_anchored_plan_check(ta_anchored_plan* plan);
/* As ta_plan_annotate: begins 0 / 0, ends gi / gj, n_free = 0; the counts and
 * the =/X CIGAR are the path's. */
int ta_anchored_plan_annotate(ta_anchored_plan* plan, const ta_device_io* io, const ta_annotate_io* out,
                              void* hip_stream);
/* After an execution (or its fills; want_cigar == 0 plans too), on the same
 * stream: the goal cells into query_end_dev[P] and target_end_dev[P].
 * Asynchronous. */
int ta_anchored_plan_ends(ta_anchored_plan* plan, uint32_t* query_end_dev, uint32_t* target_end_dev,
                          void* hip_stream);

/* Host-memory batch: ta_align_batch_banded_affine without `type`; the goal
 * cells (either may be NULL) in place of target_begin. */
int ta_align_batch_anchored(ta_context* ctx, uint32_t n_pairs, const char* query_bytes, const uint64_t* query_off,
                            const uint32_t* query_len, const char* target_bytes, const uint64_t* target_off,
                            const uint32_t* target_len, const uint32_t* band, int match, int mismatch,
                            int gap_open, int gap_extend, int want_cigar, int32_t* score, uint32_t* query_end,
                            uint32_t* target_end, char* cigar_arena, uint64_t cigar_arena_bytes,
                            uint64_t* cigar_off, uint32_t* cigar_len);

/*
 * ---- Z-drop on anchored alignment: stop the sweep once the end has died.
 * Cell values are anchored alignment's: same band, boundaries, recurrence, tie
 * order and '-' bytes, in both gap families; nothing is pruned.  The drop only
 * decides which cells EXIST for the goal scan, and -- like ksw2's -- it is tied
 * to the order in which the fill sweeps them (tests/anchored_zdrop_ref.py
 * restates it; the geometry is ta_layout.h band_drop_*):
 *   Step index.  An in-band interior cell (i, j) lies in pass p = (i-1) div 1024
 *   and is computed at step tau(i, j) = j - c0(p) + ((i-1) mod 1024) div 16 of
 *   it, c0(p) = max(1, 1024 p + 1 + lo) the pass's first swept column.  Its
 *   segment is (p, tau div 64).  Pass p has ceil(steps_p / 64) segments,
 *   steps_p = c1(p) - c0(p) + 1 + nl_p - 1, c1(p) = min(m, 1024 p + rows_p + hi),
 *   nl_p = ceil(rows_p / 16), rows_p the pass's query rows.
 *   Scan.  Segments in order (pass, then segment), B = 0 at the start:
 *     S = the maximum of -1 and every H of the segment's in-band interior cells
 *     with i <= n (an empty segment: -1);
 *     if B >= Z and S < B - Z the pair DROPS: this segment's cells still exist,
 *     every later segment's cells, and those of later passes, do not;
 *     otherwise B = max(B, S).
 *   Goal: (0, 0) with score 0 unless an existing cell has H > 0, else the first
 *   strict row-major maximum over the existing cells.
 *   Walk, CIGAR, "1\0", degenerate pairs and the range rule are unchanged.
 *   Z: 0 <= zdrop <= INT32_MAX.  zdrop < 0 is off: the plan, the kernels and
 *   the results are ta_anchored_plan_create's.
 *   swept_steps, per pair: the fill steps the pair executed -- the whole passes
 *   before the drop plus min(64 (s + 1), steps_p) in the dropping pass (p, s);
 *   the sum of steps_p when nothing drops; 0 for a degenerate pair.
 * A drop needs a scoring with negative drift (2/-4/-4, say): at 1/-1/-1 random
 * DNA drifts upward inside a band and nothing drops.
 * Planning (codes, slots, chunks, boundary rows) is sized as without z-drop: a
 * drop only leaves workspace unused.  _annotate, _ends, _check and _pair_chunks
 * work unchanged on a z-drop plan; certification does not cover the mode.
 */
int ta_anchored_plan_create_zdrop(ta_context* ctx, uint32_t n_pairs, const uint32_t* query_len_host,
                                  const uint32_t* target_len_host, const uint32_t* band_host, int match,
                                  int mismatch, int gap_open, int gap_extend, int want_cigar,
                                  uint64_t workspace_budget, uint32_t flags, int32_t zdrop, ta_anchored_plan** out);
/* Z-drop plans (else TA_ERR_ARG), after an execution (or its fills; want_cigar
 * == 0 plans too), on the same stream: swept_steps into steps_dev[P].
 * Asynchronous. */
int ta_anchored_plan_swept_steps(ta_anchored_plan* plan, uint32_t* steps_dev, void* hip_stream);
/* ta_align_batch_anchored with Z (zdrop < 0: exactly that call) and, where
 * zdrop >= 0, the per-pair swept_steps (may be NULL). */
int ta_align_batch_anchored_zdrop(ta_context* ctx, uint32_t n_pairs, const char* query_bytes,
                                  const uint64_t* query_off, const uint32_t* query_len, const char* target_bytes,
                                  const uint64_t* target_off, const uint32_t* target_len, const uint32_t* band,
                                  int match, int mismatch, int gap_open, int gap_extend, int want_cigar,
                                  int32_t* score, uint32_t* query_end, uint32_t* target_end, char* cigar_arena,
                                  uint64_t cigar_arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len,
                                  int32_t zdrop, uint32_t* swept_steps);

/*
 * ---- The row-stripe z-drop rule: a second, selectable definition of the drop.
 * The rule above (TA_ZDROP_SEGMENT) follows the fill's sweep, whose segments at
 * the end of a 1024-row pass and at the start of a pass with c0 > 1 hold only
 * cells near one edge of the band: at w > 32 it can drop a LIVE end at a pass
 * boundary.  The stripe rule is tied to rows.  Every stripe holds the cells
 * through which any path crosses its rows, so a live end cannot drop, whatever
 * the band and wherever a pass boundary falls: TA_ZDROP_STRIPE is the rule to
 * use above w = 32.  (The default stays TA_ZDROP_SEGMENT: the existing entries
 * keep their results, and the segment rule detects a dead end about one
 * stripe's sweep sooner.)
 * Cell values, band, boundaries, tie order, '-' bytes, walk, "1\0", degenerate
 * pairs, the range rule and 0 <= Z <= INT32_MAX are as above; nothing is
 * pruned.  The rule only decides which cells EXIST for the goal scan
 * (tests/anchored_zdrop_stripe_ref.py restates it; the geometry is ta_layout.h
 * band_stripe_*):
 *   Stripe g is rows 16 g + 1 .. min(16 g + 16, n), g = 0 .. ceil(n / 16) - 1.
 *   Every row has an in-band interior cell, so no stripe is empty.
 *   Stripe best: S_g = the maximum of -1 and every H of the stripe's in-band
 *   interior cells.
 *   Scan.  Stripes in order, B = 0 at the start: if B >= Z and S_g < B - Z the
 *   pair DROPS at stripe g: stripe g's rows still exist, every later row does
 *   not; otherwise B = max(B, S_g).  B carries across pass boundaries.
 *   Goal: (0, 0) with score 0 unless an existing cell has H > 0, else the first
 *   strict row-major maximum over the existing cells.  (It never lies in the
 *   dropping stripe: S_g < B - Z <= B.)
 *   swept_steps.  The fill tests the rule after every 64th step of a pass and
 *   after the pass's last step, on every stripe whose last cell has been
 *   computed.  Stripe g lies in pass p = g div 64 as lane l = g mod 64; its last
 *   cell is computed at step tau_done = min(m, i_last + hi) - c0(p) + l, i_last =
 *   min(n, 16 g + 16).  A drop at g executes the whole passes before p plus
 *   min(steps_p, 64 (tau_done div 64 + 1)) steps; without a drop the sum of
 *   steps_p; 0 for a degenerate pair.  tau_done strictly increases with l, so
 *   the finished stripes are a prefix and testing in batches gives the
 *   sequential scan's answer.  Rows below the dropping stripe that the fill has
 *   computed by then do not exist all the same.
 * rule: TA_ZDROP_SEGMENT or TA_ZDROP_STRIPE, else TA_ERR_ARG (whatever zdrop).
 * zdrop < 0 is off for either rule.  Planning is the segment rule's; _swept_steps,
 * _ends, _annotate, _check and _pair_chunks work unchanged on a stripe plan;
 * certification does not cover the mode.  `flags` as ta_anchored_plan_create.
 */
#define TA_ZDROP_SEGMENT 0
#define TA_ZDROP_STRIPE 1
int ta_anchored_plan_create_zdrop_rule(ta_context* ctx, uint32_t n_pairs, const uint32_t* query_len_host,
                                       const uint32_t* target_len_host, const uint32_t* band_host, int match,
                                       int mismatch, int gap_open, int gap_extend, int want_cigar,
                                       uint64_t workspace_budget, uint32_t flags, int32_t zdrop, int rule,
                                       ta_anchored_plan** out);
int ta_align_batch_anchored_zdrop_rule(ta_context* ctx, uint32_t n_pairs, const char* query_bytes,
                                       const uint64_t* query_off, const uint32_t* query_len,
                                       const char* target_bytes, const uint64_t* target_off,
                                       const uint32_t* target_len, const uint32_t* band, int match, int mismatch,
                                       int gap_open, int gap_extend, int want_cigar, int32_t* score,
                                       uint32_t* query_end, uint32_t* target_end, char* cigar_arena,
                                       uint64_t cigar_arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len,
                                       int32_t zdrop, int rule, uint32_t* swept_steps);

#ifdef __cplusplus
}
#endif

#endif /* TEAM_ALIGN_C_H */
