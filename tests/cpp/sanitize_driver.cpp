// tests/cpp/sanitize_driver.cpp -- host code of the build under the CPU
// sanitizers (tests/test_host_sanitizers.py builds this with
// -fsanitize=address,undefined and with -fsanitize=thread).  Modes:
//   oracle CASES     the C restatement (oracle/align_oracle.c) and the affine
//                    definition (oracle/affine_oracle.c) on the golden cases
//                    "type match mismatch gap qhex thex score tb cigarhex|-|ERR"
//                    (stdin-style file): results, path check, affine(open 0) == linear
//   planner SEED N T the host planner (bioinfo1_amd/csrc/ta_planner.cpp) on N
//                    random batches from T threads at once: every pair planned
//                    exactly once, chunk / workspace / task invariants
//                    (linear, affine and, at four band widths, banded plans)
//   blocks SEED N    the plans' device blocks (ta_plan_block.h) on N such
//                    batches: layout, pack and bind against host buffers
//   fastx PATH Q     the FASTA/FASTQ reader (tm_fastx.cpp): record count + checksum
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../bioinfo1_amd/csrc/ta_plan_block.h"
#include "../../bioinfo1_amd/csrc/ta_planner.h"
#include "../../bioinfo1_amd/csrc/tm_fastx.h"

extern "C" {
int oracle_align(const char* q, unsigned n, const char* t, unsigned m, int type, int match, int mismatch, int gap,
                 int want_cigar, int* score_out, unsigned* target_begin_out, char* cigar_out, size_t cigar_cap,
                 size_t* cigar_len);
int oracle_align_affine(const char* q, unsigned n, const char* t, unsigned m, int type, int match, int mismatch,
                        int open, int extend, int want_cigar, int* score_out, unsigned* target_begin_out,
                        char* cigar_out, size_t cigar_cap, size_t* cigar_len);
int oracle_cigar_check(const char* q, unsigned n, const char* t, unsigned m, int type, int match, int mismatch,
                       int gap, const char* cig, size_t clen, int score, unsigned target_begin);
}

namespace {

int fails = 0;
#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                         \
        }                                                                    \
    } while (0)

std::string unhex(const std::string& h) {
    std::string s;
    if (h == "-") return s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return s;
}

int run_oracle(const char* path) {
    std::ifstream in(path);
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        std::istringstream is(line);
        int type, ma, mi, g, want_score;
        unsigned want_tb;
        std::string qh, th, ws, wtb, wc;
        is >> type >> ma >> mi >> g >> qh >> th >> ws >> wtb >> wc;
        const std::string q = unhex(qh), t = unhex(th);
        std::vector<char> buf(2 * (q.size() + t.size()) + 2);
        int score = 0;
        unsigned tb = 0;
        size_t clen = 0;
        const int r = oracle_align(q.data(), (unsigned)q.size(), t.data(), (unsigned)t.size(), type, ma, mi, g, 1,
                                   &score, &tb, buf.data(), buf.size(), &clen);
        ++n_cases;
        if (ws == "ERR") {
            CHECK(r != 0);
            continue;
        }
        want_score = std::stoi(ws);
        want_tb = (unsigned)std::stoul(wtb);
        CHECK(r == 0);
        CHECK(score == want_score);
        CHECK(tb == want_tb);
        CHECK(std::string(buf.data(), clen) == unhex(wc));
        CHECK(oracle_cigar_check(q.data(), (unsigned)q.size(), t.data(), (unsigned)t.size(), type, ma, mi, g,
                                 buf.data(), clen, score, tb) == 0);
        // the affine definition with gap_open = 0 is team::Align with gap = gap_extend
        std::vector<char> abuf(buf.size());
        int as = 0;
        unsigned atb = 0;
        size_t alen = 0;
        const int ar = oracle_align_affine(q.data(), (unsigned)q.size(), t.data(), (unsigned)t.size(), type, ma, mi,
                                           0, g, 1, &as, &atb, abuf.data(), abuf.size(), &alen);
        if (ar == 0) {
            CHECK(as == score);
            CHECK(atb == tb);
            CHECK(std::string(abuf.data(), alen) == std::string(buf.data(), clen));
        }
    }
    std::printf("oracle cases %d fails %d\n", n_cases, fails);
    return fails ? 1 : 0;
}

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// What the three families' plans share (ta_planner.h PlanBase, ChunkSpan): `order` is a
// permutation, the chunks tile it, every chunk lies within the workspace, every pair's
// codes and boundary row lie inside its chunk, and the slot offsets add up.
// chunk_codes(c) / chunk_bnd(c): a chunk's totals; pair_codes(x): the code entries pair x needs.
template <class P, class ChunkCodes, class ChunkBnd, class PairCodes>
void check_common(const P& pl, uint64_t ws_codes, uint64_t ws_bnd, ChunkCodes chunk_codes, ChunkBnd chunk_bnd,
                  PairCodes pair_codes) {
    const uint32_t N = pl.n_pairs;
    std::vector<int> seen(N, 0);
    for (uint32_t x : pl.order) {
        CHECK(x < N);
        if (x < N) ++seen[x];
    }
    for (uint32_t p = 0; p < N; ++p) CHECK(seen[p] == 1);
    uint64_t count = 0;
    for (const auto& c : pl.chunks) {
        CHECK(c.begin == count && c.count > 0);
        count += c.count;
        CHECK(chunk_codes(c) <= ws_codes);
        CHECK(chunk_bnd(c) <= ws_bnd);
        for (uint32_t k = c.begin; k < c.begin + c.count && k < N; ++k) {
            const uint32_t x = pl.order[k];
            CHECK(pl.ptr_off[x] + (pl.want_cigar ? pair_codes(x) : 0) <= chunk_codes(c));
            CHECK(pl.bnd_off[x] + ta::bnd_words(pl.qlen[x], pl.tlen[x]) <= chunk_bnd(c));
        }
    }
    CHECK(count == N);
    uint64_t so = 0;
    for (uint32_t p = 0; p < N; ++p) {
        CHECK(pl.slot_off[p] == so);
        so += ta::cigar_slot_bytes(pl.qlen[p], pl.tlen[p]);
    }
    CHECK(so == pl.slots_bytes);
}

// Pipelined int32 tasks (linear and affine): every (single, pass) of a chunk with
// spasses > 1 exactly once, a task's predecessor ticketed earlier; its pair holds
// two record buffers of 4 entries per column.
template <class P, class ChunkBnd>
void check_single_tasks(const P& pl, ChunkBnd chunk_bnd) {
    bool piped = false;
    for (const auto& c : pl.chunks) piped |= c.spasses > 1;
    CHECK(piped == !pl.single_task_off.empty());
    if (!piped) return;
    CHECK(pl.single_task_off.size() == pl.singles.size() + 1);
    for (const auto& c : pl.chunks) {
        if (c.spasses < 2) continue;
        std::set<uint64_t> seen_tasks;
        uint32_t maxp = 0;
        for (uint32_t w = c.sbegin; w < c.sbegin + c.scount; ++w) {
            const uint32_t x = pl.singles[w];
            const uint32_t want = pl.qlen[x] && pl.tlen[x] ? ta::n_passes(pl.qlen[x]) : 0;
            CHECK(pl.single_task_off[w + 1] - pl.single_task_off[w] == want);
            maxp = std::max(maxp, want);
            if (want > 1) CHECK(pl.bnd_off[x] + 4ull * (pl.tlen[x] + 1) <= chunk_bnd(c));
        }
        CHECK(maxp == c.spasses);
        for (uint32_t k = pl.single_task_off[c.sbegin]; k < pl.single_task_off[c.sbegin + c.scount]; ++k) {
            const uint64_t code = pl.single_tasks[k];
            const uint32_t w = (uint32_t)(code >> 32), ps = (uint32_t)code;
            CHECK(w >= c.sbegin && w < c.sbegin + c.scount);
            if (ps) CHECK(seen_tasks.count(code - 1) == 1);  // predecessor ticketed earlier
            if (w < pl.singles.size()) CHECK(ps < pl.single_task_off[w + 1] - pl.single_task_off[w]);
            seen_tasks.insert(code);
        }
        CHECK(seen_tasks.size() == pl.single_task_off[c.sbegin + c.scount] - pl.single_task_off[c.sbegin]);
    }
}

void check_linear(const ta::Plan& pl, uint64_t budget) {
    const uint32_t P = pl.n_pairs;
    const auto chunk_bnd = [](const ta::Plan::Chunk& c) { return c.bnd_words; };
    check_common(
        pl, pl.ws_ptr_dwords, pl.ws_bnd_words, [](const ta::Plan::Chunk& c) { return c.ptr_dwords; }, chunk_bnd,
        [&](uint32_t x) { return ta::ptr_dwords_any(pl.qlen[x], pl.tlen[x], pl.blk); });
    // units partition the pairs: singles + duals + flex (a self-coupled flex pair counts once)
    std::vector<int> unit(P, 0);
    for (uint32_t x : pl.singles) ++unit[x];
    for (size_t k = 0; k + 1 < pl.duals.size(); k += 2) {  // a lone pair may be coupled with itself
        ++unit[pl.duals[k]];
        if (pl.duals[k + 1] != pl.duals[k]) ++unit[pl.duals[k + 1]];
    }
    for (size_t k = 0; k + 1 < pl.flexes.size(); k += 2) {
        ++unit[pl.flexes[k]];
        if (pl.flexes[k + 1] != pl.flexes[k]) ++unit[pl.flexes[k + 1]];
    }
    for (uint32_t p = 0; p < P; ++p) CHECK(unit[p] == 1);
    uint64_t s = 0, d = 0, f = 0;
    for (const auto& c : pl.chunks) {
        CHECK(c.sbegin == s && c.dbegin == d && c.fbegin == f);
        s += c.scount;
        d += c.dcount;
        f += c.fcount;
        // a chunk exceeds the budget only when it holds a single unit
        if (c.ptr_dwords * 4 > budget) CHECK(c.scount + c.dcount + c.fcount == 1);
    }
    CHECK(s == pl.singles.size() && d * 2 == pl.duals.size() && f * 2 == pl.flexes.size());
    // flex tasks: every (couple, pass) exactly once per chunk, pass-major
    CHECK(pl.flex_task_off.size() == pl.flexes.size() / 2 + 1);
    std::set<uint32_t> tasks(pl.flex_tasks.begin(), pl.flex_tasks.end());
    CHECK(tasks.size() == pl.flex_tasks.size());
    for (const auto& c : pl.chunks) {
        std::set<uint32_t> done;  // a task's predecessor (same couple, pass - 1) has an earlier ticket
        for (uint32_t k = pl.flex_task_off[c.fbegin]; k < pl.flex_task_off[c.fbegin + c.fcount]; ++k) {
            const uint32_t w = pl.flex_tasks[k] / 64, ps = pl.flex_tasks[k] % 64;
            CHECK(w >= c.fbegin && w < c.fbegin + c.fcount);
            if (ps) CHECK(done.count(pl.flex_tasks[k] - 1) == 1);
            done.insert(pl.flex_tasks[k]);
            CHECK(ps < pl.flex_task_off[w + 1] - pl.flex_task_off[w]);
        }
    }
    check_single_tasks(pl, chunk_bnd);
    // a pipelined plan is not fused, and its record regions are 8-byte aligned
    for (const auto& c : pl.chunks) {
        if (c.spasses < 2) continue;
        CHECK(!pl.fused);
        for (uint32_t w = c.sbegin; w < c.sbegin + c.scount; ++w) {
            const uint32_t x = pl.singles[w];
            if (pl.qlen[x] && pl.tlen[x] && ta::n_passes(pl.qlen[x]) > 1) CHECK(pl.bnd_off[x] % 2 == 0);
        }
    }
    for (size_t k = 0; k + 1 < pl.duals.size(); k += 2) {
        CHECK(pl.qlen[pl.duals[k]] == pl.qlen[pl.duals[k + 1]]);
        CHECK(pl.tlen[pl.duals[k]] == pl.tlen[pl.duals[k + 1]]);
        CHECK(ta::n_passes(pl.qlen[pl.duals[k]]) < 64);  // hand-off tags epoch * 64 + pass + 1 (ta_dual.hip)
    }
    for (size_t k = 0; k + 1 < pl.flexes.size(); k += 2) CHECK(ta::n_passes(pl.qlen[pl.flexes[k]]) < 64);
}

void check_affine(const ta::AffinePlan& pl) {
    const auto chunk_bnd = [](const ta::AffinePlan::Chunk& c) { return c.bnd_entries; };
    check_common(
        pl, pl.ws_ptr_entries, pl.ws_bnd_entries, [](const ta::AffinePlan::Chunk& c) { return c.ptr_entries; }, chunk_bnd,
        [&](uint32_t x) { return ta::ptr_dwords(pl.qlen[x], pl.tlen[x]); });
    for (size_t k = 0; k + 1 < pl.duals.size(); k += 2) CHECK(ta::n_passes(pl.qlen[pl.duals[k]]) < 64);
    check_single_tasks(pl, chunk_bnd);
}

void check_band(const ta::BandPlan& pl, uint32_t width) {
    check_common(
        pl, pl.ws_ptr_dwords, pl.ws_bnd_words, [](const ta::BandPlan::Chunk& c) { return c.ptr_dwords; },
        [](const ta::BandPlan::Chunk& c) { return c.bnd_words; },
        [&](uint32_t x) { return ta::band_ptr_dwords(pl.qlen[x], pl.tlen[x], pl.band[x]); });
    for (uint32_t p = 0; p < pl.n_pairs; ++p)
        CHECK(pl.band[p] == ta::band_clamp(pl.qlen[p], pl.tlen[p], width) && pl.band[p] <= width);
}

constexpr uint32_t kBandWidths[] = {0, 1, 37, 5000};  // (5000 clamps on most shapes below)

// One random batch and plan settings (the shapes of the planner and blocks modes).
struct Batch {
    std::vector<uint32_t> q, t;
    int type, ma, mi, g;
    uint64_t budget;
    uint32_t flags, quantum;
    bool cig;
};

Batch random_batch(uint64_t& s) {
    Batch b;
    std::vector<uint32_t>&q = b.q, &t = b.t;
    const int kind = (int)(splitmix(s) % 5);
    const uint32_t P = kind == 4 ? 2 + (uint32_t)(splitmix(s) % 3) : (uint32_t)(splitmix(s) % 300);
    q.resize(P);
    t.resize(P);
    for (uint32_t p = 0; p < P; ++p) {
        switch (kind) {
            case 0: q[p] = t[p] = 1000; break;                                                 // config 2
            case 1: q[p] = (uint32_t)(splitmix(s) % 3000); t[p] = (uint32_t)(splitmix(s) % 3000); break;  // ragged
            case 2: q[p] = 1 + (uint32_t)(splitmix(s) % 20000); t[p] = q[p] + (uint32_t)(splitmix(s) % 500); break;
            case 3: q[p] = (uint32_t)(splitmix(s) % 4) * 1024 + 7; t[p] = 300 + (uint32_t)(splitmix(s) % 3); break;
            default: q[p] = 63 * 1024 + 1 + (uint32_t)(splitmix(s) % 3) * 1024; t[p] = 40; break;  // 63..65 passes
        }
    }
    b.type = (int)(splitmix(s) % 3);
    // (kind 4: all-zero scoring, whose values fit int16 at any length: only the pass bound stops couples)
    b.ma = kind == 4 ? 0 : 1 + (int)(splitmix(s) % 3);
    b.mi = kind == 4 ? 0 : -(int)(splitmix(s) % 3);
    b.g = kind == 4 ? 0 : -(int)(splitmix(s) % 3);
    b.budget = (splitmix(s) & 1) ? (1ull << 40) : 4096ull + splitmix(s) % (64ull << 20);
    b.flags = (uint32_t)(splitmix(s) % 8) | ((splitmix(s) & 1) ? 32u : 0u) | ((splitmix(s) & 1) ? 64u : 0u);
    b.cig = splitmix(s) % 4 != 0;
    b.quantum = (splitmix(s) & 1) ? 1024u : (uint32_t)(splitmix(s) % 9);
    return b;
}

// The three families' plans of one batch, each handed to `check(plan, ...)`-style callbacks.
template <class Linear, class Affine, class Banded>
void plan_batch(const Batch& b, Linear on_linear, Affine on_affine, Banded on_banded) {
    const uint32_t P = (uint32_t)b.q.size();
    ta::Plan pl;
    ta::build_plan(pl, P, b.q.data(), b.t.data(), b.type, b.ma, b.mi, b.g, b.cig, b.budget, b.flags, b.quantum);
    on_linear(pl);
    ta::AffinePlan ap;
    ta::build_affine_plan(ap, P, b.q.data(), b.t.data(), b.type, b.ma, b.mi, -2, b.g, b.cig, b.budget, b.flags & 97u,
                          b.quantum);
    on_affine(ap);
    for (uint32_t w : kBandWidths) {
        const std::vector<uint32_t> band(P, w);
        ta::BandPlan bp;
        ta::build_band_plan(bp, P, b.q.data(), b.t.data(), band.data(), b.type, b.ma, b.mi, b.g, b.cig, b.budget);
        on_banded(bp, w);
    }
}

void plan_worker(uint64_t seed, int iters) {
    uint64_t s = seed;
    for (int it = 0; it < iters; ++it) {
        const Batch b = random_batch(s);
        plan_batch(
            b, [&](const ta::Plan& pl) { check_linear(pl, b.budget); }, [](const ta::AffinePlan& ap) { check_affine(ap); },
            [](const ta::BandPlan& bp, uint32_t w) { check_band(bp, w); });
    }
}

// ---- blocks mode: a plan's device block (ta_plan_block.h) against host buffers.
// Walks the bound block in list order, as the fourth visitor of the list: it
// checks what layout, pack and bind made of the list, not the list itself.
// That the list holds every member of the family's pointer struct, once each,
// rests on check_block's count of the listed entries against the struct's
// pointers and on its sweep for a pointer left unbound.
struct BlockChecker {
    const uint8_t* base;
    ta::BlockSpan span;
    const uint8_t* end;  // end of the previous region
    bool device_part = false;
    size_t entries = 0;
    void region(const void* ptr, uint64_t n) {
        const uint8_t* p = static_cast<const uint8_t*>(ptr);
        CHECK(reinterpret_cast<uintptr_t>(p) % 256 == 0);
        CHECK(p >= end);  // disjoint, in list order
        if (device_part) CHECK(p >= base + span.scratch);
        else CHECK(p + n <= base + span.upload);
        CHECK(p + n <= base + span.bytes);
        end = p + n;
        ++entries;
    }
    template <class T>
    void vec(T*& p, const std::vector<T>& v) {
        region(p, ta::vbytes(v));
        if (!v.empty()) CHECK(std::memcmp(p, v.data(), ta::vbytes(v)) == 0);
    }
    template <class P>
    void zeros(P*& p, uint64_t n) {
        region(p, n);
        const uint8_t* z = reinterpret_cast<const uint8_t*>(p);
        for (uint64_t k = 0; k < n; ++k) CHECK(z[k] == 0);
    }
    void device_only() {
        CHECK(uint64_t(end - base) <= span.upload && span.upload - uint64_t(end - base) < 256);
        device_part = true;
    }
    template <class P>
    void scratch(P*& p, uint64_t n) {
        region(p, n);
    }
};

// D: the family's device-array struct (pointers only).
template <class D, class H>
void check_block(const H& h, uint64_t between) {
    D d;
    const ta::BlockSpan span = ta::layout_block(h, d, between);
    CHECK(span.upload % 256 == 0 && span.scratch == span.upload + between && span.bytes >= span.scratch);
    // pack into a buffer of the uploaded part, "upload" it into the whole block, bind there
    std::vector<uint8_t> up(span.upload, 0xA5);
    ta::pack_block(h, d, up.data());
    uint8_t* blk = static_cast<uint8_t*>(std::aligned_alloc(256, std::max<uint64_t>(span.bytes, 256)));
    std::memset(blk, 0x5A, std::max<uint64_t>(span.bytes, 256));
    if (span.upload) std::memcpy(blk, up.data(), span.upload);
    ta::bind_block(h, d, blk, span);
    void* ptrs[sizeof(D) / sizeof(void*)];  // no member left unbound
    static_assert(sizeof(D) % sizeof(void*) == 0, "device arrays: pointers only");
    std::memcpy(ptrs, &d, sizeof(D));
    for (void* p : ptrs) CHECK(p >= (void*)blk && p <= (void*)(blk + span.bytes));
    BlockChecker v{blk, span, blk};
    ta::block_arrays(h, d, v);
    CHECK(v.device_part);
    CHECK(v.entries == sizeof(D) / sizeof(void*));  // every member listed (one listed twice leaves another unbound, for the sweep above)
    CHECK(((uint64_t(v.end - blk) + 255) & ~uint64_t(255)) == span.bytes);  // the total ends the last region
    std::free(blk);
}

int run_blocks(uint64_t seed, int iters) {
    uint64_t s = seed;
    uint64_t blocks = 0;
    for (int it = 0; it < iters; ++it) {
        const Batch b = random_batch(s);
        const uint64_t between = (it & 1) ? 0 : 256 * (1 + splitmix(s) % 5);  // (a host batch's own inputs)
        plan_batch(
            b, [&](const ta::Plan& pl) { check_block<ta::PlanArrays>(pl, between), ++blocks; },
            [&](const ta::AffinePlan& ap) { check_block<ta::AffineArrays>(ap, between), ++blocks; },
            [&](const ta::BandPlan& bp, uint32_t) { check_block<ta::BandArrays>(bp, between), ++blocks; });
    }
    std::printf("blocks %llu fails %d\n", (unsigned long long)blocks, fails);
    return fails ? 1 : 0;
}

// Small host batches (the drop-in call's combined batches, ta_align_batch)
// plan as ONE chunk under their own budget (ta_host_batch.h batch_budget), in
// both code layouts.
void check_small_batches() {
    const uint32_t shapes[][2] = {{1000, 1000}, {200, 200}, {5, 9}, {1000, 700}, {3000, 2500}};
    for (const auto& sh : shapes)
        for (uint32_t P : {1u, 2u, 3u, 8u, 16u, 33u})
            for (int type = 0; type < 3; ++type)
                for (uint32_t flags : {0u, 128u, 256u, 512u}) {  // TA_PLAN_NO_BLK, TA_PLAN_NO_CK, TA_PLAN_CK
                    std::vector<uint32_t> q(P, sh[0]), t(P, sh[1]);
                    const uint64_t budget = std::max<uint64_t>(ta::host_batch_code_bytes(P, q.data(), t.data(), 4), 1);
                    ta::Plan pl;
                    ta::build_plan(pl, P, q.data(), t.data(), type, 1, -1, -1, true, budget, flags, 1024);
                    check_linear(pl, budget);
                    CHECK(pl.chunks.size() == 1);
                    if (pl.chunks.size() != 1)
                        std::printf("small batch %u x %ux%u type %d flags %u: %zu chunks\n", P, sh[0], sh[1], type, flags,
                                    pl.chunks.size());
                    // every pair in the packed kernels (an odd one coupled with itself) when it fits
                    // int16 and is not tiny (or TA_PLAN_CK); band walks (blocked layout) from 8 local pairs up
                    // under TA_PLAN_NO_CK
                    const bool packed = ((uint64_t)sh[0] * sh[1] >= 4096 || flags == 512u) &&
                                        ta::fits_int16(type, sh[0], sh[1], 1, -1, -1);
                    // (n_dual_pairs counts two per couple, a self-coupled pair included)
                    if (packed) CHECK(pl.singles.empty() && pl.n_dual_pairs == 2 * ((P + 1) / 2));
                    // (tiny pairs of an even batch still couple with each other; only a lone one stays int32)
                    const bool all_packed = ta::fits_int16(type, sh[0], sh[1], 1, -1, -1) && (packed || P % 2 == 0);
                    // global / semi: checkpoints (blocked region sizes) whenever they are taken
                    const bool edge_ck = all_packed && type != ta::kLocal && flags == 512u;
                    // pairs past int16 in the dual kernel: flexible couples (self-coupled when alone),
                    // with checkpoints under TA_PLAN_CK when their H fits (ta_planner.cpp flex_ck_fits)
                    const bool flex_ck = flags == 512u && !ta::fits_int16(type, sh[0], sh[1], 1, -1, -1) &&
                                         ta::flex_ck_fits(type, sh[0], sh[1], 1, -1, -1);
                    // local: blocked codes only under TA_PLAN_NO_CK, or with checkpoints (TA_PLAN_CK)
                    CHECK(pl.blk == ((all_packed && type == ta::kLocal && P >= 8 && (flags == 256u || flags == 512u) &&
                                      sh[0] + sh[1] <= 6000) ||
                                     edge_ck || flex_ck));
                    // checkpoints and recomputing walks: small batches only with TA_PLAN_CK (gap -1 <= 0)
                    CHECK(pl.ck == (pl.blk && flags == 512u));
                    if (pl.ck) CHECK(pl.walk_group == 64);
                }
}

int run_planner(uint64_t seed, int iters, int threads) {
    check_small_batches();
    std::vector<std::thread> th;
    for (int w = 0; w < threads; ++w) th.emplace_back(plan_worker, seed + (uint64_t)w * 7919, iters);
    for (auto& x : th) x.join();
    std::printf("planner iters %d threads %d fails %d\n", iters, threads, fails);
    return fails ? 1 : 0;
}

int run_fastx(const char* path, bool fastq) {
    tmap::FastxFile f;
    std::string err;
    if (!tmap::read_fastx(path, fastq, f, err)) {
        std::printf("fastx error %s\n", err.c_str());
        return 0;  // a wrong-format read is a clean failure, not a sanitizer finding
    }
    uint64_t h = 1469598103934665603ull;
    for (const auto& r : f.records) {
        CHECK(r.off + r.len <= f.seq.size());
        for (char c : r.name) h = (h ^ (uint8_t)c) * 1099511628211ull;
        h = (h ^ r.len) * 1099511628211ull;
    }
    std::printf("fastx records %zu bases %zu hash %llx\n", f.records.size(), f.seq.size(), (unsigned long long)h);
    return fails ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "oracle") == 0) return run_oracle(argv[2]);
    if (argc >= 5 && std::strcmp(argv[1], "planner") == 0)
        return run_planner(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]), std::atoi(argv[4]));
    if (argc >= 4 && std::strcmp(argv[1], "blocks") == 0)
        return run_blocks(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 4 && std::strcmp(argv[1], "fastx") == 0) return run_fastx(argv[2], std::atoi(argv[3]) != 0);
    std::fprintf(stderr, "usage: %s oracle CASES | planner SEED N THREADS | blocks SEED N | fastx PATH FASTQ\n", argv[0]);
    return 2;
}
