// bioinfo1_amd/csrc/tm_api.cpp -- host side of the mapper ABI
// (include/team_mapper_c.h): contexts, the reference minimizer index, the
// batched mapper (minimizers -> seed hits -> FindLIS chains -> one
// team_alignment batch plan) and the file-level driver that writes the
// reference's PAF-like lines.  The per-read work runs in the HIP stages
// (tm_minimizers.hip, tm_match.hip, tm_chain.hip, libteam_alignment).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "ta_layout.h"
#include "tm_fastx.h"
#include "tm_internal.h"
#include "tm_match.h"
#include "tm_stitch.h"

struct tm_index {
    tm_context* ctx = nullptr;
    std::string name;
    uint64_t len = 0;
    uint32_t k = 0, w = 0;
    tmap::DevBuf ref2;  // [forward | reverse complement], 2*len bytes
    struct Strand {
        tmap::DevBuf keys, koff, pos;
        uint32_t n_keys = 0;
        uint64_t n_pos = 0;
        uint32_t banned = 0;
        tmap::DevIndexView view() const {
            return {keys.as<uint32_t>(), koff.as<uint32_t>(), pos.as<uint32_t>(), n_keys};
        }
    } fwd, rev;
};

namespace {

using tmap::fail;

bool valid_kw(uint32_t k, uint32_t w) { return k >= 1 && k <= tmap::kMaxK && w >= 1 && w <= tmap::kMaxW; }

// team_mapper.cpp:432-446: hashes by descending frequency.  std::sort over the
// unordered_map's iteration order, with the map built by the same sequence of
// operator[] increments as the reference (KMER::Minimize, team_minimizers.cpp
// :160-167/190-196/214-220), so equal counts fall in the same order.
std::vector<std::pair<unsigned int, int>> ranked(const uint32_t* hashes, uint64_t n) {
    std::unordered_map<unsigned int, int> freq;
    for (uint64_t i = 0; i < n; ++i) freq[hashes[i]]++;
    std::vector<std::pair<unsigned int, int>> v(freq.begin(), freq.end());
    std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.second > b.second; });
    return v;
}

// CSR over the surviving (hash, position) pairs of one strand (the
// unordered_map<hash, set<(pos, strand)>> of team_mapper.cpp:449-471).
int build_strand(tm_context* ctx, tm_index::Strand& st, const uint32_t* h, const uint32_t* p, uint64_t n,
                 const std::unordered_set<unsigned int>& ban) {
    std::vector<uint64_t> kv;
    kv.reserve(n);
    for (uint64_t i = 0; i < n; ++i)
        if (!ban.count(h[i])) kv.push_back(((uint64_t)h[i] << 32) | p[i]);
    std::sort(kv.begin(), kv.end());
    kv.erase(std::unique(kv.begin(), kv.end()), kv.end());
    std::vector<uint32_t> keys, koff, pos(kv.size());
    for (size_t i = 0; i < kv.size(); ++i) {
        const uint32_t hh = (uint32_t)(kv[i] >> 32);
        if (keys.empty() || keys.back() != hh) {
            keys.push_back(hh);
            koff.push_back((uint32_t)i);
        }
        pos[i] = (uint32_t)kv[i];
    }
    koff.push_back((uint32_t)kv.size());
    st.n_keys = (uint32_t)keys.size();
    st.n_pos = kv.size();
    st.banned = (uint32_t)ban.size();
    hipStream_t s = ctx->stream;
    TM_HIP(ctx, st.keys.reserve(keys.size() * 4 + 4));
    TM_HIP(ctx, st.koff.reserve(koff.size() * 4 + 4));
    TM_HIP(ctx, st.pos.reserve(pos.size() * 4 + 4));
    if (!keys.empty()) TM_HIP(ctx, hipMemcpyAsync(st.keys.p, keys.data(), keys.size() * 4, hipMemcpyHostToDevice, s));
    TM_HIP(ctx, hipMemcpyAsync(st.koff.p, koff.data(), koff.size() * 4, hipMemcpyHostToDevice, s));
    if (!pos.empty()) TM_HIP(ctx, hipMemcpyAsync(st.pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, s));
    TM_HIP(ctx, hipStreamSynchronize(s));
    return TM_OK;
}

}  // namespace

extern "C" {

const char* tm_status_string(int status) {
    switch (status) {
        case TM_OK: return "ok";
        case TM_ERR_BAD_TYPE: return "Unknown AlignmentType provided.";
        case TM_ERR_ARG: return "invalid argument";
        case TM_ERR_DEVICE: return "device error";
        case TM_ERR_CAPACITY: return "output buffer too small";
        case TM_ERR_INPUT: return "Given file is not in FASTA or FASTQ format!";
        default: return "unknown status";
    }
}

const char* tm_last_error(const tm_context* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int tm_context_create(int device, tm_context** out) {
    if (!out) return TM_ERR_ARG;
    *out = nullptr;
    ta_context* ta = nullptr;
    if (int r = ta_context_create(device, &ta)) return r == TA_ERR_DEVICE ? TM_ERR_DEVICE : TM_ERR_ARG;
    auto* c = new tm_context();
    c->device = device;
    c->ta = ta;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        tm_context_destroy(c);
        return TM_ERR_DEVICE;
    }
    *out = c;
    return TM_OK;
}

void tm_context_destroy(tm_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    tmap::MinimizerOut& m = c->mins;
    for (tmap::DevBuf* b : {&c->bytes, &c->off, &c->len, &m.entry_off, &m.tiles, &m.hash, &m.pos, &m.keep, &m.scan,
                          &m.kept_off, &m.khash, &m.kpos, &m.cub_tmp, &c->c_off, &c->c_f, &c->c_r, &c->c_out,
                          &c->c_prev, &c->c_lis, &c->m_qoff, &c->m_toff, &c->m_score, &c->m_tb, &c->m_slots,
                          &c->m_cstart, &c->m_clen, &c->m_coff, &c->m_cdst, &c->m_eslots, &c->m_estart, &c->m_elen, &c->m_info, &c->m_exact, &c->m_need, &c->e_qoff, &c->e_toff, &c->e_score, &c->e_tb, &c->e_slots, &c->e_cstart, &c->e_clen,
                          &c->e_qend, &c->e_tend, &c->e_meta, &c->e_rev, &c->match.cnt_f, &c->match.cnt_r, &c->match.off_f,
                          &c->match.off_r, &c->match.key_f, &c->match.key_r, &c->match.hf, &c->match.hr,
                          &c->match.list_off, &c->match.cub_tmp})
        b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    ta_context_destroy(c->ta);
    delete c;
}

int tm_index_create(tm_context* ctx, const char* name, const char* seq, uint64_t len, uint32_t k, uint32_t w, double f,
                    tm_index** out) {
    if (!ctx || !out || (len && !seq)) return TM_ERR_ARG;
    *out = nullptr;
    if (!valid_kw(k, w)) return fail(ctx, TM_ERR_ARG, "unsupported k or w");
    if (len >= (1ull << 31)) return fail(ctx, TM_ERR_ARG, "reference longer than 2^31 bases");
    TM_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    auto* idx = new tm_index();
    idx->ctx = ctx;
    idx->name = name ? name : "";
    idx->len = len;
    idx->k = k;
    idx->w = w;
    auto bail = [&](int r) {
        tm_index_destroy(idx);
        return r;
    };
    if (idx->ref2.reserve(2 * len + 1) != hipSuccess) return bail(fail(ctx, TM_ERR_DEVICE, "hipMalloc reference"));
    if (len && (hipMemcpyAsync(idx->ref2.p, seq, len, hipMemcpyHostToDevice, s) != hipSuccess ||
                tmap::launch_revcomp(idx->ref2.as<uint8_t>(), idx->ref2.as<uint8_t>() + len, len, s) != hipSuccess))
        return bail(fail(ctx, TM_ERR_DEVICE, "reference upload / reverse complement"));
    // both strands' minimizers in one batch (team_mapper.cpp:413-427)
    const uint64_t h_off[2] = {0, len};
    const uint32_t h_len[2] = {(uint32_t)len, (uint32_t)len};
    if (ctx->off.reserve(16) != hipSuccess || ctx->len.reserve(8) != hipSuccess ||
        hipMemcpyAsync(ctx->off.p, h_off, 16, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(ctx->len.p, h_len, 8, hipMemcpyHostToDevice, s) != hipSuccess)
        return bail(fail(ctx, TM_ERR_DEVICE, "index staging"));
    tmap::MinimizerOut& mo = ctx->mins;
    if (int r = tmap::minimize_device(ctx, 2, idx->ref2.as<uint8_t>(), ctx->off.as<uint64_t>(), ctx->len.as<uint32_t>(),
                                    h_len, k, w, true, mo))
        return bail(r);
    std::vector<uint32_t> full(mo.total), kh(mo.kept), kp(mo.kept);
    uint64_t kept_off[3] = {0, 0, 0};
    bool ok = (mo.total == 0 || hipMemcpyAsync(full.data(), mo.hash.p, mo.total * 4, hipMemcpyDeviceToHost, s) == hipSuccess) &&
              (mo.kept == 0 || (hipMemcpyAsync(kh.data(), mo.khash.p, mo.kept * 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
                                hipMemcpyAsync(kp.data(), mo.kpos.p, mo.kept * 4, hipMemcpyDeviceToHost, s) == hipSuccess)) &&
              hipMemcpyAsync(kept_off, mo.kept_off.p, 24, hipMemcpyDeviceToHost, s) == hipSuccess &&
              hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return bail(fail(ctx, TM_ERR_DEVICE, "index download"));
    const uint64_t ef = mo.h_entry_off[1];
    // frequency ranking per strand; both thresholds use the reverse strand's
    // unique count (the reference's GetUniqueMinimizers reads a namespace-level
    // set that the reverse Minimize call refilled last, team_mapper.cpp:431-432)
    const std::vector<std::pair<unsigned int, int>> vf = ranked(full.data(), ef);
    const std::vector<std::pair<unsigned int, int>> vr = ranked(full.data() + ef, mo.total - ef);
    const uint64_t uniq_rev = kept_off[2] - kept_off[1];
    const int thr = static_cast<int>(f * (double)uniq_rev);
    std::unordered_set<unsigned int> ban_f, ban_r;
    for (int i = 0; i < std::min(thr, (int)vf.size()); ++i) ban_f.insert(vf[i].first);
    // the reverse ban list is taken from the FORWARD ranking (team_mapper.cpp:463-465)
    for (int i = 0; i < std::min(std::min(thr, (int)vr.size()), (int)vf.size()); ++i) ban_r.insert(vf[i].first);
    if (int r = build_strand(ctx, idx->fwd, kh.data(), kp.data(), kept_off[1], ban_f)) return bail(r);
    if (int r = build_strand(ctx, idx->rev, kh.data() + kept_off[1], kp.data() + kept_off[1], kept_off[2] - kept_off[1],
                             ban_r))
        return bail(r);
    *out = idx;
    return TM_OK;
}

void tm_index_destroy(tm_index* idx) {
    if (!idx) return;
    (void)hipSetDevice(idx->ctx->device);
    for (tmap::DevBuf* b : {&idx->ref2, &idx->fwd.keys, &idx->fwd.koff, &idx->fwd.pos, &idx->rev.keys, &idx->rev.koff,
                          &idx->rev.pos})
        b->release();
    delete idx;
}

int tm_index_stats(const tm_index* idx, uint64_t* fk, uint64_t* rk, uint64_t* fp, uint64_t* rp, uint32_t* bf,
                   uint32_t* br) {
    if (!idx) return TM_ERR_ARG;
    if (fk) *fk = idx->fwd.n_keys;
    if (rk) *rk = idx->rev.n_keys;
    if (fp) *fp = idx->fwd.n_pos;
    if (rp) *rp = idx->rev.n_pos;
    if (bf) *bf = idx->fwd.banned;
    if (br) *br = idx->rev.banned;
    return TM_OK;
}

int tm_map_batch(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes, const uint64_t* off,
                 const uint32_t* len, const tm_options* opt, uint8_t* mapped, uint8_t* strand_fwd, uint32_t* q_begin,
                 uint32_t* q_end, uint32_t* t_begin, uint32_t* t_end, int32_t* score, char* arena,
                 uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len) {
    return tm_map_batch_x(ctx, idx, n_reads, bytes, off, len, opt, mapped, strand_fwd, q_begin, q_end, t_begin, t_end,
                          score, arena, arena_bytes, cigar_off, cigar_len, 0, nullptr);
}

// band: null = no band, the reference-exact ta_plan_*; else every window's band (ta_banded_plan_*).
// gap_open (with a band only): affine gaps, gap_extend = opt->gap (ta_banded_affine_plan_*).
// band_auto (band is then not read): every window at the start band of ta_layout.h
// band_exact_default_start, certified, and the uncertified windows once more in a
// second plan at their needed band -- the unbanded results (team_align_c.h).
// extend_ends (a numeric band, global type, no TM_MAP_EQX): each window is then extended
// to the read's ends by two anchored alignments and the three CIGARs are stitched.
static int map_batch_impl(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes,
                          const uint64_t* off, const uint32_t* len, const tm_options* opt, uint8_t* mapped,
                          uint8_t* strand_fwd, uint32_t* q_begin, uint32_t* q_end, uint32_t* t_begin, uint32_t* t_end,
                          int32_t* score, char* arena, uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len,
                          uint32_t flags, ta_pair_info* info, const uint32_t* band, const int* gap_open = nullptr,
                          bool band_auto = false, bool extend_ends = false, int32_t zdrop = -1,
                          int zdrop_rule = TA_ZDROP_SEGMENT);

int tm_map_batch_x(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes, const uint64_t* off,
                   const uint32_t* len, const tm_options* opt, uint8_t* mapped, uint8_t* strand_fwd, uint32_t* q_begin,
                   uint32_t* q_end, uint32_t* t_begin, uint32_t* t_end, int32_t* score, char* arena,
                   uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len, uint32_t flags, ta_pair_info* info) {
    return map_batch_impl(ctx, idx, n_reads, bytes, off, len, opt, mapped, strand_fwd, q_begin, q_end, t_begin, t_end,
                          score, arena, arena_bytes, cigar_off, cigar_len, flags, info, nullptr);
}

int tm_map_batch_band(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes, const uint64_t* off,
                      const uint32_t* len, const tm_options* opt, uint8_t* mapped, uint8_t* strand_fwd,
                      uint32_t* q_begin, uint32_t* q_end, uint32_t* t_begin, uint32_t* t_end, int32_t* score,
                      char* arena, uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len, uint32_t flags,
                      ta_pair_info* info, uint32_t band) {
    return map_batch_impl(ctx, idx, n_reads, bytes, off, len, opt, mapped, strand_fwd, q_begin, q_end, t_begin, t_end,
                          score, arena, arena_bytes, cigar_off, cigar_len, flags, info, &band);
}

int tm_map_batch_band_affine(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes,
                             const uint64_t* off, const uint32_t* len, const tm_options* opt, uint8_t* mapped,
                             uint8_t* strand_fwd, uint32_t* q_begin, uint32_t* q_end, uint32_t* t_begin,
                             uint32_t* t_end, int32_t* score, char* arena, uint64_t arena_bytes, uint64_t* cigar_off,
                             uint32_t* cigar_len, uint32_t flags, ta_pair_info* info, uint32_t band, int gap_open) {
    return map_batch_impl(ctx, idx, n_reads, bytes, off, len, opt, mapped, strand_fwd, q_begin, q_end, t_begin, t_end,
                          score, arena, arena_bytes, cigar_off, cigar_len, flags, info, &band, &gap_open);
}

uint64_t tm_ends_arena_extra(uint32_t len, uint32_t band) {
    const uint64_t cap = 3ull * len + 6;
    return 4ull * (band < cap ? band : cap) + 4;
}

int tm_map_batch_band_ends(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes,
                           const uint64_t* off, const uint32_t* len, const tm_options* opt, uint8_t* mapped,
                           uint8_t* strand_fwd, uint32_t* q_begin, uint32_t* q_end, uint32_t* t_begin, uint32_t* t_end,
                           int32_t* score, char* arena, uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len,
                           uint32_t flags, ta_pair_info* info, uint32_t band, const int* gap_open) {
    return tm_map_batch_band_ends_zdrop(ctx, idx, n_reads, bytes, off, len, opt, mapped, strand_fwd, q_begin, q_end,
                                        t_begin, t_end, score, arena, arena_bytes, cigar_off, cigar_len, flags, info,
                                        band, gap_open, -1);
}

int tm_map_batch_band_ends_zdrop(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes,
                                 const uint64_t* off, const uint32_t* len, const tm_options* opt, uint8_t* mapped,
                                 uint8_t* strand_fwd, uint32_t* q_begin, uint32_t* q_end, uint32_t* t_begin,
                                 uint32_t* t_end, int32_t* score, char* arena, uint64_t arena_bytes,
                                 uint64_t* cigar_off, uint32_t* cigar_len, uint32_t flags, ta_pair_info* info,
                                 uint32_t band, const int* gap_open, int32_t zdrop) {
    return tm_map_batch_band_ends_zdrop_rule(ctx, idx, n_reads, bytes, off, len, opt, mapped, strand_fwd, q_begin,
                                             q_end, t_begin, t_end, score, arena, arena_bytes, cigar_off, cigar_len,
                                             flags, info, band, gap_open, zdrop, TA_ZDROP_SEGMENT);
}

int tm_map_batch_band_ends_zdrop_rule(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes,
                                      const uint64_t* off, const uint32_t* len, const tm_options* opt, uint8_t* mapped,
                                      uint8_t* strand_fwd, uint32_t* q_begin, uint32_t* q_end, uint32_t* t_begin,
                                      uint32_t* t_end, int32_t* score, char* arena, uint64_t arena_bytes,
                                      uint64_t* cigar_off, uint32_t* cigar_len, uint32_t flags, ta_pair_info* info,
                                      uint32_t band, const int* gap_open, int32_t zdrop, int zdrop_rule) {
    return map_batch_impl(ctx, idx, n_reads, bytes, off, len, opt, mapped, strand_fwd, q_begin, q_end, t_begin, t_end,
                          score, arena, arena_bytes, cigar_off, cigar_len, flags, info, &band, gap_open, false, true,
                          zdrop, zdrop_rule);
}

int tm_map_batch_band_exact(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes,
                            const uint64_t* off, const uint32_t* len, const tm_options* opt, uint8_t* mapped,
                            uint8_t* strand_fwd, uint32_t* q_begin, uint32_t* q_end, uint32_t* t_begin,
                            uint32_t* t_end, int32_t* score, char* arena, uint64_t arena_bytes, uint64_t* cigar_off,
                            uint32_t* cigar_len, uint32_t flags, ta_pair_info* info, const int* gap_open) {
    const uint32_t none = 0;
    return map_batch_impl(ctx, idx, n_reads, bytes, off, len, opt, mapped, strand_fwd, q_begin, q_end, t_begin, t_end,
                          score, arena, arena_bytes, cigar_off, cigar_len, flags, info, &none, gap_open, true);
}

static int map_batch_impl(tm_context* ctx, const tm_index* idx, uint32_t n_reads, const char* bytes,
                          const uint64_t* off, const uint32_t* len, const tm_options* opt, uint8_t* mapped,
                          uint8_t* strand_fwd, uint32_t* q_begin, uint32_t* q_end, uint32_t* t_begin, uint32_t* t_end,
                          int32_t* score, char* arena, uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len,
                          uint32_t flags, ta_pair_info* info, const uint32_t* band, const int* gap_open,
                          bool band_auto, bool extend_ends, int32_t zdrop, int zdrop_rule) {
    if (!ctx || !idx || !opt) return TM_ERR_ARG;
    if (zdrop >= 0 && !extend_ends) return fail(ctx, TM_ERR_ARG, "--zdrop needs --extend-ends");
    if (zdrop_rule != TA_ZDROP_SEGMENT && zdrop_rule != TA_ZDROP_STRIPE)
        return fail(ctx, TM_ERR_ARG, "unknown z-drop rule");
    if (flags & ~TM_MAP_EQX) return fail(ctx, TM_ERR_ARG, "unknown flag");
    if (info && !(flags & TM_MAP_EQX)) return fail(ctx, TM_ERR_ARG, "info needs TM_MAP_EQX");
    const bool eqx = (flags & TM_MAP_EQX) != 0;
    if (extend_ends) {  // (the annotate records of the three pieces are not stitched)
        if (!band || band_auto) return fail(ctx, TM_ERR_ARG, "--extend-ends needs a numeric band");
        if (opt->type != TA_GLOBAL) return fail(ctx, TM_ERR_ARG, "--extend-ends needs the global alignment type");
        if (eqx) return fail(ctx, TM_ERR_ARG, "--extend-ends cannot be combined with TM_MAP_EQX");
    }
    if (opt->type != TA_GLOBAL && opt->type != TA_LOCAL && opt->type != TA_SEMI_GLOBAL)
        return fail(ctx, TM_ERR_BAD_TYPE, tm_status_string(TM_ERR_BAD_TYPE));
    if (opt->k != idx->k || opt->w != idx->w) return fail(ctx, TM_ERR_ARG, "k/w differ from the index");
    if (!n_reads) return TM_OK;
    if (!off || !len || !mapped || !strand_fwd || !q_begin || !q_end || !t_begin || !t_end || !score)
        return fail(ctx, TM_ERR_ARG, "null argument");
    if (opt->want_cigar && (!arena || !cigar_off || !cigar_len)) return fail(ctx, TM_ERR_ARG, "null cigar output");
    TM_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    uint64_t nbytes = 0;
    for (uint32_t r = 0; r < n_reads; ++r) nbytes = std::max<uint64_t>(nbytes, off[r] + len[r]);
    TM_HIP(ctx, ctx->bytes.reserve(nbytes + 1));
    TM_HIP(ctx, ctx->off.reserve(n_reads * 8ull));
    TM_HIP(ctx, ctx->len.reserve(n_reads * 4ull));
    using clk = std::chrono::steady_clock;
    auto t_last = clk::now();
    const auto t_first = t_last;
    std::fill(ctx->stage_ms, ctx->stage_ms + tmap::kStages, 0.0);
    auto stage = [&](int i) -> int {  // close stage i (the stream is drained so host time = device time)
        TM_HIP(ctx, hipStreamSynchronize(s));
        const auto t = clk::now();
        ctx->stage_ms[i] = std::chrono::duration<double, std::milli>(t - t_last).count();
        ctx->stage_ms[tmap::kStages - 1] = std::chrono::duration<double, std::milli>(t - t_first).count();
        t_last = t;
        return TM_OK;
    };
    auto stage_add = [&](int i) -> int {  // ... or add to it (a stage that runs in two parts)
        const double before = ctx->stage_ms[i];
        if (int r = stage(i)) return r;
        ctx->stage_ms[i] += before;
        return TM_OK;
    };
    if (nbytes) TM_HIP(ctx, hipMemcpyAsync(ctx->bytes.p, bytes, nbytes, hipMemcpyHostToDevice, s));
    TM_HIP(ctx, hipMemcpyAsync(ctx->off.p, off, n_reads * 8ull, hipMemcpyHostToDevice, s));
    TM_HIP(ctx, hipMemcpyAsync(ctx->len.p, len, n_reads * 4ull, hipMemcpyHostToDevice, s));
    if (int r = stage(0)) return r;
    // 1. read minimizers, first occurrences only (team_mapper.cpp:611-612, 713-714)
    tmap::MinimizerOut& mo = ctx->mins;
    if (int r = tmap::minimize_device(ctx, n_reads, ctx->bytes.as<uint8_t>(), ctx->off.as<uint64_t>(),
                                    ctx->len.as<uint32_t>(), len, opt->k, opt->w, true, mo))
        return r;
    if (int r = stage(1)) return r;
    // 2. seed hits on both strands
    tmap::MatchOut& mt = ctx->match;
    if (int r = tmap::match_device(ctx, n_reads, mo, idx->fwd.view(), idx->rev.view(), opt->fastq_rules, mt)) return r;
    if (int r = stage(2)) return r;
    // 3. FindLIS per (read, strand)
    const uint32_t n_lists = 2 * n_reads;
    TM_HIP(ctx, ctx->c_out.reserve(n_lists * 20ull));
    if (int r = tmap::chain_device(ctx, n_lists, mt.list_off.as<uint64_t>(), mt.tot_f + mt.tot_r, mt.hf.as<uint32_t>(),
                                 mt.hr.as<uint32_t>(), ctx->c_out.as<uint32_t>()))
        return r;
    std::vector<uint32_t> ch(5ull * n_lists);
    TM_HIP(ctx, hipMemcpyAsync(ch.data(), ctx->c_out.p, n_lists * 20ull, hipMemcpyDeviceToHost, s));
    TM_HIP(ctx, hipStreamSynchronize(s));
    if (int r = stage(3)) return r;
    // 4. windows (team_mapper.cpp:650-663)
    const uint32_t k = opt->k;
    std::vector<uint32_t> pair_read, ql, tl;
    std::vector<uint64_t> qo, to;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint32_t* cf = &ch[5ull * r];
        const uint32_t* cr = &ch[5ull * (n_reads + r)];
        const bool fwd = cf[0] >= cr[0];
        const uint32_t* c = fwd ? cf : cr;
        mapped[r] = c[0] != 0;
        strand_fwd[r] = fwd;
        score[r] = 0;
        if (opt->want_cigar) cigar_len[r] = 0;
        if (info) info[r] = ta_pair_info{};
        if (!c[0]) {
            q_begin[r] = q_end[r] = t_begin[r] = t_end[r] = 0;
            continue;
        }
        q_begin[r] = c[1] - 1;
        q_end[r] = c[3] + k - 2;
        t_begin[r] = c[2] - 1;
        t_end[r] = c[4] + k - 2;
        pair_read.push_back(r);
        ql.push_back(q_end[r] - q_begin[r] + 1);
        tl.push_back(t_end[r] - t_begin[r] + 1);
        qo.push_back(off[r] + q_begin[r]);
        to.push_back((fwd ? 0 : idx->len) + t_begin[r]);
    }
    // 5. one alignment batch over all windows (libteam_alignment plan, device-resident)
    uint32_t P = (uint32_t)pair_read.size();  // (band auto: the pairs of the round that runs)
    if (!P) return TM_OK;
    ta_plan* plan = nullptr;
    ta_banded_plan* bplan = nullptr;  // with a band: the banded family instead (the same band for every window)
    ta_banded_affine_plan* aplan = nullptr;  // with a band and a gap open: the banded affine family
    // the mapper owns the device: its code workspace may take most of the free
    // HBM (fewer, fuller chunks for long reads; the library default is half,
    // <= 64 GiB).  Memory the alignment context already holds from the last
    // batch is reused, so it counts as free.
    size_t free_b = 0, total_b = 0;
    const uint64_t budget = hipMemGetInfo(&free_b, &total_b) == hipSuccess
                                ? ((uint64_t)free_b + ta_context_held_bytes(ctx->ta)) / 100 * 85
                                : 0;
    // band auto: what a round leaves on the host instead of the caller's arrays
    struct Round {
        std::vector<int32_t> sc;
        std::vector<ta_pair_info> pinfo;
        std::vector<uint64_t> co;  // P + 1 offsets into cig
        std::vector<char> cig;
        std::vector<uint8_t> exact;
        std::vector<uint32_t> need;
    };
    std::vector<uint32_t> bw;  // the bands of the round that runs
    if (band) bw.assign(P, *band);
    if (band_auto)
        for (uint32_t p = 0; p < P; ++p) bw[p] = ta::band_exact_default_start(ql[p], tl[p]);
    int rc;
    auto create = [&]() -> int {  // the banded plan of either gap family over P, ql, tl, bw
        return gap_open ? ta_banded_affine_plan_create(ctx->ta, P, ql.data(), tl.data(), bw.data(), opt->type, opt->match,
                                                       opt->mismatch, *gap_open, opt->gap, opt->want_cigar || eqx,
                                                       budget, 0, &aplan)
                        : ta_banded_plan_create(ctx->ta, P, ql.data(), tl.data(), bw.data(), opt->type, opt->match,
                                                opt->mismatch, opt->gap, opt->want_cigar || eqx, budget, 0, &bplan);
    };
    if (band) {
        rc = create();
    } else {
        rc = ta_plan_create(ctx->ta, P, ql.data(), tl.data(), opt->type, opt->match, opt->mismatch, opt->gap,
                            opt->want_cigar || eqx, budget, 0, &plan);  // the annotate pass reads the CIGARs
    }
    if (rc != TA_OK) return fail(ctx, rc == TA_ERR_BAD_TYPE ? TM_ERR_BAD_TYPE : TM_ERR_DEVICE,
                                 std::string("ta_plan_create: ") + ta_last_error(ctx->ta));
    uint64_t slots = aplan   ? ta_banded_affine_plan_cigar_slots_bytes(aplan)
                     : bplan ? ta_banded_plan_cigar_slots_bytes(bplan)
                             : ta_plan_cigar_slots_bytes(plan);
    // out: null = the results go to the caller's arrays; else (band auto) a round's results and certificate
    auto run = [&](Round* out) -> int {
        TM_HIP(ctx, ctx->m_qoff.reserve(P * 8ull));
        TM_HIP(ctx, ctx->m_toff.reserve(P * 8ull));
        TM_HIP(ctx, ctx->m_score.reserve(P * 4ull));
        TM_HIP(ctx, ctx->m_tb.reserve(P * 4ull));
        TM_HIP(ctx, ctx->m_cstart.reserve(P * 8ull));
        TM_HIP(ctx, ctx->m_clen.reserve(P * 4ull));
        TM_HIP(ctx, ctx->m_slots.reserve(slots + 1));
        TM_HIP(ctx, hipMemcpyAsync(ctx->m_qoff.p, qo.data(), P * 8ull, hipMemcpyHostToDevice, s));
        TM_HIP(ctx, hipMemcpyAsync(ctx->m_toff.p, to.data(), P * 8ull, hipMemcpyHostToDevice, s));
        ta_device_io io{};
        io.query_bytes = ctx->bytes.as<const char>();
        io.query_off = ctx->m_qoff.as<const uint64_t>();
        io.target_bytes = idx->ref2.as<const char>();
        io.target_off = ctx->m_toff.as<const uint64_t>();
        io.score = ctx->m_score.as<int32_t>();
        io.target_begin = ctx->m_tb.as<uint32_t>();
        io.cigar_slots = ctx->m_slots.as<char>();
        io.cigar_start = ctx->m_cstart.as<uint64_t>();
        io.cigar_len = ctx->m_clen.as<uint32_t>();
        if (int r = stage(4)) return r;
        if (int r = aplan   ? ta_banded_affine_plan_execute(aplan, &io, s)
                    : bplan ? ta_banded_plan_execute(bplan, &io, s)
                            : ta_plan_execute(plan, &io, s))
            return fail(ctx, TM_ERR_DEVICE, std::string("ta_plan_execute: ") + ta_last_error(ctx->ta) + " (" +
                                                ta_status_string(r) + ")");
        if (out && band_auto) {  // the certificate, on the execution's stream
            TM_HIP(ctx, ctx->m_exact.reserve(P));
            TM_HIP(ctx, ctx->m_need.reserve(P * 4ull));
            if (int r = aplan ? ta_banded_affine_plan_certify(aplan, &io, ctx->m_exact.as<uint8_t>(),
                                                              ctx->m_need.as<uint32_t>(), s)
                              : ta_banded_plan_certify(bplan, &io, ctx->m_exact.as<uint8_t>(),
                                                       ctx->m_need.as<uint32_t>(), s))
                return fail(ctx, TM_ERR_DEVICE, std::string("ta_plan_certify: ") + ta_last_error(ctx->ta) + " (" +
                                                    ta_status_string(r) + ")");
            out->exact.resize(P);
            out->need.resize(P);
            TM_HIP(ctx, hipMemcpyAsync(out->exact.data(), ctx->m_exact.p, P, hipMemcpyDeviceToHost, s));
            TM_HIP(ctx, hipMemcpyAsync(out->need.data(), ctx->m_need.p, P * 4ull, hipMemcpyDeviceToHost, s));
        }
        if (int r = stage(5)) return r;
        const char* c_slots = ctx->m_slots.as<const char>();
        const uint64_t* c_start = ctx->m_cstart.as<const uint64_t>();
        const uint32_t* c_len = ctx->m_clen.as<const uint32_t>();
        std::vector<ta_pair_info> pinfo;
        if (eqx) {  // info records and the =/X CIGARs, which take the base CIGARs' place below
            TM_HIP(ctx, ctx->m_info.reserve(P * sizeof(ta_pair_info)));
            ta_annotate_io ao{};
            ao.info = ctx->m_info.as<ta_pair_info>();
            if (opt->want_cigar) {
                TM_HIP(ctx, ctx->m_eslots.reserve(slots + 1));
                TM_HIP(ctx, ctx->m_estart.reserve(P * 8ull));
                TM_HIP(ctx, ctx->m_elen.reserve(P * 4ull));
                ao.eqx_slots = ctx->m_eslots.as<char>();
                ao.eqx_start = ctx->m_estart.as<uint64_t>();
                ao.eqx_len = ctx->m_elen.as<uint32_t>();
                c_slots = ao.eqx_slots;
                c_start = ao.eqx_start;
                c_len = ao.eqx_len;
            }
            if (int r = aplan   ? ta_banded_affine_plan_annotate(aplan, &io, &ao, s)
                        : bplan ? ta_banded_plan_annotate(bplan, &io, &ao, s)
                                : ta_plan_annotate(plan, &io, &ao, s))
                return fail(ctx, TM_ERR_DEVICE, std::string("ta_plan_annotate: ") + ta_last_error(ctx->ta) + " (" +
                                                    ta_status_string(r) + ")");
            if (info || out) {
                pinfo.resize(P);
                TM_HIP(ctx, hipMemcpyAsync(pinfo.data(), ctx->m_info.p, P * sizeof(ta_pair_info), hipMemcpyDeviceToHost, s));
            }
        }
        std::vector<int32_t> sc(P);
        TM_HIP(ctx, hipMemcpyAsync(sc.data(), ctx->m_score.p, P * 4ull, hipMemcpyDeviceToHost, s));
        std::vector<uint64_t> co;
        uint64_t total = 0;
        if (opt->want_cigar) {
            // pack the CIGAR slots on the device, then copy only the CIGAR bytes
            if (int r = tmap::compact_segments(ctx, P, c_slots, c_start, c_len, ctx->m_coff, ctx->m_cdst,
                                               ctx->match.cub_tmp, total))
                return r;
            if (!out && total > arena_bytes) return fail(ctx, TM_ERR_CAPACITY, "cigar arena too small");
            co.resize(P + 1);
            TM_HIP(ctx, hipMemcpyAsync(co.data(), ctx->m_coff.p, (P + 1) * 8ull, hipMemcpyDeviceToHost, s));
            if (out) out->cig.resize(total);
            if (total) TM_HIP(ctx, hipMemcpyAsync(out ? out->cig.data() : arena, ctx->m_cdst.p, total, hipMemcpyDeviceToHost, s));
        }
        TM_HIP(ctx, hipStreamSynchronize(s));
        if (int r = aplan ? ta_banded_affine_plan_check(aplan) : bplan ? ta_banded_plan_check(bplan) : ta_plan_check(plan))
            return fail(ctx, TM_ERR_DEVICE, std::string("ta_plan_check: ") + ta_last_error(ctx->ta) + " (" +
                                                ta_status_string(r) + ")");
        if (out) {  // merged below, once both rounds are in
            out->sc.swap(sc);
            out->pinfo.swap(pinfo);
            out->co.swap(co);
            return TM_OK;
        }
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t r = pair_read[p];
            score[r] = sc[p];
            if (info) info[r] = pinfo[p];
            if (!opt->want_cigar) continue;
            cigar_off[r] = co[p];
            cigar_len[r] = (uint32_t)(co[p + 1] - co[p]);
        }
        return TM_OK;
    };
    ctx->plan_stats[0] = P;
    ctx->plan_stats[1] = aplan ? ta_banded_affine_plan_chunks(aplan) : bplan ? ta_banded_plan_chunks(bplan) : ta_plan_chunks(plan);
    ctx->plan_stats[2] = band ? 0 : ta_plan_dual_pairs(plan);
    ctx->plan_stats[3] = band ? 0 : ta_plan_flex_pairs(plan);
    ctx->plan_stats[4] = aplan   ? ta_banded_affine_plan_workspace_bytes(aplan)
                         : bplan ? ta_banded_plan_workspace_bytes(bplan)
                                 : ta_plan_workspace_bytes(plan);
    ctx->stage_cells = 0;
    for (uint32_t p = 0; p < P; ++p) ctx->stage_cells += (uint64_t)ql[p] * tl[p];
    // --extend-ends: one end (right: in place; left: the reversed bytes) of every window through an
    // anchored plan with a ta_device_io of its own -> scores, goal cells and CIGARs on the host
    struct End {
        std::vector<int32_t> sc;
        std::vector<uint32_t> gi, gj;
        std::vector<uint64_t> co;  // P + 1 offsets into cig
        std::vector<char> cig;
    };
    auto run_end = [&](const uint32_t* eq, const uint32_t* et, const char* qbytes, const uint64_t* d_qoff,
                       const char* tbytes, const uint64_t* d_toff, End& out) -> int {
        struct Guard {
            ta_anchored_plan* p = nullptr;
            ~Guard() { ta_anchored_plan_destroy(p); }
        } g;
        const std::vector<uint32_t> ebw(P, *band);
        // (both end plans get Z and the rule; zdrop < 0: the plain anchored plan)
        if (ta_anchored_plan_create_zdrop_rule(ctx->ta, P, eq, et, ebw.data(), opt->match, opt->mismatch,
                                               gap_open ? *gap_open : 0, opt->gap, opt->want_cigar, budget, 0, zdrop,
                                               zdrop_rule, &g.p) != TA_OK)
            return fail(ctx, TM_ERR_DEVICE, std::string("ta_anchored_plan_create: ") + ta_last_error(ctx->ta));
        const uint64_t eslots = ta_anchored_plan_cigar_slots_bytes(g.p);
        ctx->plan_stats[1] += ta_anchored_plan_chunks(g.p);
        ctx->plan_stats[4] = std::max<uint64_t>(ctx->plan_stats[4], ta_anchored_plan_workspace_bytes(g.p));
        TM_HIP(ctx, ctx->e_score.reserve(P * 4ull));
        TM_HIP(ctx, ctx->e_tb.reserve(P * 4ull));
        TM_HIP(ctx, ctx->e_cstart.reserve(P * 8ull));
        TM_HIP(ctx, ctx->e_clen.reserve(P * 4ull));
        TM_HIP(ctx, ctx->e_slots.reserve(eslots + 1));
        TM_HIP(ctx, ctx->e_qend.reserve(P * 4ull));
        TM_HIP(ctx, ctx->e_tend.reserve(P * 4ull));
        ta_device_io io{};
        io.query_bytes = qbytes;
        io.query_off = d_qoff;
        io.target_bytes = tbytes;
        io.target_off = d_toff;
        io.score = ctx->e_score.as<int32_t>();
        io.target_begin = ctx->e_tb.as<uint32_t>();
        io.cigar_slots = ctx->e_slots.as<char>();
        io.cigar_start = ctx->e_cstart.as<uint64_t>();
        io.cigar_len = ctx->e_clen.as<uint32_t>();
        int r = ta_anchored_plan_execute(g.p, &io, s);
        if (r == TA_OK) r = ta_anchored_plan_ends(g.p, ctx->e_qend.as<uint32_t>(), ctx->e_tend.as<uint32_t>(), s);
        if (r != TA_OK)
            return fail(ctx, TM_ERR_DEVICE, std::string("ta_anchored_plan_execute: ") + ta_last_error(ctx->ta) + " (" +
                                                ta_status_string(r) + ")");
        out.sc.resize(P);
        out.gi.resize(P);
        out.gj.resize(P);
        TM_HIP(ctx, hipMemcpyAsync(out.sc.data(), ctx->e_score.p, P * 4ull, hipMemcpyDeviceToHost, s));
        TM_HIP(ctx, hipMemcpyAsync(out.gi.data(), ctx->e_qend.p, P * 4ull, hipMemcpyDeviceToHost, s));
        TM_HIP(ctx, hipMemcpyAsync(out.gj.data(), ctx->e_tend.p, P * 4ull, hipMemcpyDeviceToHost, s));
        if (opt->want_cigar) {
            uint64_t total = 0;
            if (int rr = tmap::compact_segments(ctx, P, io.cigar_slots, io.cigar_start, io.cigar_len, ctx->m_coff,
                                                ctx->m_cdst, ctx->match.cub_tmp, total))
                return rr;
            out.co.resize(P + 1);
            out.cig.resize(total);
            TM_HIP(ctx, hipMemcpyAsync(out.co.data(), ctx->m_coff.p, (P + 1) * 8ull, hipMemcpyDeviceToHost, s));
            if (total) TM_HIP(ctx, hipMemcpyAsync(out.cig.data(), ctx->m_cdst.p, total, hipMemcpyDeviceToHost, s));
        }
        TM_HIP(ctx, hipStreamSynchronize(s));
        return TM_OK;
    };
    // the windows' results are in `mid`; extends q/t begin/end, sums the scores, stitches the CIGARs
    auto extend = [&](const Round& mid) -> int {
        const uint64_t L = idx->len;
        const uint64_t w = *band;
        // right ends: query R[qe+1 .. len), target S[te+1 .. te+1+mr), mr = min(L-1-te, nr + w), read in place
        std::vector<uint32_t> eq(P), et(P);
        std::vector<uint64_t> eqo(P), eto(P);
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t r = pair_read[p];
            const uint64_t strand = strand_fwd[r] ? 0 : L;
            eq[p] = len[r] - 1 - q_end[r];
            et[p] = (uint32_t)std::min<uint64_t>(L - 1 - t_end[r], eq[p] + w);
            eqo[p] = off[r] + q_end[r] + 1;
            eto[p] = strand + t_end[r] + 1;
        }
        TM_HIP(ctx, ctx->e_qoff.reserve(P * 8ull));
        TM_HIP(ctx, ctx->e_toff.reserve(P * 8ull));
        TM_HIP(ctx, hipMemcpyAsync(ctx->e_qoff.p, eqo.data(), P * 8ull, hipMemcpyHostToDevice, s));
        TM_HIP(ctx, hipMemcpyAsync(ctx->e_toff.p, eto.data(), P * 8ull, hipMemcpyHostToDevice, s));
        End right, left;
        if (int r = run_end(eq.data(), et.data(), ctx->bytes.as<const char>(), ctx->e_qoff.as<const uint64_t>(),
                            idx->ref2.as<const char>(), ctx->e_toff.as<const uint64_t>(), right))
            return r;
        // left ends: the reverse of R[0 .. qb) against the reverse of S[tb-ml .. tb), ml = min(tb, nl + w),
        // gathered into a staging buffer: [queries][targets], one offset array each
        std::vector<uint64_t> meta(4ull * P);  // source ends (q, t), then staging offsets (q, t)
        uint64_t at = 0;
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t r = pair_read[p];
            eq[p] = q_begin[r];
            et[p] = (uint32_t)std::min<uint64_t>(t_begin[r], eq[p] + w);
            meta[p] = off[r] + q_begin[r];
            meta[P + p] = (strand_fwd[r] ? 0 : L) + t_begin[r];
            meta[2ull * P + p] = at;
            at += eq[p];
        }
        for (uint32_t p = 0; p < P; ++p) {
            meta[3ull * P + p] = at;
            at += et[p];
        }
        TM_HIP(ctx, ctx->e_meta.reserve(4ull * P * 8 + 2ull * P * 4));
        TM_HIP(ctx, ctx->e_rev.reserve(at + 1));
        uint64_t* d_meta = ctx->e_meta.as<uint64_t>();
        uint32_t* d_lens = reinterpret_cast<uint32_t*>(d_meta + 4ull * P);
        TM_HIP(ctx, hipMemcpyAsync(d_meta, meta.data(), 4ull * P * 8, hipMemcpyHostToDevice, s));
        TM_HIP(ctx, hipMemcpyAsync(d_lens, eq.data(), P * 4ull, hipMemcpyHostToDevice, s));
        TM_HIP(ctx, hipMemcpyAsync(d_lens + P, et.data(), P * 4ull, hipMemcpyHostToDevice, s));
        if (int r = tmap::reverse_gather(ctx, P, ctx->bytes.as<const uint8_t>(), d_meta, d_lens, d_meta + 2ull * P,
                                         ctx->e_rev.as<uint8_t>()))
            return r;
        if (int r = tmap::reverse_gather(ctx, P, idx->ref2.as<const uint8_t>(), d_meta + P, d_lens + P,
                                         d_meta + 3ull * P, ctx->e_rev.as<uint8_t>()))
            return r;
        if (int r = run_end(eq.data(), et.data(), ctx->e_rev.as<const char>(), d_meta + 2ull * P,
                            ctx->e_rev.as<const char>(), d_meta + 3ull * P, left))
            return r;
        if (int r = stage_add(5)) return r;  // the extension is alignment time
        std::string text;
        uint64_t used = 0;
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t r = pair_read[p];
            score[r] = mid.sc[p] + left.sc[p] + right.sc[p];
            q_begin[r] -= left.gi[p];
            t_begin[r] -= left.gj[p];
            q_end[r] += right.gi[p];
            t_end[r] += right.gj[p];
            if (!opt->want_cigar) continue;
            if (!tmap::stitch_cigar(left.cig.data() + left.co[p], left.co[p + 1] - left.co[p],
                                    mid.cig.data() + mid.co[p], mid.co[p + 1] - mid.co[p],
                                    right.cig.data() + right.co[p], right.co[p + 1] - right.co[p], text))
                return fail(ctx, TM_ERR_DEVICE, "--extend-ends: a malformed CIGAR piece");
            if (used + text.size() > arena_bytes) return fail(ctx, TM_ERR_CAPACITY, "cigar arena too small");
            std::memcpy(arena + used, text.data(), text.size());
            cigar_off[r] = used;
            cigar_len[r] = (uint32_t)text.size();
            used += text.size();
        }
        return TM_OK;
    };
    if (extend_ends) {
        Round mid;
        rc = run(&mid);
        if (rc == TM_OK) rc = stage(6);  // (the windows' download)
        if (rc == TM_OK) rc = extend(mid);
        if (rc == TM_OK) rc = stage_add(6);  // (the stitching)
    } else if (!band_auto) {
        rc = run(nullptr);
    } else {
        // round 1 over every window, round 2 (a second plan with its own ta_device_io)
        // over the uncertified ones; round 2's results replace round 1's
        Round r1, r2;
        const uint32_t P1 = P;
        std::vector<uint32_t> again;  // round 2's k-th pair is window again[k]
        rc = run(&r1);
        ta_banded_plan_destroy(bplan);
        ta_banded_affine_plan_destroy(aplan);
        bplan = nullptr;
        aplan = nullptr;
        if (rc == TM_OK) {
            std::vector<uint32_t> ql2, tl2, bw2;
            std::vector<uint64_t> qo2, to2;
            for (uint32_t p = 0; p < P1; ++p) {
                if (r1.exact[p]) continue;
                again.push_back(p);
                ql2.push_back(ql[p]);
                tl2.push_back(tl[p]);
                qo2.push_back(qo[p]);
                to2.push_back(to[p]);
                bw2.push_back(r1.need[p]);
            }
            if (!again.empty()) {
                const double ms4 = ctx->stage_ms[4], ms5 = ctx->stage_ms[5];
                P = (uint32_t)again.size();
                ql.swap(ql2);
                tl.swap(tl2);
                qo.swap(qo2);
                to.swap(to2);
                bw.swap(bw2);
                rc = create();
                if (rc != TA_OK) {
                    rc = fail(ctx, TM_ERR_DEVICE, std::string("ta_plan_create: ") + ta_last_error(ctx->ta));
                } else {
                    slots = aplan ? ta_banded_affine_plan_cigar_slots_bytes(aplan) : ta_banded_plan_cigar_slots_bytes(bplan);
                    ctx->plan_stats[1] += aplan ? ta_banded_affine_plan_chunks(aplan) : ta_banded_plan_chunks(bplan);
                    ctx->plan_stats[4] = std::max<uint64_t>(ctx->plan_stats[4],
                                                            aplan ? ta_banded_affine_plan_workspace_bytes(aplan)
                                                                  : ta_banded_plan_workspace_bytes(bplan));
                    rc = run(&r2);
                    ctx->stage_ms[4] += ms4;  // both rounds
                    ctx->stage_ms[5] += ms5;
                }
            }
        }
        if (rc == TM_OK) {
            std::vector<uint32_t> slot2(P1, UINT32_MAX);
            for (uint32_t k = 0; k < (uint32_t)again.size(); ++k) slot2[again[k]] = k;
            uint64_t at = 0;
            for (uint32_t p = 0; p < P1 && rc == TM_OK; ++p) {
                const Round& R = slot2[p] == UINT32_MAX ? r1 : r2;
                const uint32_t i = slot2[p] == UINT32_MAX ? p : slot2[p];
                const uint32_t r = pair_read[p];
                score[r] = R.sc[i];
                if (info) info[r] = R.pinfo[i];
                if (!opt->want_cigar) continue;
                const uint64_t n = R.co[i + 1] - R.co[i];
                if (at + n > arena_bytes) {
                    rc = fail(ctx, TM_ERR_CAPACITY, "cigar arena too small");
                    break;
                }
                std::memcpy(arena + at, R.cig.data() + R.co[i], n);
                cigar_off[r] = at;
                cigar_len[r] = (uint32_t)n;
                at += n;
            }
        }
    }
    ta_plan_destroy(plan);
    ta_banded_plan_destroy(bplan);
    ta_banded_affine_plan_destroy(aplan);
    if (rc == TM_OK && !extend_ends) rc = stage(6);
    return rc;
}

int tm_stage_times(const tm_context* ctx, double* ms, uint32_t n, uint64_t* aligned_cells) {
    if (!ctx || (n && !ms)) return TM_ERR_ARG;
    for (uint32_t i = 0; i < n && i < (uint32_t)tmap::kStages; ++i) ms[i] = ctx->stage_ms[i];
    if (aligned_cells) *aligned_cells = ctx->stage_cells;
    return TM_OK;
}

int tm_align_plan_stats(const tm_context* ctx, uint64_t out[5]) {
    if (!ctx || !out) return TM_ERR_ARG;
    for (int i = 0; i < 5; ++i) out[i] = ctx->plan_stats[i];
    return TM_OK;
}

int tm_map_files(const char* reference_path, const char* reads_path, const tm_options* opt, const char* out_path,
                 int device) {
    return tm_map_files_x(reference_path, reads_path, opt, out_path, device, 0);
}

static int map_files_impl(const char* reference_path, const char* reads_path, const tm_options* opt,
                          const char* out_path, int device, uint32_t flags, const uint32_t* band,
                          const int* gap_open = nullptr, bool band_auto = false, bool extend_ends = false,
                          int32_t zdrop = -1, int zdrop_rule = TA_ZDROP_SEGMENT);

int tm_map_files_x(const char* reference_path, const char* reads_path, const tm_options* opt, const char* out_path,
                   int device, uint32_t flags) {
    return map_files_impl(reference_path, reads_path, opt, out_path, device, flags, nullptr);
}

int tm_map_files_band(const char* reference_path, const char* reads_path, const tm_options* opt, const char* out_path,
                      int device, uint32_t flags, uint32_t band) {
    return map_files_impl(reference_path, reads_path, opt, out_path, device, flags, &band);
}

int tm_map_files_band_affine(const char* reference_path, const char* reads_path, const tm_options* opt,
                             const char* out_path, int device, uint32_t flags, uint32_t band, int gap_open) {
    return map_files_impl(reference_path, reads_path, opt, out_path, device, flags, &band, &gap_open);
}

int tm_map_files_band_ends(const char* reference_path, const char* reads_path, const tm_options* opt,
                           const char* out_path, int device, uint32_t flags, uint32_t band, const int* gap_open) {
    return map_files_impl(reference_path, reads_path, opt, out_path, device, flags, &band, gap_open, false, true);
}

int tm_map_files_band_ends_zdrop(const char* reference_path, const char* reads_path, const tm_options* opt,
                                 const char* out_path, int device, uint32_t flags, uint32_t band, const int* gap_open,
                                 int32_t zdrop) {
    return tm_map_files_band_ends_zdrop_rule(reference_path, reads_path, opt, out_path, device, flags, band, gap_open,
                                             zdrop, TA_ZDROP_SEGMENT);
}

int tm_map_files_band_ends_zdrop_rule(const char* reference_path, const char* reads_path, const tm_options* opt,
                                      const char* out_path, int device, uint32_t flags, uint32_t band,
                                      const int* gap_open, int32_t zdrop, int zdrop_rule) {
    return map_files_impl(reference_path, reads_path, opt, out_path, device, flags, &band, gap_open, false, true,
                          zdrop, zdrop_rule);
}

int tm_map_files_band_exact(const char* reference_path, const char* reads_path, const tm_options* opt,
                            const char* out_path, int device, uint32_t flags, const int* gap_open) {
    const uint32_t none = 0;
    return map_files_impl(reference_path, reads_path, opt, out_path, device, flags, &none, gap_open, true);
}

static int map_files_impl(const char* reference_path, const char* reads_path, const tm_options* opt,
                          const char* out_path, int device, uint32_t flags, const uint32_t* band, const int* gap_open,
                          bool band_auto, bool extend_ends, int32_t zdrop, int zdrop_rule) {
    if (!reference_path || !reads_path || !opt || !out_path || (flags & ~TM_MAP_EQX)) return TM_ERR_ARG;
    if (zdrop >= 0 && !extend_ends) return TM_ERR_ARG;
    if (zdrop_rule != TA_ZDROP_SEGMENT && zdrop_rule != TA_ZDROP_STRIPE) return TM_ERR_ARG;
    // (before any file is read: the same rules as tm_map_batch_band_ends)
    if (extend_ends && (!band || band_auto || opt->type != TA_GLOBAL || (flags & TM_MAP_EQX))) return TM_ERR_ARG;
    const bool eqx = (flags & TM_MAP_EQX) != 0;
    tmap::FastxFile ref, reads;
    std::string err;
    if (!tmap::read_fastx(reference_path, false, ref, err) || ref.records.empty()) {
        std::fprintf(stderr, "%s\n", err.empty() ? "reference: no sequences" : err.c_str());
        return TM_ERR_INPUT;
    }
    // fragments: FASTQ first, FASTA when that fails (team_mapper.cpp:533-556)
    bool fastq = tmap::read_fastx(reads_path, true, reads, err);
    if (!fastq && !tmap::read_fastx(reads_path, false, reads, err)) {
        std::fprintf(stderr, "Given file is not in FASTA or FASTQ format! \n");
        return TM_ERR_INPUT;
    }
    tm_context* ctx = nullptr;
    if (int r = tm_context_create(device, &ctx)) return r;
    const tmap::FastxRecord& R = ref.records.front();
    tm_index* idx = nullptr;
    int rc = tm_index_create(ctx, R.name.c_str(), ref.seq.data() + R.off, R.len, opt->k, opt->w, opt->f, &idx);
    if (rc) {
        std::fprintf(stderr, "index: %s: %s\n", tm_status_string(rc), tm_last_error(ctx));
        tm_context_destroy(ctx);
        return rc;
    }
    FILE* out = std::strcmp(out_path, "-") == 0 ? stdout : std::fopen(out_path, "wb");
    if (!out) {
        tm_index_destroy(idx);
        tm_context_destroy(ctx);
        return TM_ERR_INPUT;
    }
    tm_options o = *opt;
    o.fastq_rules = fastq ? 1 : 0;
    const size_t n = reads.records.size();
    const uint64_t kBatchBases = 1ull << 30;  // reads per device batch: up to ~1 Gbase
    std::string line;
    for (size_t b = 0; b < n && rc == TM_OK;) {
        size_t e = b;
        uint64_t bases = 0;
        while (e < n && (e == b || bases + reads.records[e].len <= kBatchBases)) bases += reads.records[e++].len;
        const uint32_t nr = (uint32_t)(e - b);
        std::vector<uint64_t> off(nr);
        std::vector<uint32_t> len(nr);
        const uint64_t base = reads.records[b].off;
        uint64_t arena_bytes = 0;
        for (uint32_t i = 0; i < nr; ++i) {
            off[i] = reads.records[b + i].off - base;
            len[i] = (uint32_t)reads.records[b + i].len;
            // a run takes at least 2 bytes and consumes at least one base: the window's CIGAR fits
            // 4 len + 2; with extended ends each end's target may be `band` longer than its query
            // (tm_ends_arena_extra: the band term is bounded whatever the band)
            arena_bytes += 4ull * len[i] + 2 + (extend_ends ? tm_ends_arena_extra(len[i], *band) : 0);
        }
        std::vector<uint8_t> mapped(nr), fwd(nr);
        std::vector<uint32_t> qb(nr), qe(nr), tb(nr), te(nr), cl(nr);
        std::vector<int32_t> sc(nr);
        std::vector<uint64_t> co(nr);
        std::vector<char> arena(o.want_cigar ? arena_bytes : 0);
        std::vector<ta_pair_info> info(eqx ? nr : 0);
        rc = map_batch_impl(ctx, idx, nr, reads.seq.data() + base, off.data(), len.data(), &o, mapped.data(),
                            fwd.data(), qb.data(), qe.data(), tb.data(), te.data(), sc.data(), arena.data(), arena.size(),
                            co.data(), cl.data(), flags, eqx ? info.data() : nullptr, band, gap_open, band_auto,
                            extend_ends, zdrop, zdrop_rule);
        if (rc) {
            std::fprintf(stderr, "map: %s: %s\n", tm_status_string(rc), tm_last_error(ctx));
            break;
        }
        for (uint32_t i = 0; i < nr; ++i) {
            if (!mapped[i]) continue;
            const tmap::FastxRecord& q = reads.records[b + i];
            // team_mapper.cpp:686-697; reverse-strand windows reported in forward coordinates
            const uint64_t L = idx->len;
            const uint64_t ts = fwd[i] ? tb[i] : L - te[i] - 1, tend = fwd[i] ? (uint64_t)te[i] + 1 : L - tb[i];
            line.clear();
            line += q.name;
            line += '\t' + std::to_string(q.len) + '\t' + std::to_string(qb[i]) + '\t' + std::to_string(qe[i] + 1ull);
            line += fwd[i] ? "\t+\t" : "\t-\t";
            line += idx->name + '\t' + std::to_string(L) + '\t' + std::to_string(ts) + '\t' + std::to_string(tend);
            line += '\t' + std::to_string(sc[i]) + '\t' + std::to_string(qe[i] - qb[i] + 1ull) + "\t60";
            if (o.want_cigar) {
                line += "\tcg:Z:";
                line.append(arena.data() + co[i], cl[i]);
            }
            if (eqx) line += "\tNM:i:" + std::to_string((uint64_t)info[i].n_x + info[i].n_ins + info[i].n_del);
            line += '\n';
            std::fwrite(line.data(), 1, line.size(), out);
        }
        b = e;
    }
    if (out != stdout) std::fclose(out);
    else std::fflush(stdout);
    tm_index_destroy(idx);
    tm_context_destroy(ctx);
    return rc;
}

}  // extern "C"
