// bioinfo1_amd/csrc/ta_band_exact.hip -- exact banded alignment: the
// certificate of a banded execution (band_certify_kernel, behind
// ta_banded_plan_certify / ta_banded_affine_plan_certify through
// ta_plan_driver.h plan_certify) and the two-round host batches
// ta_align_batch_banded_exact / ta_align_batch_banded_affine_exact.
//
// The rule is DEFINED in include/team_align_c.h, evaluated by ta_layout.h
// band_exact_* (host and device alike) and restated in tests/band_exact_ref.py;
// DESIGN.md §3.17 has the proof sketch.
//
// Kernel.  One wave64 per pair.  Only the global bound reads the number of '-'
// bytes, so only a global pair short of its full band under a certifiable
// scoring is counted: the lanes stride over the query's and the target's bytes
// (single bytes up to the first 4-byte boundary, aligned dwords, single bytes
// after the last), one per-lane count, one wave reduction.  Lane 0 evaluates
// the rule and writes exact[p] and band_needed[p].  No LDS, no workspace.
//
// Host batches.  The sequences are in host memory, so the host evaluates the
// same ta_layout.h functions on the first round's scores (one pass over the
// bytes of the global pairs that need a dash count) and runs the uncertified
// pairs once more, gathered by offset, at their needed band.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/team_align_c.h"
#include "ta_context.h"
#include "ta_device.h"
#include "ta_layout.h"
#include "ta_plan_driver.h"

namespace ta {
namespace {

// '-' bytes of S[0 .. len) seen by this lane; the lanes' counts sum to the sequence's.
__device__ __forceinline__ uint32_t count_dashes(const uint8_t* S, uint32_t len, int lane) {
    uint32_t c = 0;
    const uint32_t mis = (uint32_t)(4u - ((uintptr_t)S & 3u)) & 3u;
    const uint32_t head = min(len, mis);
    if ((uint32_t)lane < head) c += S[lane] == '-';
    const uint32_t nw = (len - head) >> 2;  // whole aligned dwords inside the sequence
    const uint32_t* W = reinterpret_cast<const uint32_t*>(S + head);
    for (uint32_t i = (uint32_t)lane; i < nw; i += kWave) {
        const uint32_t x = W[i] ^ 0x2D2D2D2Du;  // a '-' byte becomes 0
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 in each zero byte
        c += (uint32_t)__popc(z);
    }
    const uint32_t base = head + 4u * nw;
    if (base + (uint32_t)lane < len) c += S[base + lane] == '-';  // < 4 bytes
    return c;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

__global__ __launch_bounds__(kBlock) void band_certify_kernel(BandCertifyArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t p = wave_id();
    if (p >= a.n_pairs) return;  // wave-uniform
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.qlen[p]);
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.tlen[p]);
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.band[p]);
    uint32_t dashes = 0;
    if (a.mode == kGlobal && !band_exact_full(n, m, w) && band_exact_certifiable(a.gap_open, a.gap_extend)) {
        dashes = count_dashes(a.qbytes + a.qoff[p], n, lane) + count_dashes(a.tbytes + a.toff[p], m, lane);
        dashes = wave_sum(dashes);
    }
    if (lane == 0) {
        const long long s = a.score[p];
        const bool ok = band_exact_certified(a.mode, n, m, w, a.match, a.mismatch, a.gap_open, a.gap_extend, dashes, s);
        a.exact[p] = ok ? 1 : 0;
        a.band_needed[p] =
            ok ? w : band_exact_needed(a.mode, n, m, w, a.match, a.mismatch, a.gap_open, a.gap_extend, dashes, s);
    }
}

}  // namespace

hipError_t launch_band_certify(const BandCertifyArgs& a, hipStream_t s) {
    if (a.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(band_certify_kernel, dim3((a.n_pairs + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0,
                       s, a);
    return hipGetLastError();
}

}  // namespace ta

// ---------------------------------------------------------------------------
// The two-round host batches, over the banded host entries of either family.
namespace {

struct Round {  // one banded batch's host arrays
    std::vector<uint64_t> qoff, toff, coff;
    std::vector<uint32_t> qlen, tlen, band, tb, clen;
    std::vector<int32_t> score;
    std::unique_ptr<char[]> arena;  // not initialised: only the pages the CIGARs reach are touched
    uint64_t cap = 0;
    void outputs(uint32_t P, const uint32_t* ql, const uint32_t* tl, bool cigar) {
        score.assign(P, 0);
        tb.assign(P, 0);
        if (!cigar) return;
        coff.assign(P, 0);
        clen.assign(P, 0);
        for (uint32_t p = 0; p < P; ++p) cap += ta::cigar_slot_bytes(ql[p], tl[p]);
        arena.reset(new char[std::max<uint64_t>(cap, 1)]);
    }
};

// run(P, qoff, qlen, toff, tlen, band, score, target_begin, arena, arena_bytes, cigar_off, cigar_len):
// the family's banded host batch over the caller's byte buffers.
template <class Run>
int batch_exact(ta_context* ctx, uint32_t P, const char* qb, const uint64_t* qoff, const uint32_t* qlen,
                const char* tbytes, const uint64_t* toff, const uint32_t* tlen, const uint32_t* band_start, int type,
                int match, int mismatch, int gap_open, int gap_extend, int want_cigar, int32_t* score,
                uint32_t* target_begin, char* arena, uint64_t arena_bytes, uint64_t* cigar_off, uint32_t* cigar_len,
                uint32_t* band_used, uint8_t* rounds, Run run) {
    if (!ctx) return TA_ERR_ARG;
    // what the banded entry refuses, it refuses here (its message, before any work)
    if (P == 0 || !qoff || !qlen || !toff || !tlen || (want_cigar && (!arena || !cigar_off || !cigar_len)) ||
        !ta_host::valid_type(type)) {
        const uint32_t none = 0;
        return run(P, qoff, qlen, toff, tlen, band_start ? band_start : &none, score, target_begin, arena, arena_bytes,
                   cigar_off, cigar_len);
    }
    Round r1;
    r1.band.resize(P);
    for (uint32_t p = 0; p < P; ++p)
        r1.band[p] = ta::band_clamp(qlen[p], tlen[p],
                                    band_start ? band_start[p] : ta::band_exact_default_start(qlen[p], tlen[p]));
    r1.outputs(P, qlen, tlen, want_cigar != 0);
    if (int r = run(P, qoff, qlen, toff, tlen, r1.band.data(), r1.score.data(), r1.tb.data(), r1.arena.get(), r1.cap,
                    r1.coff.data(), r1.clen.data()))
        return r;
    // ---- the certificate; the uncertified pairs gathered for round 2
    Round r2;
    std::vector<uint32_t> again;  // pair of round 2's k-th entry
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t n = qlen[p], m = tlen[p], w = r1.band[p];
        uint64_t dashes = 0;
        if (type == TA_GLOBAL && !ta::band_exact_full(n, m, w) && ta::band_exact_certifiable(gap_open, gap_extend))
            dashes = (uint64_t)std::count(qb + qoff[p], qb + qoff[p] + n, '-') +
                     (uint64_t)std::count(tbytes + toff[p], tbytes + toff[p] + m, '-');
        if (ta::band_exact_certified(type, n, m, w, match, mismatch, gap_open, gap_extend, dashes, r1.score[p])) continue;
        again.push_back(p);
        r2.qoff.push_back(qoff[p]);
        r2.qlen.push_back(n);
        r2.toff.push_back(toff[p]);
        r2.tlen.push_back(m);
        r2.band.push_back(
            ta::band_exact_needed(type, n, m, w, match, mismatch, gap_open, gap_extend, dashes, r1.score[p]));
    }
    const uint32_t P2 = (uint32_t)again.size();
    if (P2) {
        r2.outputs(P2, r2.qlen.data(), r2.tlen.data(), want_cigar != 0);
        if (int r = run(P2, r2.qoff.data(), r2.qlen.data(), r2.toff.data(), r2.tlen.data(), r2.band.data(),
                        r2.score.data(), r2.tb.data(), r2.arena.get(), r2.cap, r2.coff.data(), r2.clen.data()))
            return r;
    }
    // ---- merge: round 2's results replace round 1's; CIGARs back to back in pair order
    std::vector<uint32_t> slot2(P, UINT32_MAX);
    for (uint32_t k = 0; k < P2; ++k) slot2[again[k]] = k;
    if (want_cigar) {
        uint64_t total = 0;
        for (uint32_t p = 0; p < P; ++p) total += slot2[p] == UINT32_MAX ? r1.clen[p] : r2.clen[slot2[p]];
        if (total > arena_bytes) return ta_host::fail(ctx, TA_ERR_CAPACITY, "cigar arena too small");
    }
    uint64_t at = 0;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t k = slot2[p];
        const Round& r = k == UINT32_MAX ? r1 : r2;
        const uint32_t i = k == UINT32_MAX ? p : k;
        if (score) score[p] = r.score[i];
        if (target_begin) target_begin[p] = r.tb[i];
        if (band_used) band_used[p] = r.band[i];
        if (rounds) rounds[p] = k == UINT32_MAX ? 1 : 2;
        if (want_cigar) {
            std::copy(r.arena.get() + r.coff[i], r.arena.get() + r.coff[i] + r.clen[i], arena + at);
            cigar_off[p] = at;
            cigar_len[p] = r.clen[i];
            at += r.clen[i];
        }
    }
    return TA_OK;
}

}  // namespace

extern "C" {

int ta_align_batch_banded_exact(ta_context* ctx, uint32_t n_pairs, const char* qb, const uint64_t* qoff,
                                const uint32_t* qlen, const char* tbytes, const uint64_t* toff, const uint32_t* tlen,
                                const uint32_t* band_start, int type, int match, int mismatch, int gap, int want_cigar,
                                int32_t* score, uint32_t* target_begin, char* arena, uint64_t arena_bytes,
                                uint64_t* cigar_off, uint32_t* cigar_len, uint32_t* band_used, uint8_t* rounds) {
    return batch_exact(ctx, n_pairs, qb, qoff, qlen, tbytes, toff, tlen, band_start, type, match, mismatch, 0, gap,
                       want_cigar, score, target_begin, arena, arena_bytes, cigar_off, cigar_len, band_used, rounds,
                       [&](uint32_t P, const uint64_t* qo, const uint32_t* ql, const uint64_t* to, const uint32_t* tl,
                           const uint32_t* band, int32_t* sc, uint32_t* tb, char* ar, uint64_t cap, uint64_t* co,
                           uint32_t* cl) {
                           return ta_align_batch_banded(ctx, P, qb, qo, ql, tbytes, to, tl, band, type, match, mismatch,
                                                        gap, want_cigar, sc, tb, ar, cap, co, cl);
                       });
}

int ta_align_batch_banded_affine_exact(ta_context* ctx, uint32_t n_pairs, const char* qb, const uint64_t* qoff,
                                       const uint32_t* qlen, const char* tbytes, const uint64_t* toff,
                                       const uint32_t* tlen, const uint32_t* band_start, int type, int match,
                                       int mismatch, int gap_open, int gap_extend, int want_cigar, int32_t* score,
                                       uint32_t* target_begin, char* arena, uint64_t arena_bytes, uint64_t* cigar_off,
                                       uint32_t* cigar_len, uint32_t* band_used, uint8_t* rounds) {
    return batch_exact(ctx, n_pairs, qb, qoff, qlen, tbytes, toff, tlen, band_start, type, match, mismatch, gap_open,
                       gap_extend, want_cigar, score, target_begin, arena, arena_bytes, cigar_off, cigar_len, band_used,
                       rounds,
                       [&](uint32_t P, const uint64_t* qo, const uint32_t* ql, const uint64_t* to, const uint32_t* tl,
                           const uint32_t* band, int32_t* sc, uint32_t* tb, char* ar, uint64_t cap, uint64_t* co,
                           uint32_t* cl) {
                           return ta_align_batch_banded_affine(ctx, P, qb, qo, ql, tbytes, to, tl, band, type, match,
                                                               mismatch, gap_open, gap_extend, want_cigar, sc, tb, ar,
                                                               cap, co, cl);
                       });
}

}  // extern "C"
