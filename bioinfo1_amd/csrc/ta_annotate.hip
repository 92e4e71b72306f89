// bioinfo1_amd/csrc/ta_annotate.hip -- the annotate post-pass:
// after a plan's execution, one wave per pair reads the finished CIGAR text,
// the two sequences and the plan's goal cell, and writes the pair's
// ta_pair_info record and, optionally, the extended CIGAR in which every M
// run is split into maximal '=' / 'X' runs.  Work is proportional to the
// alignment columns (n + m); no fill or walk is involved.
//
// The text is parsed 64 bytes per step: a lane holding an op letter reads its
// run's digits back, and wave prefix sums give each run its first column and
// its (i, j).  The step's columns are then processed 64 at a time: lane k finds
// the run of column c0 + k by a binary search over the inclusive column sums
// (ds_bpermute), classifies the column, and ballots give the counts and the
// sub-run boundaries.  A sub-run is written when the next one starts (its
// length from the boundary ballot, or from the carry when it began in an
// earlier step), forward from the start of the pair's slot.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_internal.h"

namespace ta {
namespace {

__device__ __forceinline__ uint32_t bperm(uint32_t v, uint32_t src_lane) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), (int)v);
}

__device__ __forceinline__ uint32_t scan_incl(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

__device__ __forceinline__ uint32_t ndigits(uint32_t c) {
    return 1u + (c >= 10u) + (c >= 100u) + (c >= 1000u) + (c >= 10000u) + (c >= 100000u) + (c >= 1000000u) +
           (c >= 10000000u) + (c >= 100000000u) + (c >= 1000000000u);
}

// "<c><op>" at dst (digits + 1 bytes)
__device__ __forceinline__ void put_run(char* dst, uint32_t c, uint32_t digits, uint32_t op) {
    dst[digits] = (char)op;
#pragma unroll
    for (uint32_t d = 0; d < 10u; ++d) {
        if (d < digits) dst[digits - 1u - d] = (char)('0' + c % 10u);
        c /= 10u;
    }
}

// Lane k of a text step: byte t0 + k and, when it is an op letter, its run's
// length from the digits before it (at most 10); cnt 0 otherwise.
__device__ __forceinline__ void parse_step(const uint8_t* text, uint32_t len, uint32_t t0, int lane, uint32_t& ch,
                                           uint32_t& cnt) {
    const uint32_t t = t0 + (uint32_t)lane;
    ch = t < len ? (uint32_t)text[t] : (uint32_t)'0';
    cnt = 0;
    if (ch < '0' || ch > '9') {
        uint32_t mul = 1;
        bool stop = false;
#pragma unroll
        for (uint32_t d = 1; d <= 10u; ++d) {
            const uint32_t b = t >= d ? (uint32_t)text[t - d] - (uint32_t)'0' : 99u;
            stop |= b > 9u;
            if (!stop) cnt += b * mul;
            mul *= 10u;
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

__device__ __forceinline__ uint32_t popc(uint64_t b) { return (uint32_t)__builtin_popcountll(b); }

__global__ __launch_bounds__(kBlock) void annotate_kernel(AnnotateArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t p = wave_id();
    if (p >= a.n_pairs) return;
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.qlen[p]);
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.tlen[p]);
    // the goal cell: analytic where no cell exists (n or m 0: local and anchored (0, 0), semi-global (0, m))
    uint32_t gi = n, gj = m;
    if (a.mode != kGlobal) {
        gi = 0;
        gj = a.mode == kSemi ? m : 0;
        if (n && m) {
            gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.goal_i[p]);
            gj = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.goal_j[p]);
        }
    }
    const uint64_t so = a.slot_off[p];
    const uint64_t cap = cigar_slot_bytes(n, m);
    const uint64_t st = a.cigar_start[p];
    uint32_t len = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.cigar_len[p]);
    // a text outside the pair's slot (no execution yet) is read as empty: nothing past the slot is touched
    if (st < so || st + len > so + cap) len = 0;
    const uint8_t* text = reinterpret_cast<const uint8_t*>(a.slots) + st;
    if (len == 2) {  // the empty op string's "1\0"
        const uint32_t b1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)text[1]);
        if (b1 == 0) len = 0;
    }
    const uint8_t* Q = a.qbytes + a.qoff[p];
    const uint8_t* T = a.tbytes + a.toff[p];
    char* out = a.eqx_slots ? a.eqx_slots + so : nullptr;

    uint32_t Cb = 0, Ib = 0, Jb = 0;  // columns before this text step, and its first column's (i, j)
    if (a.mode == kLocal) {  // the path ends at the goal cell: it starts there minus its consumption
        uint32_t qsum = 0, tsum = 0;
        for (uint32_t t0 = 0; t0 < len; t0 += 64u) {
            uint32_t ch, cnt;
            parse_step(text, len, t0, lane, ch, cnt);
            qsum += (ch == 'M' || ch == 'D') ? cnt : 0u;
            tsum += (ch == 'M' || ch == 'I') ? cnt : 0u;
        }
        Ib = gi - wave_sum(qsum);
        Jb = gj - wave_sum(tsum);
    }
    const uint32_t i0 = Ib, j0 = Jb;
    uint32_t lead_len = 0, first_op = 0;
    uint32_t n_eq = 0, n_x = 0, n_ins = 0, n_del = 0, n_gap = 0, n_free = 0, lead_cnt = 0;
    uint32_t carry_key = 0, carry_len = 0;  // the last column's class; the open sub-run's length
    uint32_t used = 0;
    for (uint32_t t0 = 0; t0 < len; t0 += 64u) {
        uint32_t ch, cnt;
        parse_step(text, len, t0, lane, ch, cnt);
        const bool letter = cnt != 0u;
        const uint32_t qc = (ch == 'M' || ch == 'D') ? cnt : 0u;
        const uint32_t tc = (ch == 'M' || ch == 'I') ? cnt : 0u;
        const uint32_t incC = scan_incl(cnt, lane);
        const uint32_t incI = scan_incl(qc, lane);
        const uint32_t incJ = scan_incl(tc, lane);
        const uint32_t total = (uint32_t)rdlane((int)incC, 63);
        if (t0 == 0) {
            const uint64_t lb = ballot(letter);
            if (lb) {
                const uint32_t fl = (uint32_t)__builtin_ctzll(lb);
                first_op = (uint32_t)rdlane((int)ch, fl);
                if (a.mode == kSemi && (first_op == 'I' || first_op == 'D')) lead_len = (uint32_t)rdlane((int)cnt, fl);
            }
        }
        const uint32_t exC = incC - cnt, exI = Ib + incI - qc, exJ = Jb + incJ - tc;  // run starts
        for (uint32_t cc = 0; cc < total; cc += 64u) {
            const uint32_t c = cc + (uint32_t)lane;
            const bool valid = c < total;
            const uint32_t ncol = min(64u, total - cc);
            // the run of column c: the first lane whose inclusive column sum exceeds c
            uint32_t lo = 0;
#pragma unroll
            for (uint32_t b = 32u; b; b >>= 1) {
                const uint32_t v = bperm(incC, lo + b - 1u);
                if (v <= c) lo += b;
            }
            const uint32_t rop = bperm(ch, lo), rC = bperm(exC, lo), rI = bperm(exI, lo), rJ = bperm(exJ, lo);
            const uint32_t d = c - rC;
            const uint32_t i = rI + (rop != 'I' ? d : 0u), j = rJ + (rop != 'D' ? d : 0u);
            uint32_t op = rop;
            if (valid && rop == 'M') op = (i < n && j < m && Q[i] == T[j]) ? '=' : 'X';
            bool fre = false;
            if (a.mode == kSemi) {
                const bool trailing = i >= gi && j >= gj;  // the path has reached the goal cell
                const bool leading = Cb + c < lead_len;
                fre = trailing || leading;
                lead_cnt += popc(ballot(valid && leading && !trailing));
            }
            const uint32_t key = valid ? (op | (fre ? 0x100u : 0u)) : 0u;
            uint32_t prev = (uint32_t)__shfl_up((int)key, 1, 64);
            if (lane == 0) prev = carry_key;
            const bool scored = valid && !fre;
            n_eq += popc(ballot(scored && op == '='));
            n_x += popc(ballot(scored && op == 'X'));
            n_ins += popc(ballot(scored && op == 'I'));
            n_del += popc(ballot(scored && op == 'D'));
            n_free += popc(ballot(valid && fre));
            n_gap += popc(ballot(scored && (op == 'I' || op == 'D') && key != prev));
            if (out) {
                // a sub-run starts where the op differs from the previous column's; the one
                // before it is finished there
                const uint64_t B = ballot(valid && (key & 0xFFu) != (prev & 0xFFu));
                const uint64_t below = B & ((1ull << lane) - 1ull);
                const uint32_t rl = below ? (uint32_t)lane - (63u - (uint32_t)__builtin_clzll(below))
                                          : carry_len + (uint32_t)lane;
                const bool em = ((B >> lane) & 1ull) && rl > 0u;
                const uint32_t dg = ndigits(rl);
                const uint32_t L = em ? dg + 1u : 0u;
                const uint32_t incl = scan_incl(L, lane);
                const uint64_t pos = (uint64_t)used + incl - L;
                if (em && pos + L <= cap) put_run(out + pos, rl, dg, prev & 0xFFu);
                used += (uint32_t)rdlane((int)incl, 63);
                if (B) carry_len = ncol - (63u - (uint32_t)__builtin_clzll(B));
                else carry_len += ncol;
            }
            carry_key = (uint32_t)rdlane((int)key, ncol - 1u);
        }
        Cb += total;
        Ib += (uint32_t)rdlane((int)incI, 63);
        Jb += (uint32_t)rdlane((int)incJ, 63);
    }
    if (lane != 0) return;
    if (out) {
        if (Cb == 0) {  // the empty op string, as the base CIGAR
            out[0] = '1';
            out[1] = '\0';
            used = 2;
        } else {
            const uint32_t dg = ndigits(carry_len);
            if ((uint64_t)used + dg + 1u <= cap) put_run(out + used, carry_len, dg, carry_key & 0xFFu);
            used += dg + 1u;
        }
        a.eqx_start[p] = so;
        a.eqx_len[p] = used;
    }
    if (a.info) {
        ta_pair_info r;
        if (a.mode == kGlobal) {
            r.query_begin = 0;
            r.target_begin = 0;
        } else if (a.mode == kLocal) {  // the ends minus the consumption
            r.query_begin = i0;
            r.target_begin = j0;
        } else {  // the cell after the free leading run (kAnchored comes here too: no free run, so 0 / 0)
            r.query_begin = first_op == 'D' ? lead_cnt : 0u;
            r.target_begin = first_op == 'I' ? lead_cnt : 0u;
        }
        r.query_end = gi;
        r.target_end = gj;
        r.n_eq = n_eq;
        r.n_x = n_x;
        r.n_ins = n_ins;
        r.n_del = n_del;
        r.n_gap_runs = n_gap;
        r.n_free = n_free;
        a.info[p] = r;
    }
}

}  // namespace

hipError_t launch_annotate(const AnnotateArgs& a, hipStream_t s) {
    if (!a.n_pairs) return hipSuccess;
    hipLaunchKernelGGL(annotate_kernel, dim3((a.n_pairs + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace ta
