// bioinfo1_amd/csrc/ta_walk_affine.h -- the affine three-state traceback walk,
// shared by the affine plan (ta_affine.hip, codes of the whole matrix) and the
// banded affine plan (ta_banded_affine.hip, codes of the swept columns only).
//
// The walk (oracle/affine_oracle.c): H-state follows the source code, E/F-state
// emits one I/D per cell and keeps going while the cell's extension bit is
// set.  One cell per iteration (a whole run in H-state on M codes); the wave
// holds the codes of 64 consecutive steps of the current lane stripe (lane k:
// step tt0 + k) in two VGPRs and writes runs through the shared RunWriter.
//
// The two plans differ only in where a pass's codes lie.  GEO tells the walk,
// once per pass it enters:
//     uint32_t c0(pass)      the column of lane 0 at the pass's step 0
//     uint32_t steps(pass)   steps whose codes the pass stores
//     uint64_t offset(pass)  the pass's first entry in the pair's region
// and the entry of (pass, step t, lane l) is offset + t * 64 + l, row r of the
// stripe at bit 15 - r of each plane (.x = D << 16 | I, .y = F-ext << 16 | E-ext).
#pragma once

#include "ta_device.h"

namespace ta {
namespace {

// The whole matrix: every pass stores pass_steps(m) steps from column 1.
struct AffFullGeo {
    uint32_t Tmax;
    __device__ __forceinline__ uint32_t c0(uint32_t) const { return 1u; }
    __device__ __forceinline__ uint32_t steps(uint32_t) const { return Tmax; }
    __device__ __forceinline__ uint64_t offset(uint32_t pass) const { return (uint64_t)pass * Tmax * kWave; }
};

// The banded layout (ta_layout.h band_*): pass p stores the steps of its
// columns band_c0 .. band_c1, passes back to back.
struct AffBandGeo {
    uint32_t n, m, w;
    __device__ __forceinline__ uint32_t c0(uint32_t pass) const { return band_c0(n, m, w, pass); }
    __device__ __forceinline__ uint32_t steps(uint32_t pass) const { return band_pass_steps(n, m, w, pass); }
    __device__ __forceinline__ uint64_t offset(uint32_t pass) const { return band_pass_offset(n, m, w, pass); }
};

template <int MODE, class GEO>
__device__ __forceinline__ void aff_traceback_pair(const uint2* P, const GEO& geo, uint32_t n, uint32_t m, uint32_t gi,
                                                   uint32_t gj, char* slot, uint64_t cap, int lane,
                                                   uint64_t* start_in_slot, uint32_t* len) {
    RunWriter w{slot + cap, 0u, 0u, 0u, 0u, 0u, 0u, lane};
    if (MODE == kSemi && (gj != m || gi != n)) {  // :306-315 (the walk runs backwards: pushed first)
        if (gi == n) {
            if (m - gj) w.push('I', m - gj);
        } else if (gj == m && n - gi) {
            w.push('D', n - gi);
        }
    }
    uint32_t i = gi, j = gj, state = 0;  // 0 H, 1 E, 2 F
    uint32_t tP = 0xFFFFFFFFu, tL = 0xFFFFFFFFu, tt0 = 0;
    uint32_t pc0 = 1, psteps = 0;  // the current pass's first column and stored steps
    uint64_t pbase = 0;            // its first entry
    uint32_t cx = 0, cy = 0;
    // every iteration moves or leaves H-state, so 2(n+m)+2 bounds a correct
    // walk; the bound (and the E/F edge checks) only keep a corrupt code from
    // spinning the wave
    for (uint32_t it = 0; it < 2u * (n + m) + 2u; ++it) {
        if ((state == 1 && j == 0) || (state == 2 && i == 0)) break;
        if (state == 0) {
            if (MODE == kLocal) {
                if (min(i, j) == 0) break;  // boundary cost 0 ends the walk (:202)
            } else {
                if (i == 0) {  // row 0: INSERT run (:89-92)
                    if (j) w.push('I', j);
                    break;
                }
                if (j == 0) {  // column 0: DELETE run (:83-86)
                    w.push('D', i);
                    break;
                }
            }
        }
        const uint32_t row = i - 1;
        const uint32_t ln = (row >> 4) & 63u, r = row & 15u, ps = row >> 10;
        const bool new_pass = ps != tP;
        if (new_pass) {
            tP = ps;
            pc0 = geo.c0(ps);
            psteps = geo.steps(ps);
            pbase = geo.offset(ps);
        }
        const uint32_t t = (j - pc0) + ln;
        if (new_pass || ln != tL || t < tt0) {
            tL = ln;
            tt0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(max(t, 63u) - 63u));
            const uint32_t ts = tt0 + (uint32_t)lane;
            cx = cy = 0;
            if (ts < psteps) {
                const uint2 v = P[pbase + (uint64_t)ts * kWave + tL];
                cx = v.x;
                cy = v.y;
            }
        }
        const uint32_t kk = t - tt0;
        const uint32_t sh = 15u - r;
        const uint32_t x = (uint32_t)rdlane((int)cx, kk) >> sh, y = (uint32_t)rdlane((int)cy, kk) >> sh;
        if (state == 0) {
            const uint32_t dflag = (x >> 16) & 1u, iflag = x & 1u;
            if (MODE == kLocal && (dflag & iflag)) break;  // STOP: cost == 0 (:202)
            if (dflag) {
                state = 2;
            } else if (iflag) {
                state = 1;
            } else {
                // a whole M run at once: lane L holds step tt0 + L of this stripe, i.e. the
                // diagonal cell d = kk - L back (row r - d); the streak of M codes going down
                // from lane kk is the run (capped at the stripe's first row and the borders)
                const uint32_t v = (cx >> ((sh + (kk - (uint32_t)lane)) & 31u)) & 0x10001u;
                const uint32_t run = min(streak_down(ballot(v == 0u), kk), min(min(i, j), r + 1u));
                w.push('M', run);
                i -= run;
                j -= run;
            }
        } else if (state == 1) {
            w.push('I', 1);
            --j;
            state = (y & 1u) ? 1u : 0u;
        } else {
            w.push('D', 1);
            --i;
            state = ((y >> 16) & 1u) ? 2u : 0u;
        }
    }
    w.finish();
    *start_in_slot = cap - w.used;
    *len = w.used;
}

}  // namespace
}  // namespace ta
