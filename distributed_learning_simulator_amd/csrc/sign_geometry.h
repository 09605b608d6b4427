// The sign vote's launch geometry (csrc/sign.hip), for host and device: how many
// waves sweep a model, how many 64-parameter vote groups a lane owns (G), and the
// range of groups each wave owns.  launch_vote, k_sign_vote and the host-only
// queries dls_sign_vote_geometry / dls_sign_vote_wave_ranges all call the two
// functions below, so what the host tests pin is what the kernel runs.
//
// Invariant: every wave's range is at most 64 G groups long and G <= kVoteG, so
// the wave's 64 lanes x G groups cover the whole range.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DLS_HD __host__ __device__ __forceinline__
#else
#define DLS_HD inline
#endif

namespace dls {

constexpr int kVoteG = 4;       // widest G (registers: single-buffered 8-client batches)
constexpr int kVoteAlign = 8;   // wide ranges start on 8 groups = 128 bytes of a plane row

struct VoteGeometry {
    int64_t nwaves;
    int G;    // vote groups per lane, 1..kVoteG
    int wpb;  // waves per block
};

// vote_groups: DLS_SIGN_WORDS(P) / 2 (whole 256-parameter tiles).  wide_counters:
// the counter width class CB > 12, which keeps one group per lane (registers).
// wpc: waves per CU on large models (DLS_VOTE_WPC; 0: fixed ranges, one wave per
// block); wpb: waves per block of the wide layout (DLS_VOTE_WPB).  Host only.
inline VoteGeometry vote_geometry(int64_t vote_groups, int cus, bool wide_counters, int wpc,
                                  int wpb) {
    if (cus < 1) cus = 1;
    // Large models: wpc waves per CU, each a contiguous range of R groups,
    // 2-4 groups per lane (each wave streams R x 16 B of every client row:
    // multi-KB pieces measured 12 % faster than 1 KB at P = 11.2M).  Small
    // models: R = 64, 1 group per lane, double-buffered batches.
    VoteGeometry g{(vote_groups + 63) / 64, 1, 1};
    if (wide_counters) return g;
    constexpr int64_t kMaxRange = 64 * kVoteG;
    if (wpc > 0) {
        // exactly wpc waves per CU, near-equal ranges of up to 64 G groups; a
        // range is at most ceil(vote_groups / waves) groups plus the kVoteAlign - 1
        // its start is aligned down by (vote_wave_range)
        int64_t waves = (int64_t)wpc * cus;
        int64_t r = (vote_groups + waves - 1) / waves + (kVoteAlign - 1);
        if (r > kMaxRange) {
            // models past 64 kVoteG groups per wave (P > ~16.7M on 256 CUs, e.g.
            // VGG-16): a multiple m of wpc waves per CU, so that every wave keeps
            // the wide layout instead of G = 1.  m = ceil(r / 256) can leave r at
            // 257..263 (the alignment slack is not divided by m): m grows until the
            // range fits 64 kVoteG groups.
            const int64_t base = waves;
            int64_t m = (r + kMaxRange - 1) / kMaxRange;
            do {
                waves = base * m++;
                r = (vote_groups + waves - 1) / waves + (kVoteAlign - 1);
            } while (r > kMaxRange);
        }
        if (r > 64) {
            g.nwaves = waves;
            g.G = (int)((r + 63) / 64);
            g.wpb = wpb;
        }
    } else if ((vote_groups + kMaxRange - 1) / kMaxRange >= 512) {
        // fixed ranges, one wave per block: ceil(vote_groups / nwaves) is at most
        // 64 kVoteG - (kVoteAlign - 1), which leaves room for the alignment
        constexpr int64_t kRange = kMaxRange - (kVoteAlign - 1);
        g.nwaves = (vote_groups + kRange - 1) / kRange;
        g.G = kVoteG;
    }
    return g;
}

// Wave `wave` of nwaves owns the groups [wlo, whi): nwaves near-equal contiguous
// ranges (sizes differ by at most one group; with G > 1, by up to 8: every range
// starts on a multiple of 8 groups = 128 bytes, and the last ends at vote_groups).
DLS_HD void vote_wave_range(int64_t wave, int64_t vote_groups, int64_t nwaves, int G, int64_t &wlo,
                            int64_t &whi) {
    wlo = wave * vote_groups / nwaves;
    whi = (wave + 1) * vote_groups / nwaves;
    if (G > 1) {
        wlo &= ~(int64_t)(kVoteAlign - 1);
        whi = wave + 1 == nwaves ? vote_groups : whi & ~(int64_t)(kVoteAlign - 1);
    }
}

}  // namespace dls

#undef DLS_HD
