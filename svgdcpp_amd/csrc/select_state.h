// select_state.h -- the median select's state, capacities and pinned slots
// shared by the kernels, the launchers and the host policy (internal; host
// only, no HIP: median_plan.cpp and the CPU tests include it too).
#pragma once
#include <stdint.h>

namespace svgd_amd {

constexpr int RADIX_BITS = 11;
constexpr int RADIX = 1 << RADIX_BITS;

// Device-resident state of the (dual) radix select over 63-bit keys
// (non-negative doubles as uint64).  Digits from the top: bits 62..52,
// 51..41, 40..30, 29..19, 18..8, 7..0.
struct SelState {
    uint64_t prefix[2];   // resolved high bits of the two selected keys
    uint64_t rank[2];     // remaining rank within the current prefix
    uint64_t lo_key;      // candidate bracket [lo_key, hi_key)
    uint64_t hi_key;
    int32_t nsel;         // 1 or 2 active selections
    int32_t shift;        // shift of the current digit
    int32_t width;        // width of the current digit
    int32_t pass;         // digits resolved so far
    int32_t error;        // rank outside the histogram (should not happen)
    int32_t pad_;
    double binv;          // key-range buckets of [lo_key, hi_key): NBK / (hi - lo)
    int32_t bsel[2];      // bucket of each selection (bucket select path)
};

// Key-range buckets of the candidate bracket: bucket(key) = floor((key - lo)
// * binv), clamped to [0, NBK) -- monotone in the key, so buckets are
// contiguous key ranges.  The collect pass histograms them, so one all-reduce
// (counts + buckets) tells every rank which bucket holds each order statistic.
constexpr int NBK = 2048;
// per-rank capacity of the compacted selected-bucket keys (gathered over
// ranks).  At cfg4 (N = 262144, 3.4e10 pairs) a sampled bracket's bucket
// holds ~25k keys on one rank (2^22-pair sample) and ~100k at P > 1 (2^20):
// 16384 sent every cfg4 step down the radix path, so it never speculated
// and never tracked its bracket.  The synchronous path's all-gather moves
// the step's own total, the speculative one the adaptive spec cap.
constexpr int CAPG = 262144;
// per-rank segment capacity of the speculative bucket select: adaptive
// (median_plan.cpp spec_segment_cap: twice the last step's selected-bucket
// total, rounded up to a power of two, within [CAPR_MIN, CAPG]); the
// all-gather (P > 1) moves cap + 1 keys per rank.  At cfg3 a bucket holds ~3k
// keys: a fixed 4096 made ~1 in 5 early steps fail the plan (each failure
// redoes the step); the selection reads only the keys present.
constexpr int CAPR_MIN = 4096;

// cnt = [below, candidates, overflowed regions, NBK bucket counts (zero without
// bpart), lo_key, hi_key]: the first 3 + NBK entries are sums over ranks.
constexpr int CNT_LO = 3 + NBK, CNT_HI = 4 + NBK, CNT_LEN = 5 + NBK;

// Slots of the pinned host buffer the selection publishes a step's bracket and
// keys in (svgd_ctx::h_trk, TRK_LEN uint64): written by the device plan
// (block 0 of launch_compact_buckets with PlanArgs::trk) and by
// launch_select_small, read by the host's bracket tracking.
enum TrkSlot {
    TRK_LO = 0,    // this step's bracket [lo_key, hi_key) ...
    TRK_HI = 1,
    TRK_BELOW = 2, // ... the keys below it and its candidates (all ranks)
    TRK_CAND = 3,
    TRK_KEY0 = 4,  // the selected keys (lower, upper order statistic)
    TRK_KEY1 = 5,
    TRK_ERR = 6,   // the selection's error flag
    TRK_TOT = 7,   // the selected buckets' keys (the next step's segment size)
    TRK_SEQ = 8,   // the speculative step's sequence number, stored last
    TRK_LEN = 16,
};

} // namespace svgd_amd
