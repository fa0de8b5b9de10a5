// median_plan.h -- the median's host policy (internal; host only, no HIP).
//
// Which order statistics a step selects, the bracket sample and its ranks,
// the bracket tracked from the last medians, the candidate regions' and the
// speculative segment's capacities, the select state the device starts from:
// pure arithmetic, made here without a context, a HIP call or an environment
// read.  svgd_capi.cpp owns one BracketTracker and one SamplePlan per context
// and launches what they decide; the CPU tests and the sanitizer driver run
// the same code (the svgd_plan_* entry points at the end of median_plan.cpp).
#pragma once
#include <stdint.h>

#include "select_state.h"

namespace svgd_amd {

inline int64_t upper_pairs(int64_t n) { return n * (n - 1) / 2; }
inline double key_value(uint64_t k) { return __builtin_bit_cast(double, k); }

// Bracket tracking (speculative steps): the median of D^2 moves smoothly
// from step to step, so the collect pass's bracket is predicted from the last
// selected keys (quadratic or cubic extrapolation, half-width a multiple of
// the largest of the last 3 prediction errors) instead of a sample and its
// two radix passes.  The selection stays exact; a bracket that misses the
// order statistics is a failed plan, and the step is redone with a sample.
struct BracketTracker {
    bool allowed = true;     // SVGD_TRACK_BRACKET=0 disables
    double err_mult = 4.0;   // SVGD_TRACK_ERR_MULT: half-width / recent error (set at creation)
    double min_width = 2e-5; // SVGD_TRACK_MIN_WIDTH: relative half-width floor
    // the history
    double m[4] = {0, 0, 0, 0}; // last selected D^2 (lower order statistic), newest first
    int n = 0;
    double err[3] = {0, 0, 0};  // recent relative errors of the quadratic extrapolation
    int nerr = 0;
    double errc[3] = {0, 0, 0}; // ... and of the cubic one (4 medians)
    int nerrc = 0;
    double dens = 0; // candidates per unit of D^2 in the last bracket (all ranks)
    double gap = 0;  // (upper - lower selected D^2) / lower of the last selection
    // this step
    double pq = -1, pc = -1; // its two extrapolations (< 0: none)
    double pred = -1;        // its predicted median D^2 (< 0: sampled bracket)
    double width = 0;        // the predicted bracket's relative half-width
    // counters (svgd_get_diagnostics): predicted steps, the ones whose bracket
    // missed, the sum of their predicted band shares
    int64_t steps = 0, miss = 0;
    double band_sum = 0;

    // The history restarts: the medians alone (a selection that left no keys
    // or flagged an error; the recent errors still bound the next widths), or
    // with the errors too (new particles).
    void restart(bool errors_too = false)
    {
        n = 0;
        if (errors_too) nerr = nerrc = 0;
    }
    // a step begins: no prediction made yet
    void begin_step() { pred = pq = pc = -1; }
    // The next median D^2 from the last 2, 3 or 4: linear, quadratic (order 2:
    // on SVGD trajectories its errors are ~5x below the linear one's) or cubic
    // (order 3: through 4 points; on the bench trajectories another 2-5x below
    // the quadratic one's while the median still moves fast, noisier once it
    // settles -- profiles/r06_track_predictor.txt)
    double extrapolate(int order = 2) const;
    // A resolved selection -> the history: the selected keys (lower, upper
    // order statistic) and the selection's error flag, the bracket it was
    // taken from and its candidates (all ranks).
    void record(uint64_t key_lo, uint64_t key_hi, uint64_t error, uint64_t bracket_lo_key,
                uint64_t bracket_hi_key, uint64_t cand);
    // The predicted bracket [*lo_key, *hi_key) for this step and its expected
    // share *band of the Mq pairs (counted in steps / band_sum), or false:
    // sample it.
    bool predict(double Mq, double band_samp, uint64_t *lo_key, uint64_t *hi_key, double *band);
    // the step's plan failed: a miss if its bracket was the predicted one
    void failed() { miss += pred >= 0 ? 1 : 0; }
};

// The distinct non-negative upper-list ranks a step selects
// (svgd_plan_median_ranks; a rank of -1 is a diagonal zero and selects
// nothing) and where the averaged statistics come from: sel_rank[src_lo],
// sel_rank[src_hi] (-1: zero), navg of them.  sim_world > 1 (measurement
// contexts): the same quantile of one rank's share of sim_pairs pairs.
struct RankPlan {
    int nsel = 0;
    int64_t sel_rank[2] = {0, 0};
    int src_lo = -1, src_hi = -1, navg = 1;
};
RankPlan plan_ranks(int64_t n, int sim_world, int64_t sim_pairs);

// The bracket sample of a step over M pairs.
constexpr int64_t SAMPLE_TILE = 64; // tile path: whole 64 x 64 tiles of keys are drawn
struct SamplePlan {
    int64_t S = 0;            // keys drawn (a multiple of the tile when tile_sample)
    bool tile_sample = false; // whole random tiles, else scattered pairs
    double sigma = 0;         // sample-quantile standard deviations either side
    double band_samp = 0;     // its bracket's expected share of the pairs at q = 1/2
    // the step's draw from it (median_begin): the target quantiles, and
    // whether ranks draw disjoint parts of it (then `local` keys here)
    double qlo = 0, qhi = 0;
    bool shard = false;
    int64_t local = 0;
};
// tile_path: the tile kernels' median with at least two full blocks;
// forced: a set sample size (0: automatic); multi: more than one rank shares
// the step (a communicator, or a measurement context).
SamplePlan plan_sample(int64_t M, bool tile_path, int64_t forced, bool multi, bool shard_sample,
                       int sim_world, double bracket_sigma);

// Sample ranks bracketing the target quantiles (sigma sample-quantile
// standard deviations either side) and the bracket's expected share of the
// pairs.
struct SampleRanks {
    uint64_t slo, shi;
    double band_est;
};
SampleRanks sample_ranks(int64_t S, double qlo, double qhi, double sigma);

// A fresh select state.  Bits >= known_from of every selected key are
// already known to equal those of `prefix` (64: nothing known; keys are
// < 2^63); the first digit is the RADIX_BITS below them.
SelState make_state(int nsel, const uint64_t *ranks, uint64_t lo_key, uint64_t hi_key,
                    int known_from = 63, uint64_t prefix = 0);
// every candidate key lies in [lo_key, hi_key): the bit from which their
// leading bits agree (63: nothing known, or an empty bracket)
int known_from(uint64_t lo_key, uint64_t hi_key);

// Keys per candidate region of the collect pass: for a predicted bracket of
// expected share `band` (4x the band), and for a sampled one (2x its target
// span plus the sample's resolution; cand_capacity > 0: that total instead).
int64_t region_cap_predicted(double band, int64_t pairs_own, int64_t nregions);
int64_t region_cap_sampled(const SamplePlan &s, int64_t cand_capacity, int64_t pairs_own,
                           int64_t nregions);
// per-rank segment capacity of a speculative step: twice the last selection's
// keys, a power of two in [CAPR_MIN, CAPG]
int64_t spec_segment_cap(int64_t last_tot);

} // namespace svgd_amd
