// median_plan.cpp -- the median's host policy (host only, no GPU needed):
// see median_plan.h.
#include <algorithm>
#include <cmath>
#include <new>

#include "../../include/svgdcpp_amd/svgd_capi.h"
#include "median_plan.h"

namespace svgd_amd {

double BracketTracker::extrapolate(int order) const
{
    double p = order >= 3 && n >= 4 ? 4.0 * m[0] - 6.0 * m[1] + 4.0 * m[2] - m[3]
               : n >= 3            ? 3.0 * m[0] - 3.0 * m[1] + m[2]
                                   : 2.0 * m[0] - m[1];
    return p > 0.0 ? p : m[0];
}

// The selected lower key, the error of the prediction the last steps implied,
// the bracket's density.
void BracketTracker::record(uint64_t key_lo, uint64_t key_hi, uint64_t error, uint64_t bracket_lo_key,
                            uint64_t bracket_hi_key, uint64_t cand)
{
    const double ms = key_value(key_lo);
    if (error || !(ms > 0.0) || !std::isfinite(ms)) {
        restart();
        return;
    }
    // both extrapolations' errors (the ones this step's plan made, else from
    // the same history)
    if (n >= 2) {
        const double p = pq >= 0 ? pq : extrapolate(2);
        err[2] = err[1];
        err[1] = err[0];
        err[0] = std::fabs(ms - p) / ms;
        nerr = std::min(nerr + 1, 3);
    }
    if (n >= 4) {
        const double p = pc >= 0 ? pc : extrapolate(3);
        errc[2] = errc[1];
        errc[1] = errc[0];
        errc[0] = std::fabs(ms - p) / ms;
        nerrc = std::min(nerrc + 1, 3);
    }
    const double lo = key_value(bracket_lo_key);
    const double hi = bracket_hi_key >= 0x7ff0000000000000ull ? INFINITY : key_value(bracket_hi_key);
    dens = (std::isfinite(hi) && hi > lo) ? (double)cand / (hi - lo) : 0.0;
    // the averaged upper statistic: next to the lower one (1e-9 m at cfg3),
    // or across a gap of the distance list (two equal clusters, even n)
    const double m_hi = key_value(key_hi);
    gap = m_hi > ms && std::isfinite(m_hi) ? (m_hi - ms) / ms : 0.0;
    m[3] = m[2];
    m[2] = m[1];
    m[1] = m[0];
    m[0] = ms;
    n = std::min(n + 1, 4);
}

// The predicted band must not hold more candidates than the sampled
// bracket's would (band_samp: its expected share of the pairs).  Of the
// quadratic and the cubic extrapolation, the one whose half-width -- err_mult
// (cubic: twice that) x the largest of its last 3 relative errors -- is
// narrower.
bool BracketTracker::predict(double Mq, double band_samp, uint64_t *lo_key, uint64_t *hi_key, double *band)
{
    if (!allowed || n < 2 || !(dens > 0.0)) return false;
    const double m1 = m[0], m2 = m[1];
    pq = extrapolate(2);
    pc = n >= 4 ? extrapolate(3) : -1.0;
    double e = 0.0;
    if (nerr == 0) e = std::fabs(m1 - m2) / m1; // no error seen yet: the drift itself
    for (int k = 0; k < nerr; ++k) e = std::max(e, err[k]);
    double wp = err_mult * e, p = pq;
    if (pc >= 0 && nerrc == 3) {
        double ec = 0.0;
        for (int k = 0; k < 3; ++k) ec = std::max(ec, errc[k]);
        if (2.0 * err_mult * ec < wp) {
            wp = 2.0 * err_mult * ec;
            p = pc;
        }
    }
    const double w = std::max(wp, min_width);
    // the bracket has to hold both averaged statistics: the prediction follows
    // the lower one, the upper one lay `gap` above it.  Across a gap of the
    // list (two equal clusters, even n: the largest distance inside a cluster
    // and the smallest between the two) they move independently and no
    // extrapolation of the lower one places the upper one -- a bracket around
    // the lower one alone missed on every step, each redone: sample instead.
    if (!(w < 0.05) || !(gap < 0.05)) return false;
    const double lo = p * (1.0 - w), hi = p * (1.0 + gap) * (1.0 + w);
    const double b = dens * (hi - lo) / Mq;
    if (!(b <= band_samp)) return false;
    *lo_key = __builtin_bit_cast(uint64_t, lo);
    *hi_key = __builtin_bit_cast(uint64_t, hi) + 1;
    *band = b;
    pred = p;
    width = w;
    steps += 1;
    band_sum += b;
    return true;
}

RankPlan plan_ranks(int64_t n, int sim_world, int64_t sim_pairs)
{
    RankPlan r;
    int64_t rlo, rhi;
    r.navg = svgd_plan_median_ranks(n, &rlo, &rhi);
    if (sim_world > 1 && rlo >= 0) { // the same quantile of this rank's share of the pairs
        const int64_t d = rhi - rlo;
        rlo = (int64_t)((long double)rlo * (long double)sim_pairs / (long double)upper_pairs(n));
        rhi = rlo + d;
    }
    if (rlo >= 0) {
        r.sel_rank[r.nsel] = rlo;
        r.src_lo = r.nsel++;
    }
    if (rhi >= 0) {
        if (r.nsel == 1 && rhi == rlo) {
            r.src_hi = 0;
        } else {
            r.sel_rank[r.nsel] = rhi;
            r.src_hi = r.nsel++;
        }
    }
    if (r.navg == 1) r.src_hi = r.src_lo;
    return r;
}

SamplePlan plan_sample(int64_t M, bool tile_path, int64_t forced, bool multi, bool shard_sample,
                       int sim_world, double bracket_sigma)
{
    // sample size: the band it leaves costs the collect pass, sampling and
    // the two bracket passes cost ~S; measured optimum near M / 256 pairs
    // (cfg2, M = 1.3e8: 2^19 -> median 0.222 vs 0.262 ms at 2^22), capped
    // at 2^22 (cfg3, M = 2.1e9)
    // tile path: whole random 64 x 64 tiles (MFMA Gram, ~1/1000 of the
    // collect pass) instead of scattered pairs (2 random 8d-byte rows each).
    // Its keys come in correlated 4096-key tiles, so it keeps 2^22 (1024
    // tiles) whatever M: the bracket's sigma assumes many independent draws.
    int64_t S = forced > 0  ? forced
                : tile_path ? int64_t(1) << 22
                            : std::min<int64_t>(std::max<int64_t>(M / 256, int64_t(1) << 18), int64_t(1) << 22);
    if (multi && !shard_sample && forced <= 0)
        S = std::min<int64_t>(S, int64_t(1) << 20); // every rank draws all of it
    S = std::min<int64_t>(S, M);
    // whole-tile samples are correlated (a far particle shifts its tile's
    // 64 x 64 keys together): 3 sigma of S independent draws missed the
    // bracket on ~40 % of cfg5 steps (each miss: a second collect pass);
    // 12 measured none at no cost (the band stays ~1 % of the pairs)
    constexpr int64_t TILE_KEYS = SAMPLE_TILE * SAMPLE_TILE;
    auto sigma_of = [&](int64_t s) { return tile_path && s >= TILE_KEYS ? 4.0 * bracket_sigma : bracket_sigma; };
    SamplePlan p;
    // the share a tracked bracket is weighed against: that of this nominal
    // size (sample_ranks at q = 1/2), before a rank's share and whole tiles
    p.band_samp = (2.0 * sigma_of(S) * (std::sqrt((double)S * 0.25) + 1.0) + 3.0) / (double)S;
    if (sim_world > 1 && shard_sample) S = std::max<int64_t>(1, S / sim_world); // a rank's share
    p.tile_sample = tile_path && S >= TILE_KEYS;
    p.sigma = sigma_of(S);
    p.S = p.tile_sample ? S / TILE_KEYS * TILE_KEYS : S;
    return p;
}

SampleRanks sample_ranks(int64_t S, double qlo, double qhi, double sigma)
{
    const double sig_lo = std::sqrt((double)S * qlo * (1 - qlo)) + 1.0;
    const double sig_hi = std::sqrt((double)S * qhi * (1 - qhi)) + 1.0;
    double slo = std::floor(qlo * S - sigma * sig_lo) - 1;
    double shi = std::ceil(qhi * S + sigma * sig_hi) + 1;
    if (slo < 0) slo = 0;
    if (shi > S - 1) shi = (double)(S - 1);
    return SampleRanks{(uint64_t)slo, (uint64_t)shi, (shi - slo + 1.0) / (double)S};
}

SelState make_state(int nsel, const uint64_t *ranks, uint64_t lo_key, uint64_t hi_key, int known_from,
                    uint64_t prefix)
{
    SelState s{};
    s.nsel = nsel;
    s.rank[0] = ranks[0];
    s.rank[1] = nsel > 1 ? ranks[1] : 0;
    const uint64_t pm = known_from >= 64 ? 0ull : ~((1ull << known_from) - 1ull);
    s.prefix[0] = s.prefix[1] = prefix & pm;
    s.shift = known_from > RADIX_BITS ? known_from - RADIX_BITS : 0;
    s.width = known_from > RADIX_BITS ? RADIX_BITS : known_from;
    s.lo_key = lo_key;
    s.hi_key = hi_key;
    s.binv = (double)NBK / (double)(hi_key - lo_key);
    return s;
}

int known_from(uint64_t lo_key, uint64_t hi_key)
{
    if (!(hi_key > lo_key)) return 63;
    const uint64_t diff = lo_key ^ (hi_key - 1);
    const int k = diff ? 64 - __builtin_clzll(diff) : 0;
    return k > 63 ? 63 : k;
}

int64_t region_cap_predicted(double band, int64_t pairs_own, int64_t nregions)
{
    const int64_t total = (int64_t)(4.0 * band * (double)pairs_own) + 2048 * nregions;
    return std::max<int64_t>(1, total / nregions);
}

int64_t region_cap_sampled(const SamplePlan &s, int64_t cand_capacity, int64_t pairs_own, int64_t nregions)
{
    int64_t total = cand_capacity;
    if (total <= 0) {
        const double frac = (s.qhi - s.qlo) + 16.0 / std::sqrt((double)s.S) + 0.004;
        total = (int64_t)(2.0 * frac * (double)pairs_own) + 2048 * nregions;
    }
    return std::max<int64_t>(1, total / nregions);
}

int64_t spec_segment_cap(int64_t last_tot)
{
    int64_t cap = CAPR_MIN;
    while (cap < 2 * last_tot && cap < CAPG) cap <<= 1;
    return std::min<int64_t>(cap, CAPG);
}

} // namespace svgd_amd

using namespace svgd_amd;

extern "C" {

void *svgd_plan_tracker_new(double err_mult, double min_width)
{
    BracketTracker *t = new (std::nothrow) BracketTracker;
    if (t) {
        t->err_mult = err_mult;
        t->min_width = min_width;
    }
    return t;
}

void svgd_plan_tracker_free(void *t) { delete static_cast<BracketTracker *>(t); }
void svgd_plan_tracker_restart(void *t) { static_cast<BracketTracker *>(t)->restart(true); }
void svgd_plan_tracker_begin_step(void *t) { static_cast<BracketTracker *>(t)->begin_step(); }

int svgd_plan_tracker_predict(void *t, double pairs, double band_samp, uint64_t *lo_key, uint64_t *hi_key,
                              double *band, double *pred, double *width)
{
    BracketTracker *b = static_cast<BracketTracker *>(t);
    if (!b->predict(pairs, band_samp, lo_key, hi_key, band)) return 0;
    *pred = b->pred;
    *width = b->width;
    return 1;
}

void svgd_plan_tracker_record(void *t, uint64_t key_lo, uint64_t key_hi, int error, uint64_t bracket_lo_key,
                              uint64_t bracket_hi_key, uint64_t cand)
{
    static_cast<BracketTracker *>(t)->record(key_lo, key_hi, error ? 1 : 0, bracket_lo_key, bracket_hi_key, cand);
}

int64_t svgd_plan_median_sample(int64_t n, int tile_kernels, int64_t forced, int multi, int shard_sample,
                                int sim_world, double bracket_sigma, double *band_samp)
{
    const SamplePlan p = plan_sample(upper_pairs(n), tile_kernels && n / SAMPLE_TILE >= 2, forced, multi != 0,
                                     shard_sample != 0, sim_world, bracket_sigma);
    if (band_samp) *band_samp = p.band_samp;
    return p.S;
}

void svgd_plan_sample_ranks(int64_t S, double qlo, double qhi, double sigma, int64_t *slo, int64_t *shi,
                            double *band_est)
{
    const SampleRanks r = sample_ranks(S, qlo, qhi, sigma);
    *slo = (int64_t)r.slo;
    *shi = (int64_t)r.shi;
    if (band_est) *band_est = r.band_est;
}

int64_t svgd_plan_spec_cap(int64_t last_tot) { return spec_segment_cap(last_tot); }

} // extern "C"
