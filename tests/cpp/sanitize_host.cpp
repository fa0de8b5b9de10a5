// Host-code sanitizer driver (AddressSanitizer + UndefinedBehaviorSanitizer):
// the planners (plan.cpp, the phi plan included, and the median's host policy
// median_plan.cpp), the host Gaussian-sum models (host_models.cpp) and
// the CPU oracle (oracle/svgd_oracle.c, test infrastructure) built with
// -fsanitize=address,undefined and exercised with cross-checks
// (`make sanitize`, run by tests/test_sanitize.py).  The HIP-side host code
// (svgd_capi.cpp, ctx_*.cpp, hostcomm.cpp) drives the GPU and is covered by the -m gpu
// tests instead: GPU sanitizers are not available on this pool.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <vector>

#include "../../include/svgdcpp_amd/svgd_capi.h"
#include "../../svgdcpp_amd/csrc/plan.h"
#include "../../svgdcpp_amd/csrc/median_plan.h"

extern "C" {
void or_fill_splitmix(double *X, long count, double scale, uint64_t seed);
void or_median_scale(const double *X, int d, long n, double *a_out, double *med_out);
double or_upper_sqdist_kth(const double *X, int d, long n, long k);
void or_phi_rows(const double *X, const double *G, int d, long n, double a, long i0, long i1,
                 double *phi, double *K, double *Kg);
void or_logp_grad_gmm(const double *X, int d, long n, int k, const double *mu,
                      const double *covs, double *G);
void or_neg_hess_sum_gmm(const double *X, int d, long n, int k, const double *mu,
                         const double *covs, double *H);
void or_phi_matrix_rows(const double *X, const double *G, int d, long n, const double *M,
                        long i0, long i1, double *out);
}

static int failures = 0;
#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++failures;                                                                       \
        }                                                                                     \
    } while (0)

static void test_plan()
{
    // row shards tile [0, n) exactly
    for (int64_t n : {1, 2, 7, 64, 1000, 65537})
        for (int world : {1, 2, 3, 8}) {
            int64_t next = 0;
            for (int r = 0; r < world; ++r) {
                int64_t a, b;
                svgd_plan_rows(n, world, r, &a, &b);
                CHECK(a == next && b >= a && b <= n);
                next = b;
            }
            CHECK(next == n);
        }
    // median ranks of the n^2 list
    for (int64_t n : {1, 2, 3, 4, 5, 100, 101}) {
        int64_t lo, hi;
        const int navg = svgd_plan_median_ranks(n, &lo, &hi);
        CHECK(navg == 1 || navg == 2);
        CHECK(lo <= hi);
    }
    // pair tiles: every unordered block pair exactly once over the ranks
    for (int64_t n : {5, 300, 1000})
        for (int block : {64, 256})
            for (int world : {1, 2, 3}) {
                const int64_t nb = (n + block - 1) / block;
                std::vector<int> seen(nb * nb, 0);
                int64_t tot = 0;
                for (int r = 0; r < world; ++r) {
                    const int64_t t = svgd_plan_pair_tiles(n, block, world, r);
                    tot += t;
                    for (int64_t k = 0; k < t; ++k) {
                        int64_t I, J;
                        svgd_plan_pair_tile(n, block, world, r, k, &I, &J);
                        CHECK(I >= 0 && I < nb && J >= 0 && J < nb);
                        const int64_t a = I < J ? I : J, b = I < J ? J : I;
                        seen[a * nb + b] += 1;
                    }
                }
                CHECK(tot == nb * (nb + 1) / 2);
                for (int64_t a = 0; a < nb; ++a)
                    for (int64_t b = a; b < nb; ++b) CHECK(seen[a * nb + b] == 1);
            }
    // bucket select against a direct scan
    std::vector<unsigned long long> cnt(2048);
    uint64_t s = 12345;
    for (auto &c : cnt) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        c = (s >> 33) % 7;
    }
    int64_t total = 0;
    for (auto c : cnt) total += (int64_t)c;
    for (int64_t r0 : {int64_t(0), total / 3, total - 1}) {
        const int64_t ranks[2] = {r0, r0 + (r0 + 1 < total ? 1 : 0)};
        int bsel[2];
        int64_t rin[2], tot = 0;
        CHECK(svgd_plan_bucket_select(cnt.data(), 2048, 2, ranks, bsel, rin, &tot) == 0);
        for (int q = 0; q < 2; ++q) {
            int64_t cum = 0;
            for (int b = 0; b < bsel[q]; ++b) cum += (int64_t)cnt[b];
            CHECK(cum + rin[q] == ranks[q] && rin[q] < (int64_t)cnt[bsel[q]]);
        }
    }
    const int64_t bad[2] = {total, total};
    int bsel[2];
    int64_t rin[2], tot = 0;
    CHECK(svgd_plan_bucket_select(cnt.data(), 2048, 2, bad, bsel, rin, &tot) == -1);
}

// The entries of one list of built.h that the enumerated plans name.
template <auto &LIST> struct Named {
    bool hit[std::size(LIST)] = {};
    template <class T> void name(const T &v) // (a) a plan names built instantiations only
    {
        for (size_t i = 0; i < std::size(LIST); ++i)
            if (LIST[i] == v) {
                hit[i] = true;
                return;
            }
        CHECK(!"the plan names an instantiation that is not in the built list");
    }
    void all_named(const char *list) const // (b) nothing is built that no plan names
    {
        for (size_t i = 0; i < std::size(LIST); ++i)
            if (!hit[i]) {
                std::fprintf(stderr, "built, but named by no plan: %s entry %zu\n", list, i);
                ++failures;
            }
    }
};

// Every kernel instantiation a plan stands for -- the phi kernel, and the
// median pair passes a context of that plan launches -- against the lists the
// launchers dispatch over.
struct NamedKernels {
    Named<svgd_amd::ROW_DIMS> rows[2], pair_rows; // k_phi_rows by RowsKind; k_pair_rows
    Named<svgd_amd::SYM_DIMS> sym;
    Named<svgd_amd::TILES_F64> f64;
    Named<svgd_amd::TILES_F32> f32;
    Named<svgd_amd::TILES_S1V> s1v_f64, s1v_f32, b3_s1v[std::size(svgd_amd::B3_RG)];
    Named<svgd_amd::TILES_F32S> f32s;
    Named<svgd_amd::TILES_B3> b3[std::size(svgd_amd::B3_RG)];
    Named<svgd_amd::PAIR_KP_F64> pair_f64; // k_pair_tiles<double>
    Named<svgd_amd::PAIR_KP_F32> pair_f32; // k_pair_tiles<float>, k_pair_tcol / k_pair_tcol3

    void name(const svgd_amd::PhiPlan &p, int dtype)
    {
        using namespace svgd_amd;
        const TileClass t{p.KP, p.NCB};
        switch (p.path) {
        case PHI_SYM:
            sym.name(p.dim);
            break;
        case PHI_ROWS:
            CHECK(p.R == phi_rows_per_lane(p.dim)); // the only R built
            rows[p.rows_kind].name(p.dim);
            break;
        case PHI_TILE_F64:
            p.s1v ? s1v_f64.name(t) : f64.name(t);
            break;
        case PHI_TILE_F32:
            p.s1v ? s1v_f32.name(t) : f32.name(t);
            break;
        case PHI_F32S:
            CHECK(!p.s1v);
            f32s.name(t);
            break;
        case PHI_B3:
            CHECK(built(B3_RG, p.b3_rg));
            for (size_t i = 0; i < std::size(B3_RG); ++i)
                if (B3_RG[i] == p.b3_rg) p.s1v ? b3_s1v[i].name(t) : b3[i].name(t);
            break;
        }
        if (p.rows())
            pair_rows.name(p.dim);
        else if (dtype == SVGD_F32)
            pair_f32.name(p.KP);
        else
            pair_f64.name(p.KP);
    }
    void all_named() const
    {
        rows[svgd_amd::ROWS_4W].all_named("ROW_DIMS (k_phi_rows, 4 waves)");
        rows[svgd_amd::ROWS_8W].all_named("ROW_DIMS (k_phi_rows, 8 waves)");
        pair_rows.all_named("ROW_DIMS (k_pair_rows)");
        sym.all_named("SYM_DIMS");
        f64.all_named("TILES_F64");
        f32.all_named("TILES_F32");
        s1v_f64.all_named("TILES_S1V (k_phi<double>)");
        s1v_f32.all_named("TILES_S1V (k_phi<float>)");
        f32s.all_named("TILES_F32S");
        for (auto &b : b3) b.all_named("TILES_B3, for one of B3_RG");
        for (auto &b : b3_s1v) b.all_named("TILES_S1V (k_phi_b3), for one of B3_RG");
        pair_f64.all_named("PAIR_KP_F64");
        pair_f32.all_named("PAIR_KP_F32");
    }
};

// plan_phi over every dimension, both dtypes, three world sizes and the A/B
// knobs, with the capability flags the library uses (built.h: phi_caps over
// the lists the launchers instantiate).  Both ways: every plan, its
// matrix-scale variant and the median passes they imply name a built
// instantiation, and every built instantiation is named by some plan.
static void test_phi_plan()
{
    using namespace svgd_amd;
    std::vector<Knobs> settings(9);
    settings[1].phi_tile_generic = true;
    settings[2].phi_b3 = {true, 0};
    settings[3].phi_s1v = {true, 0};
    settings[4].phi_b3_rg = {true, 2};
    settings[5].phi_sym = {true, 0};
    settings[6].phi_sym = {true, 1};
    settings[7].phi_sym = {true, 2};
    // (two knobs at once: the ones-column k_phi_b3 of d = 32 / 64 with two row groups)
    settings[8].phi_s1v = {true, 0};
    settings[8].phi_b3_rg = {true, 2};
    PhiPlan p;
    char name[96];
    const PhiCaps c8 = phi_caps(8, false);
    CHECK(c8.rows_kp == 12 && c8.sym);
    CHECK(plan_phi(8, 65536, SVGD_F64, 1, 0, settings[0], c8, &p));
    phi_plan_name(p, c8, name, (int)sizeof name);
    CHECK(std::strcmp(name, "k_phi_sym<8>") == 0);
    phi_plan_name(matrix_scale_plan(p), c8, name, (int)sizeof name);
    CHECK(std::strcmp(name, "k_phi_rows<8, 4, 4, 4096, 1>") == 0);
    CHECK(plan_phi(8, 333, SVGD_F64, 1, 0, settings[0], c8, &p));
    phi_plan_name(p, c8, name, (int)sizeof name);
    CHECK(std::strcmp(name, "k_phi_rows<8, 4, 8, 8192, 8>") == 0);
    CHECK(!plan_phi(65, 333, SVGD_F64, 1, 0, settings[0], phi_caps(65, false), &p));
    CHECK(!plan_phi(0, 333, SVGD_F64, 1, 0, settings[0], phi_caps(0, false), &p));
    NamedKernels named;
    for (int d = 1; d <= 64; ++d) {
        int KP = 0, NCB = 0;
        CHECK(pick_tiles(d, &KP, &NCB));
        {
            // what the lists must amount to, stated by dimension
            const PhiCaps cap = phi_caps(d, false);
            CHECK(cap.rows_kp == (d <= 16 ? ((d + 1 + 3) / 4) * 4 : 0));
            CHECK(cap.sym == (d <= 8));
            CHECK(cap.tile_s1v == (d > 16 && d % 16 == 0));
            CHECK(cap.f32s == (KP % 16 == 0));
            CHECK(cap.b3 == (KP == 32 || KP == 64));
        }
        for (int dtype : {SVGD_F64, SVGD_F32})
            for (int world : {1, 2, 8})
                for (int64_t n : {int64_t(333), int64_t(65536)})
                    for (int rank = 0; rank < world; ++rank)
                        for (const Knobs &k : settings) {
                            int64_t r0, r1;
                            svgd_plan_rows(n, world, rank, &r0, &r1);
                            const bool f32 = dtype == SVGD_F32;
                            const PhiCaps cap = phi_caps(d, f32);
                            CHECK(cap.tile_waves == (f32 ? 4 : 8) && cap.tile_pre == !f32 && cap.b3_waves == 8);
                            CHECK(plan_phi(d, n, dtype, world, r0, k, cap, &p));
                            named.name(p, dtype);
                            named.name(matrix_scale_plan(p), dtype);
                            char name[8]; // (shorter than any name: the formatter must truncate)
                            phi_plan_name(p, cap, name, (int)sizeof name);
                            CHECK(std::strlen(name) == sizeof name - 1 && std::strncmp(name, "k_phi", 5) == 0);
                            CHECK(p.dim == d && p.KP >= d && p.NCB >= 1 && p.NCB <= 5);
                            CHECK(p.VW == 16 * p.NCB);
                            // S1V exactly where d = 16 NCB; else room for the column of ones
                            CHECK(p.s1v == (d == 16 * p.NCB));
                            CHECK(p.VW >= d + (p.s1v ? 0 : 1));
                            if (p.s1v) CHECK(cap.tile_s1v && !k.phi_s1v.set && (!f32 || cap.b3));
                            if (!f32 && d <= 16) {
                                CHECK(p.rows() && p.KP == cap.rows_kp && p.R == (d <= 8 ? 4 : 2) && p.rows_kind == ROWS_8W);
                                if (p.path == PHI_SYM) CHECK(d <= 8 && k.phi_sym.or_(1) != 0);
                                if (k.phi_sym.set) CHECK((p.path == PHI_SYM) == (d <= 8 && k.phi_sym.v != 0));
                                else CHECK((p.path == PHI_SYM) == (d <= 8 && n >= 32768 && n / world >= 8192));
                            } else if (!f32) {
                                CHECK(p.path == PHI_TILE_F64 && p.KP == KP);
                            } else {
                                CHECK(p.KP == KP);
                                CHECK(p.path == PHI_TILE_F32 || p.path == PHI_F32S || p.path == PHI_B3);
                                if (p.path != PHI_TILE_F32) CHECK(r0 % 16 == 0 && !k.phi_tile_generic && cap.f32s);
                                if (p.path == PHI_B3) CHECK(cap.b3 && k.phi_b3.or_(1) != 0);
                                if (p.path == PHI_TILE_F32) CHECK(r0 % 16 != 0 || k.phi_tile_generic || !cap.f32s);
                                CHECK(p.b3_rg == (cap.b3 && !k.phi_tile_generic && k.phi_b3.or_(1) ? k.phi_b3_rg.or_(1) : 1));
                            }
                            CHECK(p.fused() == (p.path != PHI_TILE_F64 && p.path != PHI_TILE_F32));
                        }
    }
    named.all_named();
}

static uint64_t key_of(double x) { return __builtin_bit_cast(uint64_t, x); }

// The median's host policy (median_plan.cpp), at the edges of its arithmetic.
static void test_median_plan()
{
    using namespace svgd_amd;
    // the tracker through 0 .. 6 records of a smooth history: a prediction
    // from the second record on, holding the next median
    const double pairs = 1e8;
    for (int nrec = 0; nrec <= 6; ++nrec) {
        BracketTracker t;
        double m = 4.0;
        for (int k = 0; k < nrec; ++k, m *= 0.99) {
            t.begin_step();
            t.record(key_of(m), key_of(m), 0, key_of(0.99 * m), key_of(1.01 * m), 1000000);
            CHECK(t.n == (k + 1 < 4 ? k + 1 : 4) && t.dens > 0 && t.gap == 0);
        }
        CHECK(t.nerr == (nrec >= 2 ? (nrec - 2 < 3 ? nrec - 2 : 3) : 0));
        CHECK(t.nerrc == (nrec >= 4 ? nrec - 4 : 0));
        uint64_t lo = 0, hi = 0;
        double band = 0;
        t.begin_step();
        const bool go = t.predict(pairs, 1.0, &lo, &hi, &band);
        CHECK(go == (nrec >= 2));
        if (go) {
            CHECK(lo <= key_of(m) && key_of(m) < hi && band > 0 && t.pred > 0 && t.width >= t.min_width);
            CHECK(t.steps == 1 && t.band_sum == band);
            t.failed();
            CHECK(t.miss == 1);
            // a non-finite or a flagged record: the medians are forgotten, the errors kept
            const int nerr = t.nerr;
            t.record(key_of(INFINITY), key_of(INFINITY), 0, lo, hi, 10);
            CHECK(t.n == 0 && t.nerr == nerr);
            CHECK(!t.predict(pairs, 1.0, &lo, &hi, &band));
            t.record(key_of(m), key_of(m), 0, key_of(0.99 * m), key_of(1.01 * m), 10);
            t.record(key_of(m), key_of(m), 1, key_of(0.99 * m), key_of(1.01 * m), 10);
            CHECK(t.n == 0);
            t.restart(true);
            CHECK(t.nerr == 0 && t.nerrc == 0);
        } else {
            t.failed(); // (a sampled bracket's failure is no miss)
            CHECK(t.miss == 0 && t.steps == 0);
        }
        // a bracket open to the infinity pattern (and beyond): no density, no prediction
        for (uint64_t top : {0x7ff0000000000000ull, ~0ull}) {
            t.record(key_of(m), key_of(m), 0, key_of(0.99 * m), top, 1000000);
            CHECK(t.dens == 0);
            t.begin_step();
            CHECK(!t.predict(pairs, 1.0, &lo, &hi, &band));
        }
    }
    // make_state at the edges of the known prefix
    const uint64_t ranks[2] = {5, 9}, prefix = 0xfedcba9876543210ull;
    for (int kf : {0, 11, 12, 63, 64}) {
        const SelState s = make_state(2, ranks, 0, ~0ull, kf, prefix);
        CHECK(s.nsel == 2 && s.rank[0] == 5 && s.rank[1] == 9);
        CHECK(s.width == (kf > RADIX_BITS ? RADIX_BITS : kf) && s.shift == (kf > RADIX_BITS ? kf - RADIX_BITS : 0));
        CHECK(s.shift + s.width == kf);
        CHECK(s.prefix[0] == (kf >= 64 ? 0 : prefix >> kf << kf) && s.prefix[1] == s.prefix[0]);
        CHECK(s.binv > 0);
    }
    CHECK(make_state(1, ranks, 0, 0).rank[1] == 0);
    CHECK(known_from(0, 0) == 63 && known_from(8, 8) == 63 && known_from(8, 9) == 0);
    CHECK(known_from(8, 10) == 1 && known_from(0, ~0ull) == 63 && known_from(0x4000, 0x4100) == 8);
    // the rank plan: n = 0 .. 3 (diagonal zeros among the averaged), even and odd pair counts
    for (int64_t n : {0, 1, 2, 3, 4, 5, 6, 7, 100, 101}) {
        const RankPlan r = plan_ranks(n, 1, 0);
        int64_t lo, hi;
        CHECK(r.navg == svgd_plan_median_ranks(n, &lo, &hi));
        CHECK(r.nsel >= 0 && r.nsel <= 2 && r.src_lo < r.nsel && r.src_hi < r.nsel);
        CHECK((r.src_lo < 0) == (lo < 0) && (r.src_hi < 0) == (hi < 0));
        if (r.src_lo >= 0) CHECK(r.sel_rank[r.src_lo] == lo);
        if (r.src_hi >= 0) CHECK(r.sel_rank[r.src_hi] == hi);
        if (r.nsel == 2) CHECK(r.sel_rank[0] < r.sel_rank[1]);
        // (n = 0, an empty list, names rank 0 as svgd_plan_median_ranks does: no context has n < 1)
        for (int q = 0; q < r.nsel && n > 0; ++q) CHECK(r.sel_rank[q] >= 0 && r.sel_rank[q] < upper_pairs(n));
        if (n >= 4) { // one of 4 ranks' share: the same quantile (rounded down), the same spacing
            const int64_t M = upper_pairs(n), Ms = M / 4;
            const RankPlan q = plan_ranks(n, 4, Ms);
            CHECK(q.nsel == r.nsel);
            CHECK(q.sel_rank[0] * M <= r.sel_rank[0] * Ms && (q.sel_rank[0] + 1) * M > r.sel_rank[0] * Ms);
            CHECK(q.sel_rank[q.nsel - 1] - q.sel_rank[0] == r.sel_rank[r.nsel - 1] - r.sel_rank[0]);
        }
    }
    CHECK(plan_ranks(1, 1, 0).nsel == 0 && plan_ranks(1, 1, 0).src_lo == -1 && plan_ranks(1, 1, 0).src_hi == -1);
    CHECK(plan_ranks(2, 1, 0).nsel == 1 && plan_ranks(3, 1, 0).nsel == 1 && plan_ranks(4, 1, 0).nsel == 2);
    // the sample plan with fewer pairs than the sample (and the usual sizes)
    for (bool tiles : {false, true})
        for (int64_t M : {int64_t(1), int64_t(4095), int64_t(5000), int64_t(1) << 27, int64_t(1) << 31}) {
            for (bool multi : {false, true}) {
                const SamplePlan p = plan_sample(M, tiles, 0, multi, false, 1, 3.0);
                CHECK(p.S >= 1 && p.S <= M && p.S <= (int64_t(1) << (multi ? 20 : 22)));
                CHECK(p.tile_sample == (tiles && M >= 4096) && (!p.tile_sample || p.S % 4096 == 0));
                CHECK(p.sigma == (p.tile_sample ? 12.0 : 3.0) && p.band_samp > 0);
                const SampleRanks r = sample_ranks(p.S, 0.5, 0.5, p.sigma);
                CHECK(r.slo <= r.shi && (int64_t)r.shi <= p.S - 1 && r.band_est > 0 && r.band_est <= 1.0);
                if (!p.tile_sample && M >= (int64_t(1) << 27)) CHECK(std::fabs(r.band_est - p.band_samp) * p.S <= 2.0);
                SamplePlan s = p;
                s.qlo = s.qhi = 0.5;
                CHECK(region_cap_sampled(s, 0, 1 << 20, 64) >= 2048 && region_cap_sampled(s, 10, 1 << 20, 64) == 1);
            }
            CHECK(plan_sample(M, tiles, 777, true, false, 1, 3.0).S == (M < 777 ? M : 777));
            CHECK(plan_sample(M, tiles, 0, true, true, 4, 3.0).S >= 1);
        }
    CHECK(region_cap_predicted(0.0, 1 << 20, 64) == 2048 && region_cap_predicted(1e-3, 1 << 20, 1) == 4194 + 2048);
    CHECK(spec_segment_cap(0) == CAPR_MIN && spec_segment_cap(2048) == 4096 && spec_segment_cap(2049) == 8192);
    CHECK(spec_segment_cap(CAPG) == CAPG && spec_segment_cap(int64_t(1) << 40) == CAPG);
    // the handle the Python tests drive
    void *h = svgd_plan_tracker_new(4.0, 2e-5);
    CHECK(h != nullptr);
    uint64_t lo, hi;
    double band, pred, width;
    svgd_plan_tracker_begin_step(h);
    CHECK(svgd_plan_tracker_predict(h, pairs, 1.0, &lo, &hi, &band, &pred, &width) == 0);
    svgd_plan_tracker_record(h, key_of(2.0), key_of(2.0), 0, key_of(1.9), key_of(2.1), 1000);
    svgd_plan_tracker_record(h, key_of(2.01), key_of(2.01), 0, key_of(1.9), key_of(2.1), 1000);
    svgd_plan_tracker_begin_step(h);
    CHECK(svgd_plan_tracker_predict(h, pairs, 1.0, &lo, &hi, &band, &pred, &width) == 1);
    CHECK(pred == 2.0 * 2.01 - 2.0 && width > 0 && lo < hi);
    svgd_plan_tracker_restart(h);
    CHECK(svgd_plan_tracker_predict(h, pairs, 1.0, &lo, &hi, &band, &pred, &width) == 0);
    svgd_plan_tracker_free(h);
    double bs = 0;
    int64_t a, b;
    CHECK(svgd_plan_median_sample(3, 0, 0, 0, 0, 1, 3.0, &bs) == 3 && bs > 0);
    svgd_plan_sample_ranks(3, 0.5, 0.5, 3.0, &a, &b, nullptr);
    CHECK(a == 0 && b == 2);
    CHECK(svgd_plan_spec_cap(5000) == 16384);
}

static void test_models_vs_oracle()
{
    const int d = 5, k = 3;
    const long n = 257;
    std::vector<double> X(n * d), mu(k * d), cov(k * d * d, 0.0);
    or_fill_splitmix(X.data(), n * d, 3.0, 0x5EED);
    or_fill_splitmix(mu.data(), k * d, 2.0, 0x5EEE);
    for (int c = 0; c < k; ++c)
        for (int r = 0; r < d; ++r) {
            cov[(c * d + r) * d + r] = 1.0 + 0.25 * c;
            if (r + 1 < d) cov[(c * d + r) * d + r + 1] = cov[(c * d + r + 1) * d + r] = 0.1;
        }
    void *m = nullptr;
    CHECK(svgd_model_create(&m, d, k, mu.data(), cov.data()) == SVGD_OK);
    std::vector<double> G(n * d), Gr(n * d), H(d * d), Hr(d * d);
    CHECK(svgd_model_logp_grad(m, X.data(), n, G.data()) == SVGD_OK);
    or_logp_grad_gmm(X.data(), d, n, k, mu.data(), cov.data(), Gr.data());
    double err = 0;
    for (long e = 0; e < n * d; ++e) err = std::fmax(err, std::fabs(G[e] - Gr[e]));
    CHECK(err <= 1e-12);
    CHECK(svgd_model_neg_hess_sum(m, X.data(), n, H.data()) == SVGD_OK);
    or_neg_hess_sum_gmm(X.data(), d, n, k, mu.data(), cov.data(), Hr.data());
    err = 0;
    for (int e = 0; e < d * d; ++e) err = std::fmax(err, std::fabs(H[e] - Hr[e]) / (1 + std::fabs(Hr[e])));
    CHECK(err <= 1e-10);
    CHECK(svgd_model_destroy(m) == SVGD_OK);
    m = nullptr;
    CHECK(svgd_model_create(&m, d, k, mu.data(), nullptr) == SVGD_ERR_ARG && m == nullptr);
}

static void test_oracle_paths()
{
    const int d = 3;
    const long n = 97;
    std::vector<double> X(n * d), G(n * d), ph(n * d), pm(n * d);
    or_fill_splitmix(X.data(), n * d, 1.0, 7);
    or_fill_splitmix(G.data(), n * d, 1.0, 8);
    double a = 0, med = 0;
    or_median_scale(X.data(), d, n, &a, &med);
    CHECK(med > 0 && std::isfinite(a));
    // the median of the n^2 list is the mean of two upper-list order statistics here
    const double lo = or_upper_sqdist_kth(X.data(), d, n, 0);
    CHECK(lo >= 0);
    std::vector<double> K(n * n), Kg(n * n * d);
    or_phi_rows(X.data(), G.data(), d, n, a, 0, n, ph.data(), K.data(), Kg.data());
    CHECK(K[0] == 1.0); // the diagonal
    // the matrix form with M = a I equals the isotropic phi
    std::vector<double> M(d * d, 0.0);
    for (int r = 0; r < d; ++r) M[r * d + r] = a;
    or_phi_matrix_rows(X.data(), G.data(), d, n, M.data(), 0, n, pm.data());
    double err = 0;
    for (long e = 0; e < n * d; ++e) err = std::fmax(err, std::fabs(ph[e] - pm[e]));
    CHECK(err <= 1e-13);
}

int main()
{
    test_plan();
    test_phi_plan();
    test_median_plan();
    test_models_vs_oracle();
    test_oracle_paths();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("sanitize_host: all checks passed\n");
    return 0;
}
