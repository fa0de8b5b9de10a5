// plan.cpp -- host-only work partitioning of the SVGD step (no GPU needed).
//
// Rows: particle i's phi_hat (SVGD.hpp:407-454) depends on every particle
// but is written only to row i, and the optimizer state is per particle
// (Adam.hpp:61-67), so ranks own contiguous row ranges.
//
// Median pairs: the reference takes the median over all n^2 distances
// (GaussianRBFKernel.hpp:185, 222-254): n diagonal zeros plus every
// off-diagonal distance twice.  Only the n(n-1)/2 upper-triangle values are
// visited, as block x block tiles (block = 256 on the row-stream path, 64 on
// the MFMA tile path): row block I pairs with itself (upper
// triangle inside the tile) and with column blocks I+1 .. I+H (mod nb),
// H = floor((nb-1)/2), plus I + nb/2 when nb is even and I < nb/2.  Every
// unordered pair of blocks then appears exactly once and every row block
// has the same number of tiles (+-1), so contiguous tile ranges balance the
// ranks.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/svgdcpp_amd/svgd_capi.h"
#include "plan.h"

namespace svgd_amd {

// Which phi kernel a context runs, decided once (svgd_capi.cpp allocates for
// it, run_phi launches it, svgd_phi_kernel_name prints it):
//   fp64 d <= 16: the row stream, or the symmetric pass where it pays
//   fp64 d > 16:  the fp64 tile kernel
//   F32:          k_phi_b3 (KP 32 / 64) or k_phi_f32s (KP 16) on 16-aligned
//                 rows, else the generic fp32 tile kernel
bool plan_phi(int dim, int64_t n, int dtype, int plan_world, int64_t row0, const Knobs &k,
              const PhiCaps &cap, PhiPlan *p)
{
    *p = PhiPlan{};
    p->dim = dim;
    if (dim <= 0 || !pick_tiles(dim, &p->KP, &p->NCB)) return false;
    const bool f32 = dtype == SVGD_F32;
    const bool rows = !f32 && cap.rows_kp > 0;
    // row stream: xc rows are the median records [xc | |xc|^2 | 0..]
    if (rows) p->KP = cap.rows_kp;
    // F32: the phi on the bf16 matrix cores where it applies (SVGD_PHI_B3=0:
    // the fp32-MFMA kernel k_phi_f32s)
    const bool b3 = f32 && cap.b3 && !k.phi_tile_generic && k.phi_b3.or_(1);
    // fp64 tiles and the bf16 F32 phi with d = 16 NCB: no V column of ones
    // (row sums on the VALU); SVGD_PHI_S1V=0 keeps the ones column (A/B knob)
    p->s1v = (!f32 || b3) && cap.tile_s1v && k.phi_s1v.or_(1);
    if (p->s1v) p->NCB = dim / 16;
    p->VW = 16 * p->NCB;
    // k_phi_b3 with one 16-row group per wave, or two (SVGD_PHI_B3_RG=2:
    // half its LDS reads and barriers per MFMA, a measured wash at cfg5 on the
    // power-limited chip, profiles/r06_b3_rg_il_ab.txt)
    if (b3) p->b3_rg = k.phi_b3_rg.or_(1);
    if (rows) {
        p->R = phi_rows_per_lane(dim);
        // 8-wave work-groups, 8192-entry table, columns split over the waves;
        // the 4-wave kernel serves the full-matrix scales (matrix_scale_plan)
        p->rows_kind = ROWS_8W;
        // symmetric phi pass: isotropic scales, d <= 8 (a pair feeds two
        // particles).  One rank: default since round 5 from N = 32768 up (with 16-byte record reads
        // cfg3 phi 3.59 -> 3.08 ms, step 4.12 -> 3.68 ms, cfg4 65.5 -> 56.5
        // ms; at cfg2, N = 16384, its extra launches outweigh the saving,
        // 0.200 vs 0.265 ms -- profiles/r05_sym_ab.txt.  SVGD_PHI_SYM=1 / 0
        // forces it on / off)
        // P > 1: rank r runs the units [U r / P, U (r+1) / P), sums every
        // particle's partials from them and a point-to-point exchange hands
        // each rank the pieces of its rows (sym_exchange).  Its phi saving
        // grows as N^2 / P, the exchange as N.  Round 5 (a reduce-scatter of
        // all N (d+1) sums, units not balanced at P = 8): default from N / P >=
        // 16384 (cfg3 shares P = 2 2.008 -> 1.875 ms, P = 4 1.066 -> 1.003, P =
        // 8 0.587 -> 0.582; cfg4 P = 8 7.92 -> 6.84 ms, profiles/r05_sim_sym.txt,
        // r05_cfg4_sim8_sym.txt).  Round 6: the padding-only sub-tiles left out
        // of the units (11 per work-group at cfg3 P = 8 instead of 11 or 12) and
        // ~2.5 MB sent per rank at cfg3 P = 8 instead of 4.1 MB in ring steps:
        // default from N / P >= 8192 (cfg3 at P = 8 included)
        const bool sym = cap.sym && (k.phi_sym.set ? k.phi_sym.v != 0
                                                   : n >= 32768 && n / (plan_world < 1 ? 1 : plan_world) >= 8192);
        p->path = sym ? PHI_SYM : PHI_ROWS;
    } else if (!f32) {
        p->path = PHI_TILE_F64;
    } else {
        // the streamed kernels' waves own 16-row groups of the padded rows: a
        // shard that starts elsewhere takes the generic kernel
        const bool streamed = cap.f32s && !k.phi_tile_generic && row0 % 16 == 0;
        p->path = !streamed ? PHI_TILE_F32 : b3 ? PHI_B3 : PHI_F32S;
    }
    return true;
}

void phi_plan_name(const PhiPlan &p, const PhiCaps &cap, char *buf, int len)
{
    const char *const tf[] = {"false", "true"};
    switch (p.path) {
    case PHI_SYM:
        snprintf(buf, (size_t)len, "k_phi_sym<%d>", p.dim);
        break;
    case PHI_ROWS: {
        // <D, R, NW, TABN, WC>, the geometry the launcher instantiates (built.h)
        const RowsGeom g = rows_geom(p.rows_kind);
        snprintf(buf, (size_t)len, "k_phi_rows<%d, %d, %d, %d, %d>", p.dim, p.R, g.NW, g.TABN, g.WC);
        break;
    }
    case PHI_B3:
        snprintf(buf, (size_t)len, "k_phi_b3<%d, %d, %d, %s, %d>", p.KP, p.NCB, cap.b3_waves, tf[p.s1v],
                 p.b3_rg);
        break;
    case PHI_F32S:
        snprintf(buf, (size_t)len, "k_phi_f32s<%d, %d>", p.KP, p.NCB);
        break;
    case PHI_TILE_F32:
    case PHI_TILE_F64:
        snprintf(buf, (size_t)len, "k_phi<%s, %d, %d, %d, %s, %s>", p.path == PHI_TILE_F64 ? "double" : "float",
                 p.KP, p.NCB, cap.tile_waves, tf[cap.tile_pre], tf[p.s1v]);
        break;
    }
}

} // namespace svgd_amd

extern "C" {

// Equal chunks of ceil(n/world) rows (the last ones may be short or empty),
// so the per-step all-gather is a single in-place ncclAllGather.
void svgd_plan_rows(int64_t n, int world, int rank, int64_t *row0, int64_t *row1)
{
    if (world < 1) world = 1;
    const int64_t chunk = (n + world - 1) / world;
    const int64_t r0 = chunk * rank, r1 = chunk * (rank + 1);
    *row0 = r0 < n ? r0 : n;
    *row1 = r1 < n ? r1 : n;
}

int svgd_plan_median_ranks(int64_t n, int64_t *rank_lo, int64_t *rank_hi)
{
    // full sorted list v of n^2 values; index k < n are the diagonal zeros,
    // index k >= n maps to upper-list rank (k - n) / 2.
    const int64_t total = n * n;
    auto map = [n](int64_t k) -> int64_t { return k < n ? -1 : (k - n) / 2; };
    if (total % 2 == 0) {
        *rank_lo = map(total / 2 - 1);
        *rank_hi = map(total / 2);
        return 2;
    }
    *rank_lo = *rank_hi = map(total / 2);
    return 1;
}

static int64_t tiles_total(int64_t nb) { return nb * (nb + 1) / 2; }

int64_t svgd_plan_pair_tiles(int64_t n, int block, int world, int rank)
{
    const int64_t nb = (n + block - 1) / block;
    const int64_t T = tiles_total(nb);
    if (world < 1) world = 1;
    return T * (rank + 1) / world - T * rank / world;
}

void svgd_plan_pair_tile(int64_t n, int block, int world, int rank, int64_t t,
                         int64_t *row_block, int64_t *col_block)
{
    const int64_t nb = (n + block - 1) / block;
    if (world < 1) world = 1;
    t += tiles_total(nb) * rank / world;
    const int64_t H = (nb - 1) / 2;
    int64_t I, slot;
    if ((nb & 1) == 0) {
        const int64_t c1 = H + 2, c2 = H + 1, half = nb / 2;
        if (t < half * c1) {
            I = t / c1;
            slot = t - I * c1;
        } else {
            const int64_t u = t - half * c1;
            I = half + u / c2;
            slot = u - (I - half) * c2;
        }
    } else {
        I = t / (H + 1);
        slot = t - I * (H + 1);
    }
    *row_block = I;
    *col_block = slot == 0 ? I : (I + slot) % nb;
}

// The symmetric phi pass's units: (tile, sub-tile) pairs of the tile plan in
// order, each tile's sub-tiles of `block / nsub` columns -- except the last
// column block's sub-tiles past n (all padding columns), which are not units
// at all: at N = 2^16 and 2^18 with 1536-row blocks the real units then
// divide evenly over 256 work-groups at P = 1, 2, 4 and 8.
static int64_t sym_cnt_h(int64_t nb, int64_t I) // tiles of row block I (slots 0 .. cnt-1)
{
    const int64_t H = (nb - 1) / 2;
    return ((nb & 1) == 0 && I < nb / 2) ? H + 2 : H + 1;
}
static int64_t sym_qlast(int64_t n, int block, int nsub, int64_t nb) // real sub-tiles of block nb - 1
{
    const int64_t sub = block / nsub, valid = n - (nb - 1) * block;
    return (valid + sub - 1) / sub;
}
// units of row block I: its tiles' sub-tiles, the one tile (if any) whose
// column block is the last one counting qlast
static int64_t sym_units_of(int64_t nb, int nsub, int64_t qlast, int64_t I)
{
    const int64_t cnt = sym_cnt_h(nb, I), s = nb - 1 - I; // slot of column block nb - 1
    return cnt * nsub - (s < cnt ? nsub - qlast : 0);
}

int64_t svgd_plan_sym_total(int64_t n, int block, int nsub)
{
    const int64_t nb = (n + block - 1) / block, ql = sym_qlast(n, block, nsub, nb);
    int64_t U = 0;
    for (int64_t I = 0; I < nb; ++I) U += sym_units_of(nb, nsub, ql, I);
    return U;
}

int svgd_plan_sym_unit(int64_t n, int block, int nsub, int64_t u, int64_t *tile, int64_t *q)
{
    const int64_t nb = (n + block - 1) / block, ql = sym_qlast(n, block, nsub, nb);
    int64_t t = 0;
    for (int64_t I = 0; I < nb; ++I) {
        const int64_t uI = sym_units_of(nb, nsub, ql, I), cnt = sym_cnt_h(nb, I);
        if (u >= uI) {
            u -= uI;
            t += cnt;
            continue;
        }
        for (int64_t slot = 0; slot < cnt; ++slot) {
            const int64_t J = (I + slot) % nb, nq = J == nb - 1 ? ql : nsub;
            if (u < nq) {
                *tile = t + slot;
                *q = u;
                return 0;
            }
            u -= nq;
        }
    }
    *tile = *q = -1;
    return -1;
}

// The symmetric phi pass's unit plan (svgd_capi.cpp, k_phi_sym / k_sym_finish).
int64_t svgd_plan_sym_units(int64_t n, int block, int nsub, int world, int rank, int grid,
                            int64_t *u0, int64_t *u1, int *blkg, int *rbase, int64_t *Ia, int64_t *Ib)
{
    if (world < 1) world = 1;
    const int64_t nb = (n + block - 1) / block;
    const int64_t U = svgd_plan_sym_total(n, block, nsub);
    *u0 = U * rank / world;
    *u1 = U * (rank + 1) / world;
    const int64_t V = *u1 - *u0;
    for (int64_t P = 0; P < nb; ++P) {
        blkg[2 * P] = INT32_MAX;
        blkg[2 * P + 1] = -1;
    }
    *Ia = 0;
    *Ib = -1;
    if (V <= 0 || grid < 1) {
        for (int64_t P = 0; P < nb; ++P) rbase[P] = 0;
        return 0;
    }
    // work-group g takes the contiguous units [u0 + V g / G, u0 + V (g+1) / G)
    // (G <= V: none is empty) and visits the row blocks of their tiles
    int64_t J;
    for (int64_t g = 0; g < grid; ++g) {
        const int64_t a = *u0 + V * g / grid, b = *u0 + V * (g + 1) / grid;
        if (b <= a) continue;
        int64_t I0, I1, ta, tb, q;
        svgd_plan_sym_unit(n, block, nsub, a, &ta, &q);
        svgd_plan_sym_unit(n, block, nsub, b - 1, &tb, &q);
        svgd_plan_pair_tile(n, block, 1, 0, ta, &I0, &J);
        svgd_plan_pair_tile(n, block, 1, 0, tb, &I1, &J);
        for (int64_t P = I0; P <= I1; ++P) {
            if ((int)g < blkg[2 * P]) blkg[2 * P] = (int)g;
            if ((int)g > blkg[2 * P + 1]) blkg[2 * P + 1] = (int)g;
        }
    }
    // each row block's row-sum records contiguous, in work-group order
    int64_t nrec = 0;
    for (int64_t P = 0; P < nb; ++P) {
        rbase[P] = (int)nrec;
        if (blkg[2 * P + 1] >= blkg[2 * P]) nrec += blkg[2 * P + 1] - blkg[2 * P] + 1;
    }
    int64_t ta, tb, q;
    svgd_plan_sym_unit(n, block, nsub, *u0, &ta, &q);
    svgd_plan_sym_unit(n, block, nsub, *u1 - 1, &tb, &q);
    svgd_plan_pair_tile(n, block, 1, 0, ta, Ia, &J);
    svgd_plan_pair_tile(n, block, 1, 0, tb, Ib, &J);
    return nrec;
}

// The particles rank src's symmetric-pass units add to: a cyclic run of
// blocks from its first row block Ia through Ib + the largest slot (SM - 1 =
// (nb - 1) / 2 + 1, the even-nb extra slot included: a hull), intersected
// with dst's rows.
void svgd_plan_sym_exchange(int64_t n, int block, int nsub, int world, int src, int dst, int64_t *r0,
                            int64_t *r1)
{
    if (world < 1) world = 1;
    int64_t d0, d1;
    svgd_plan_rows(n, world, dst, &d0, &d1);
    *r0 = *r1 = d0;
    const int64_t nb = (n + block - 1) / block;
    const int64_t U = svgd_plan_sym_total(n, block, nsub);
    const int64_t u0 = U * src / world, u1 = U * (src + 1) / world;
    if (u1 <= u0 || d1 <= d0) return;
    int64_t Ia, Ib, J, ta, tb, q;
    svgd_plan_sym_unit(n, block, nsub, u0, &ta, &q);
    svgd_plan_sym_unit(n, block, nsub, u1 - 1, &tb, &q);
    svgd_plan_pair_tile(n, block, 1, 0, ta, &Ia, &J);
    svgd_plan_pair_tile(n, block, 1, 0, tb, &Ib, &J);
    const int64_t len = Ib - Ia + 1 + (nb - 1) / 2 + 1; // blocks Ia .. Ib + SM - 1
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    auto meet = [&](int64_t a, int64_t b) { // particles [a, b) against dst's rows
        a = a > d0 ? a : d0;
        b = b < d1 ? b : d1;
        if (a < b) {
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
    };
    if (len >= nb) {
        meet(0, n);
    } else if (Ia + len <= nb) {
        meet(Ia * block, (Ia + len) * block < n ? (Ia + len) * block : n);
    } else {
        meet(Ia * block, n);
        meet(0, (Ia + len - nb) * block);
    }
    if (lo < hi) {
        *r0 = lo;
        *r1 = hi;
    }
}

// Bucket of each selection from the all-reduced key-range bucket counts
// (NBK buckets, ascending key order): ranks[s] is the rank among the
// candidates; writes the bucket and the rank within it, and the total count
// of the distinct selected buckets.  Returns -1 if a rank lies past the
// counted candidates.
int svgd_plan_bucket_select(const unsigned long long *counts, int nb, int nsel,
                            const int64_t *ranks, int *bsel, int64_t *rank_in, int64_t *total)
{
    if (nsel < 1 || nsel > 2) return -1;
    int64_t cum = 0;
    bsel[0] = bsel[1] = -1;
    for (int b = 0; b < nb; ++b) {
        const int64_t c = (int64_t)counts[b];
        for (int s = 0; s < nsel; ++s)
            if (bsel[s] < 0 && ranks[s] >= cum && ranks[s] < cum + c) {
                bsel[s] = b;
                rank_in[s] = ranks[s] - cum;
            }
        cum += c;
    }
    for (int s = 0; s < nsel; ++s)
        if (bsel[s] < 0) return -1;
    if (nsel == 1) {
        bsel[1] = bsel[0];
        rank_in[1] = rank_in[0];
    }
    *total = (int64_t)counts[bsel[0]] + (bsel[1] != bsel[0] ? (int64_t)counts[bsel[1]] : 0);
    return 0;
}

} // extern "C"
