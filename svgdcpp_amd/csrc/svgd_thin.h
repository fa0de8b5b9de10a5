// svgd_thin.h -- launchers of the Stein thinning kernels (svgd_thin.hip;
// internal).  Geometry: one thread per candidate, THIN_WG candidates per
// work-group, every per-candidate array padded to thin_padded(n).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svgd_amd {

constexpr int THIN_WG = 256;
// candidates with padding; the kernels index them with an int
constexpr int64_t THIN_MAX_N = 0x7fffffff - THIN_WG;
constexpr int64_t thin_padded(int64_t n) { return (n + THIN_WG - 1) / THIN_WG * THIN_WG; }
constexpr int64_t thin_groups(int64_t n) { return thin_padded(n) / THIN_WG; }
// (value, index) partial slots: two parities of thin_groups(n), then the one
// slot k_thin_select writes
constexpr int64_t thin_part_slots(int64_t n) { return 2 * thin_groups(n) + 1; }

// The work arrays of one selection (all device memory):
struct ThinArgs {
    const double *X, *G; // n x d particles and scores, row-major
    double *xs;          // 2d x thin_padded(n): x then s, coordinate-major
    double *diag, *acc;  // thin_padded(n): u_jj, the running sum of u(pi_s, j)
    double *pval;        // thin_part_slots(n) objective minima ...
    int *pidx;           // ... and where they are attained
    int64_t *idx;        // m picks
    double *S;           // m running sums S_t
};

// xs, diag, acc = 0 and the work-groups' minima of obj_1 = u_jj / 2 into
// parity 0 of the partials
hipError_t launch_thin_prep(bool imq, int d, int64_t n, double a, const ThinArgs &w, hipStream_t stream);
// the m picks: m launches of k_thin_pick (each reduces the last one's
// partials first), or with `select` m pairs k_thin_select, k_thin_pick
hipError_t launch_thin_picks(bool imq, int d, int64_t n, double a, int64_t m, bool select,
                             const ThinArgs &w, hipStream_t stream);

} // namespace svgd_amd
