// svgd_mmd.h -- host-callable launchers of the maximum mean discrepancy pass
// between two point sets (svgd_mmd.hip; internal).
//
// With both sets centred on one point mu (z~ = z - mu), n = |z~|^2 and
//   r2 = max(n_i + n_j - 2 x~_i.z~_j, 0)
//   RBF  k = exp(-a r2)            IMQ  k = (1 + a r2)^(-1/2)
// a pass writes, for a window of rows of one set and the columns of another
// (or the same) set, the row sums  sum_j k(x_i, z_j)  in S column-tile ranges.
// In a same-set pass the column j = i counts exactly 1, by index.  The centre
// and the fixed-order finish are svgd_ksd.h's (launch_ksd_mean,
// launch_ksd_finish: the partials have its layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svgd_imq.h"

namespace svgd_amd {

constexpr int MMD_WAVES = IMQ_WAVES; // waves per work-group, 16 rows each
constexpr int MMD_ROWS_PER_WG = 16 * MMD_WAVES;
constexpr int MMD_TILE = 64;         // records per LDS tile, and the padding unit

// point record [z~ (d) | 0 .. (KP) | n | 0 ...], KP = imq_kp(d); a padding
// record is all zeros.  Stride (doubles): the smallest odd multiple of 4 that
// holds KP + 1 (the rule of imq_rec_stride: 32-byte aligned records, and the
// MFMA operand read of 16 records x 4 coordinates touches distinct banks).
constexpr int mmd_rec_stride(int d)
{
    const int q = (imq_kp(d) + 1 + 3) / 4;
    return 4 * ((q & 1) ? q : q + 1);
}
constexpr int mmd_off_n(int d) { return imq_kp(d); }
// records of a set's device copy: whole tiles, the tail being padding records
inline int64_t mmd_padded(int64_t n) { return (n + MMD_TILE - 1) / MMD_TILE * MMD_TILE; }
inline int64_t mmd_tiles(int64_t n) { return mmd_padded(n) / MMD_TILE; }

// work-groups of the pass for this d and kernel that one CU holds at a time
// (from the kernel's registers and LDS)
int mmd_blocks_per_cu(int d, int kernel);

// rec[j] for j < mmd_padded(n) from Z (n x d, row-major) and the centre mu
hipError_t launch_mmd_prep(int d, const double *Z, const double *mu, int64_t n, double *rec,
                           hipStream_t stream);
// part[s][li] = the s-th of S column-tile ranges' sum of k(row row0 + li, col j)
// over j < ncol, li < nrows.  rowrec: the records of the row set (row0 + nrows
// within it); colrec: the mmd_padded(ncol) records of the column set; same:
// the two are one set (the column j = row0 + li counts 1).
// 1 <= S <= mmd_tiles(ncol); ldp >= nrows
hipError_t launch_mmd_pass(int d, int kernel, double a, const double *rowrec, int64_t row0, int64_t nrows,
                           const double *colrec, int64_t ncol, bool same, int S, double *part,
                           int64_t ldp, hipStream_t stream);

} // namespace svgd_amd
