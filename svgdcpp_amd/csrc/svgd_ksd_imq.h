// svgd_ksd_imq.h -- host-callable launchers of the kernelized Stein
// discrepancy pass under the inverse multiquadric kernel (svgd_ksd_imq.hip;
// internal).
//
// With centred coordinates xc, scores s = grad log p, q = 1 + a |x - y|^2 and
// k = q^(-1/2):
//   n_i = |xc_i|^2,  p_i = s_i.xc_i
//   r2  = max(n_i + n_j - 2 xc_i.xc_j, 0)
//   u_ij = k s_i.s_j + a k^3 (p_i + p_j - s_i.xc_j - xc_i.s_j + d) - 3 a^2 k^5 r2
//   u_ii = |s_i|^2 + a d  (taken as such, not through the Gram form)
//   row_i = (1/N) sum_j u_ij
// The centre, the row finish and the two fixed-tree sums are svgd_ksd.h's
// (launch_ksd_mean, launch_ksd_finish: the partials have its layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svgd_imq.h"

namespace svgd_amd {

constexpr int KSD_IMQ_WAVES = IMQ_WAVES; // waves per work-group, 16 particle rows each
constexpr int KSD_IMQ_ROWS_PER_WG = 16 * KSD_IMQ_WAVES;

// column record [xc (d) | 0 .. (KP) | s (d) | 0 .. (2 KP) | n | p | 0 ...];
// a padding record is all zeros.  2 KP + 2 doubles, as the IMQ phi record:
// the same stride (imq_rec_stride: the smallest odd multiple of 4 doubles
// that holds it, so the A-operand reads are conflict-free), the same padding
// and the same tile.
constexpr int ksd_imq_rec_stride(int d) { return imq_rec_stride(d); }
constexpr int ksd_imq_off_s(int d) { return imq_kp(d); }
constexpr int ksd_imq_off_n(int d) { return 2 * imq_kp(d); }
constexpr int ksd_imq_off_p(int d) { return 2 * imq_kp(d) + 1; }
inline int64_t ksd_imq_padded(int64_t n) { return imq_padded(n); }
// records per LDS tile of the pass at this d (64, or 32 where two 64-record
// buffers would leave room for one work-group per CU only; divides IMQ_PAD)
int ksd_imq_tile(int d);
inline int64_t ksd_imq_tiles(int d, int64_t n) { return ksd_imq_padded(n) / ksd_imq_tile(d); }

// work-groups of the pass for this d that one CU holds at a time (from the
// kernel's registers and LDS)
int ksd_imq_blocks_per_cu(int d);

// rec[j] for j < ksd_imq_padded(n) from X (n x d), its centre mu and the
// scores G (n x d); diag[j] = |s_j|^2 + a d (0 for padding records)
hipError_t launch_ksd_imq_prep(int d, const double *X, const double *G, const double *mu, double a,
                               int64_t n, double *rec, double *diag, hipStream_t stream);
// part[s][li] = the s-th of S tile ranges' sum of u_ij for the rows row0 + li,
// li < nrows, against all n columns (the column j = i counts diag[i]).
// 1 <= S <= ksd_imq_tiles(d, n); ldp >= nrows
hipError_t launch_ksd_imq_pass(int d, double a, const double *rec, const double *diag, int64_t row0,
                               int64_t nrows, int64_t n, int S, double *part, int64_t ldp,
                               hipStream_t stream);

} // namespace svgd_amd
