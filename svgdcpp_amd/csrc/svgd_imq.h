// svgd_imq.h -- host-callable launchers of the inverse multiquadric (IMQ) phi
// pass (svgd_imq.hip; internal).
//
//   k_ij  = (1 + a |x_i - x_j|^2)^(-1/2)
//   phi_i = (1/N) sum_j [ k_ij G_j + a k_ij^3 (x_i - x_j) ]
//         = (1/N) [ sum_j k_ij G_j + a ( xc_i sum_j k_ij^3 - sum_j k_ij^3 xc_j ) ]
// on the step's centred coordinates xc.  The arithmetic is fp64 whatever the
// context's dtype (as the KSD's and the GLM's): an SVGD_F32 context's IMQ phi
// is the fp64 one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svgd_amd {

constexpr int IMQ_WAVES = 8; // waves per work-group, 16 particle rows each
constexpr int IMQ_ROWS_PER_WG = 16 * IMQ_WAVES;
constexpr int IMQ_PAD = 64;  // records come in whole blocks of 64 (every LDS tile divides it)
constexpr int IMQ_FIN_THREADS = 256;

// coordinates padded to the f64 MFMA's K
constexpr int imq_kp(int d) { return (d + 3) / 4 * 4; }
// column record [xc (d) | 0 .. (KP) | w | G (d) | 0 .. (2 KP + 1) | n | 0 ...]
// with w = 1 and n = |xc|^2; a padding record is all zeros (w = 0 too).
// Stride (doubles): the smallest odd multiple of 4 that holds 2 KP + 2 --
// 32-byte aligned records, so a tile goes to LDS as straight 16-byte copies,
// and the Gram A-operand read (lane (lo, hi) -> record lo, coordinate
// 4 kk + hi) touches 16 records x 4 coordinates in distinct banks.
constexpr int imq_rec_stride(int d)
{
    const int q = (2 * imq_kp(d) + 2 + 3) / 4;
    return 4 * ((q & 1) ? q : q + 1);
}
constexpr int imq_off_w(int d) { return imq_kp(d); }
constexpr int imq_off_g(int d) { return imq_kp(d) + 1; }
constexpr int imq_off_n(int d) { return 2 * imq_kp(d) + 1; }
// records of the device copy: n rounded up to whole blocks of IMQ_PAD, the
// tail being padding records
inline int64_t imq_padded(int64_t n) { return (n + IMQ_PAD - 1) / IMQ_PAD * IMQ_PAD; }
// records per LDS tile of the pass at this d (64, or 32 where two 64-record
// buffers would leave room for one work-group per CU only)
int imq_tile(int d);
inline int64_t imq_tiles(int d, int64_t n) { return imq_padded(n) / imq_tile(d); }
// partial sums per row over j != i: [sum k G (d) | sum k^3 xc (d) | sum k^3]
constexpr int imq_part_width(int d) { return 2 * d + 1; }

// work-groups of the pass for this d that one CU holds at a time (from the
// kernel's registers and LDS)
int imq_blocks_per_cu(int d);

// rec[j] for j < imq_padded(n) from xc (stride xs, centred) and G (stride d)
hipError_t launch_imq_prep(int d, const double *xc, int xs, const double *G, int64_t n, double *rec,
                           hipStream_t stream);
// part[s][li][:] = the s-th of S tile ranges' sums for the rows row0 + li,
// li < nrows, against all n columns; a = *a_ptr.  1 <= S <= imq_tiles(d, n);
// ldp >= nrows
hipError_t launch_imq_pass(int d, const double *rec, const double *a_ptr, int64_t row0, int64_t nrows,
                           int64_t n, int S, double *part, int64_t ldp, hipStream_t stream);
// phi[li][c] = inv_n (G_i + sum_s part G + a (xc_i sum_s part k3 - sum_s part X)), s ascending
hipError_t launch_imq_finish(int d, const double *rec, const double *a_ptr, int64_t row0, int64_t nrows,
                             const double *part, int S, int64_t ldp, double inv_n, double *phi,
                             hipStream_t stream);

} // namespace svgd_amd
