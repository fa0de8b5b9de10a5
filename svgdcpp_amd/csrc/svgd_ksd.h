// svgd_ksd.h -- host-callable launchers of the kernelized Stein discrepancy
// pass (svgd_ksd.hip; internal).
//
// With centred coordinates xc, scores s = grad log p and k = exp(-a |x - y|^2):
//   v_i = s_i - 2a xc_i,  n_i = |xc_i|^2,  c_i = 2a s_i.xc_i - 4a^2 n_i
//   u_ij = exp(-a max(n_i + n_j - 2 xc_i.xc_j, 0)) (v_i.v_j + 4a^2 xc_i.xc_j + c_i + c_j + 2ad)
//   u_ii = |s_i|^2 + 2ad  (taken as such, not through the Gram form)
//   row_i = (1/N) sum_j u_ij
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svgd_amd {

constexpr int KSD_MEAN_BLOCKS = 256; // column-sum partials of the centring
constexpr int KSD_TILE = 64;         // rows / columns per tile of the d > 16 kernel
constexpr int KSD_FIN_THREADS = 256; // rows per block of the row finish

// padded particle count of the KSD work arrays: whole column chunks / tiles
// may be read past n (the padding columns contribute exactly 0)
inline int64_t ksd_padded(int64_t n) { return (n + KSD_TILE - 1) / KSD_TILE * KSD_TILE + KSD_TILE; }
// record stride (doubles) of the d <= 16 kernel: [xc (d) | v (d) | e_j | c_j + 2ad]
constexpr int ksd_rec_stride(int d) { return 2 * d + 2; }
// coordinate stride of the k-major copies of the d > 16 kernel
inline int ksd_kp(int d) { return (d + 15) / 16 * 16; }
// rows per lane of the d <= 16 kernel: as many as keep the row operands
// (2 d R doubles), the pair temporaries and one column record inside 256
// VGPRs at two waves per SIMD
constexpr int ksd_rows_per_lane(int d) { return d <= 6 ? 4 : d <= 8 ? 3 : d <= 14 ? 2 : 1; }
// rows per work-group of the pair kernels
constexpr int ksd_rows_per_wg(int d) { return d <= 16 ? 256 * ksd_rows_per_lane(d) : KSD_TILE; }

// work-groups of the pair kernel for this d that one CU holds at a time (from
// the kernel's registers and LDS): the caller sizes its column splits so the
// grid fills the device a whole number of times
int ksd_blocks_per_cu(int d);

// mu = column means of X (n x d), in a fixed order: partial holds
// KSD_MEAN_BLOCKS x d doubles
hipError_t launch_ksd_mean(const double *X, int64_t n, int d, double *partial, double *mu,
                           hipStream_t stream);
// Per particle j < np (padding j >= n: zero operands, nrm = +inf):
//   d <= 16: rec[j] (stride ksd_rec_stride(d));  d > 16: xt / vt [k][np] for k < ksd_kp(d)
//   nrm[j] = n_j, cvec[j] = c_j, diag[j] = |s_j|^2 + 2ad
hipError_t launch_ksd_prep(const double *X, const double *G, const double *mu, double a, int64_t n,
                           int64_t np, int d, double *rec, double *xt, double *vt, double *nrm,
                           double *cvec, double *diag, hipStream_t stream);
// part[s][li] = sum over the s-th of S column ranges of u_ij, for the rows
// li < nrows of this rank (global row row0 + li); ldp >= nrows
hipError_t launch_ksd_pairs(int d, double a, const double *rec, const double *xt, const double *vt,
                            const double *nrm, const double *cvec, const double *diag, int64_t row0,
                            int64_t nrows, int64_t n, int64_t np, int S, double *part, int64_t ldp,
                            hipStream_t stream);
// rows[li] = (1/N) sum_s part[s][li] (s ascending); bpart[b] = [sum of rows,
// sum of diag] over block b's rows by a fixed tree; then out[0..1] = the sums
// of bpart in a fixed order.  nblk = ceil(nrows / KSD_FIN_THREADS) (>= 1).
hipError_t launch_ksd_finish(const double *part, int S, int64_t ldp, int64_t nrows, double inv_n,
                             const double *diag_rows, double *rows, double *bpart, double *out,
                             hipStream_t stream);

} // namespace svgd_amd
