// svgd_glm.h -- host-callable launchers of the device GLM score (svgd_glm.hip;
// internal).
//
//   z_im = a_m . theta_i
//   G_i  = scale sum_{m in window} r(y_m, z_im) a_m - lambda theta_i
//   r    = y - sigma(z) (logistic),  r = y - z (Gaussian link)
// with scale = s M / B (host_glm.cpp has the model).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svgd_amd {

constexpr int GLM_TILE = 64;         // data records per LDS tile
constexpr int GLM_WAVES = 8;         // waves per work-group, 16 particle rows each
constexpr int GLM_ROWS_PER_WG = 16 * GLM_WAVES;
constexpr int GLM_FIN_THREADS = 256; // elements per block of the finish

// coordinates padded to the f64 MFMA's K
constexpr int glm_kp(int d) { return (d + 3) / 4 * 4; }
// record [a (d) | 0 .. (KP) | y | 0 ...]: stride (doubles) the smallest odd
// multiple of 4 that holds KP + 1 -- 32-byte aligned records for 16-byte
// copies from any window start, and the Gram A-operand read (lane (lo, hi) ->
// record lo, coordinate 4 kk + hi) touches 16 records x 4 coordinates in
// distinct banks
constexpr int glm_rec_stride(int d)
{
    const int q = glm_kp(d) / 4 + 1;
    return 4 * ((q & 1) ? q : q + 1);
}
// records of the device copy: whole tiles are read from any window start, so
// one tile of zero records (a = 0, y = 0) follows the data
inline int64_t glm_padded(int64_t m) { return m + GLM_TILE; }
// tiles of a window of `count` records
inline int64_t glm_tiles(int64_t count) { return (count + GLM_TILE - 1) / GLM_TILE; }

// work-groups of the pass for this (d, link) that one CU holds at a time
// (from the kernel's registers and LDS)
int glm_blocks_per_cu(int d, int link);

// part[s][li][c] = sum over the s-th of S tile ranges of the window
// [m0, m0 + count) of r(y_m, z_im) a_mc, for the particles li < nrows (rows of
// X, stride d); rec holds glm_padded(M) records, m0 + count <= M;
// 1 <= S <= glm_tiles(count); ldp >= nrows
hipError_t launch_glm_pass(int d, int link, const double *X, int64_t nrows, const double *rec,
                           int64_t m0, int64_t count, int S, double *part, int64_t ldp,
                           hipStream_t stream);
// G[li][c] = scale sum_s part[s][li][c] (s ascending) - lambda X[li][c]
hipError_t launch_glm_finish(int d, const double *X, int64_t nrows, const double *part, int S,
                             int64_t ldp, double scale, double lambda, double *G,
                             hipStream_t stream);

// ---- Hessian sum: -sum_i hess log p(theta_i) over `nrows` particles
//   H = scale sum_{m in window} W_m a_m a_m^T + lambda nrows I
//   W_m = sum_i w(a_m . theta_i), w = e / (1 + e)^2, e = exp(-|z|)  (logistic)
//   W_m = nrows                                                     (Gaussian link)
constexpr int GLM_GRAM_THREADS = 256;
constexpr int GLM_GRAM_BLOCK = 64;    // records per block of the weighted Gram
constexpr int GLM_GRAM_CHUNK = 64;    // records in LDS at a time
constexpr int GLM_GRAM_MAXGRID = 512; // work-groups, each a contiguous range of blocks
constexpr int GLM_GRAM_EPT = (64 * 65 / 2 + GLM_GRAM_THREADS - 1) / GLM_GRAM_THREADS; // triangle elements per thread

// record groups of the weight pass (one work-group's GLM_ROWS_PER_WG records)
inline int64_t glm_wgroups(int64_t count) { return (count + GLM_ROWS_PER_WG - 1) / GLM_ROWS_PER_WG; }
inline int64_t glm_gram_blocks(int64_t count) { return (count + GLM_GRAM_BLOCK - 1) / GLM_GRAM_BLOCK; }
inline int glm_gram_grid(int64_t count)
{
    const int64_t b = glm_gram_blocks(count);
    return (int)(b < GLM_GRAM_MAXGRID ? b : GLM_GRAM_MAXGRID);
}

// work-groups of the weight pass for this d that one CU holds at a time
int glm_wpass_blocks_per_cu(int d);

// W[m] = sum_i w(a_{m0+m} . theta_i) for m < count, over S ranges of the
// particles' tiles (1 <= S <= glm_tiles(nrows)) added in ascending order;
// wpart holds S * glm_wgroups(count) * GLM_ROWS_PER_WG doubles, W count
hipError_t launch_glm_weights(int d, const double *X, int64_t nrows, const double *rec, int64_t m0,
                              int64_t count, int S, double *wpart, double *W, hipStream_t stream);
// H (d x d, exactly symmetric) = scale sum_m W_m a_m a_m^T + diag I over the
// window, in blocks of GLM_GRAM_BLOCK records added in ascending order; W ==
// nullptr: every W_m = wconst; hpart holds glm_gram_grid(count) * d (d + 1) / 2
hipError_t launch_glm_wgram(int d, const double *rec, int64_t m0, int64_t count, const double *W,
                            double wconst, double scale, double diag, double *hpart, double *H,
                            hipStream_t stream);

} // namespace svgd_amd
