// built.h -- what the kernel translation units instantiate (internal; host
// only, no HIP).
//
// The lists below are the ones the launchers hand to dispatch() (dispatch.h),
// so a kernel is built exactly when its entry stands here, and everything that
// asks "is there a kernel for this?" -- phi_caps, the plan, the printed kernel
// name, the host sanitizer driver -- reads the same lists.
#pragma once
#include <stddef.h>

#include <iterator>

namespace svgd_amd {

// ---- the row stream (fp64, d <= 16) ---------------------------------------
inline constexpr int ROW_DIMS[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
constexpr int ROWS_MAX_D = ROW_DIMS[std::size(ROW_DIMS) - 1];
// rows per lane of k_phi_rows (register budget): the only R built for d
constexpr int phi_rows_per_lane(int d) { return d <= 8 ? 4 : 2; }
// k_phi_rows<D, R(D), NW, TABN, WC> is built in two geometries
struct RowsGeom {
    int NW, TABN, WC; // waves per work-group, exp table entries, column groups over the waves
    constexpr int rows_per_wg(int R) const { return NW / WC * 64 * R; }
};
enum RowsKind {
    ROWS_4W, // 4 waves, each its own 64 R rows: the full-matrix scales' kernel (signature rows)
    ROWS_8W, // 8 waves over one 64 R-row group, the mask-free 8192-entry table: every other step
};
constexpr RowsGeom rows_geom(RowsKind k) { return k == ROWS_8W ? RowsGeom{8, 8192, 8} : RowsGeom{4, 4096, 1}; }
// record strides (doubles) of the row-stream path: phi records
// [xc | G - 2a xc | c | 0..] and median records [xc | |xc|^2 | 0..]
constexpr int phi_rec_stride(int d) { return ((2 * d + 1 + 7) / 8) * 8; }
constexpr int med_rec_stride(int d) { return ((d + 1 + 3) / 4) * 4; }
constexpr int med_f32_stride(int d) { return ((d + 1 + 7) / 8) * 8; }
// the symmetric pass k_phi_sym<D>
inline constexpr int SYM_DIMS[] = {1, 2, 3, 4, 5, 6, 7, 8};

// ---- the MFMA tile kernels ------------------------------------------------
// A tile class: xc stride KP, NCB 16-column blocks of V.
struct TileClass {
    int KP, NCB;
    constexpr bool operator==(const TileClass &o) const { return KP == o.KP && NCB == o.NCB; }
};
// (KP, NCB) of dimension d with V's column of ones; false above 64
constexpr bool pick_tiles(int d, int *KP, int *NCB)
{
    constexpr struct {
        int maxd;
        TileClass t;
    } tab[] = {{4, {4, 1}},   {8, {8, 1}},   {12, {12, 1}}, {15, {16, 1}}, {16, {16, 2}},
               {31, {32, 2}}, {32, {32, 3}}, {63, {64, 4}}, {64, {64, 5}}};
    for (auto &e : tab)
        if (d <= e.maxd) {
            *KP = e.t.KP;
            *NCB = e.t.NCB;
            return true;
        }
    return false;
}
// k_phi<float, KP, NCB, ..., false>: every class of pick_tiles
inline constexpr TileClass TILES_F32[] = {{4, 1},  {8, 1},  {12, 1}, {16, 1}, {16, 2},
                                          {32, 2}, {32, 3}, {64, 4}, {64, 5}};
// k_phi<double, KP, NCB, ..., false>: d > 16 only (below, fp64 is the row stream)
inline constexpr TileClass TILES_F64[] = {{32, 2}, {32, 3}, {64, 4}, {64, 5}};
// S1V, d = 16 NCB > 16 (row sums on the VALU, no column of ones): k_phi<T, ..., true>
// of both types and k_phi_b3<..., true, RG>
inline constexpr TileClass TILES_S1V[] = {{32, 2}, {64, 3}, {64, 4}};
// k_phi_f32s<KP, NCB> (KP % 16 == 0; never S1V: that needs the bf16 kernel)
inline constexpr TileClass TILES_F32S[] = {{16, 1}, {16, 2}, {32, 2}, {32, 3}, {64, 4}, {64, 5}};
// k_phi_b3<KP, NCB, NW, false, RG>, and its row groups per wave RG
inline constexpr TileClass TILES_B3[] = {{32, 2}, {32, 3}, {64, 4}, {64, 5}};
inline constexpr int B3_RG[] = {1, 2};
// median tile passes: k_pair_tiles<T, KP, MODE>; k_pair_tcol<KP> / k_pair_tcol3<KP> (fp32)
inline constexpr int PAIR_KP_F64[] = {32, 64};
inline constexpr int PAIR_KP_F32[] = {4, 8, 12, 16, 32, 64};
// MODE: 0 collect, 1 radix histogram, 2 debug dump; tiles also 3, the sampled tiles
inline constexpr int PAIR_ROW_MODES[] = {0, 1, 2};  // k_pair_rows<D, MODE>, D in ROW_DIMS
inline constexpr int PAIR_TILE_MODES[] = {0, 1, 2, 3};

// Wave counts and the register prefetch of k_phi / k_phi_b3: the fp32 tile
// kernel's are fixed, the other three are what the kernel translation unit was
// built with (phi_build(), svgd_kernels.h; the defaults unless overridden for a
// measurement).
constexpr int TILE_F32_NW = 4;
constexpr bool TILE_F32_PRE = false;
struct PhiBuild {
    int tile_nw = 8;      // SVGD_PHI_NW
    bool tile_pre = true; // SVGD_PHI_PRE
    int b3_nw = 8;        // SVGD_B3_NW
};

template <class T, size_t N> constexpr bool built(const T (&list)[N], const T &v)
{
    for (const T &e : list)
        if (e == v) return true;
    return false;
}

// What is built for this dimension and dtype: the plan's input.
struct PhiCaps {
    int rows_kp;   // med_rec_stride(d) where the row stream has this d, else 0
    bool sym;      // k_phi_sym<d>
    bool tile_s1v; // an S1V class with 16 NCB = d
    bool f32s, b3; // k_phi_f32s / k_phi_b3 of pick_tiles' class
    // template arguments only the kernel name needs
    int tile_waves; // k_phi's waves per work-group of the dtype ...
    bool tile_pre;  // ... and its register prefetch
    int b3_waves;   // k_phi_b3's waves
};
constexpr PhiCaps phi_caps(int dim, bool f32, const PhiBuild &b = PhiBuild{})
{
    int KP = 0, NCB = 0;
    (void)pick_tiles(dim, &KP, &NCB);
    return PhiCaps{built(ROW_DIMS, dim) ? med_rec_stride(dim) : 0,
                   built(SYM_DIMS, dim),
                   dim % 16 == 0 && built(TILES_S1V, TileClass{KP, dim / 16}),
                   built(TILES_F32S, TileClass{KP, NCB}),
                   built(TILES_B3, TileClass{KP, NCB}),
                   f32 ? TILE_F32_NW : b.tile_nw,
                   f32 ? TILE_F32_PRE : b.tile_pre,
                   b.b3_nw};
}

} // namespace svgd_amd
