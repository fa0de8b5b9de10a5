// plan.h -- the tuning knobs and the phi plan (internal; host only, no HIP).
//
// svgd_capi.cpp reads the environment once into Knobs (read_knobs) and takes
// what is built for the dimension from built.h (phi_caps); plan_phi
// (plan.cpp) turns those into the one PhiPlan a context allocates for,
// launches from and reports as its kernel name.
#pragma once
#include <stdint.h>

#include <string>

#include "built.h"

namespace svgd_amd {

// One environment variable: unset, or its parsed value.
template <class T> struct Knob {
    bool set = false;
    T v{};
    T or_(T dflt) const { return set ? v : dflt; }
};

// Every SVGD_* variable the library reads, parsed
// by read_knobs (svgd_capi.cpp) at the top of each svgd_create*.  A default
// that depends on N, d, P, the CPU quota or the host ISA is applied where
// the value is used, as knob.or_(default).
struct Knobs {
    bool phi_tile_generic = false; // set at all: on
    Knob<int> phi_b3, phi_s1v;     // on / off
    Knob<int> phi_b3_rg;           // 1 or 2
    Knob<int> phi_sym;             // 0 off, 1 on, 2 the sharded form on one rank
    Knob<int> phi_split;           // on / off
    Knob<int> phi_split_frac;      // percent, 10..90
    Knob<int> x_mirror;            // on / off
    Knob<int64_t> bucket_cap;
    Knob<int64_t> median_sample;   // >= 1
    Knob<double> median_sigma;     // >= 0
    Knob<int> mcol;                // SVGD_COLLECT_FP64 inverted
    Knob<int> mcol_bf16;           // on / off
    Knob<int> speculate, track_bracket; // on / off
    Knob<double> track_min_width, track_err_mult;
    Knob<int> host_threads;        // >= 1
    Knob<int> debug_coll, g_comm;  // on / off
    Knob<std::string> hostcomm;    // the shared-memory name
    Knob<int> thin_select;         // on / off: Stein thinning's two-launch pick
};

// Which kernel computes phi_hat for a context's rows.
enum PhiPath {
    PHI_SYM,      // k_phi_sym: each unordered pair once (fp64, d <= 8)
    PHI_ROWS,     // k_phi_rows: the row stream (fp64, d <= 16)
    PHI_TILE_F64, // k_phi<double>
    PHI_TILE_F32, // k_phi<float>: the generic fp32 tile kernel
    PHI_F32S,     // k_phi_f32s: fp32 MFMA over operand-ordered column copies
    PHI_B3,       // k_phi_b3: fp32 products as bf16 part products
};

struct PhiPlan {
    PhiPath path = PHI_ROWS;
    int dim = 0;
    int KP = 0;        // stride of the centred coordinates xc (tile class, or the row stream's median record)
    int NCB = 0;       // 16-column blocks of V (tile kernels)
    int VW = 0;        // 16 NCB
    bool s1v = false;  // d = 16 NCB: row sums on the VALU, no V column of ones
    int R = 0;         // row stream: phi_rows_per_lane(dim)
    RowsKind rows_kind = ROWS_8W; // row stream: the geometry launched (ROWS_4W under a matrix scale)
    int b3_rg = 1;     // k_phi_b3's row groups per wave
    bool rows() const { return path == PHI_SYM || path == PHI_ROWS; }
    // the kernel's epilogue applies the optimizer update (else k_opt_update)
    bool fused() const { return rows() || path == PHI_F32S || path == PHI_B3; }
};

// The phi plan of rows [row0, ...) of n particles shared by plan_world
// ranks; false if the device path has no kernel for dim.  Pure: no HIP call,
// no environment read, no context.
bool plan_phi(int dim, int64_t n, int dtype, int plan_world, int64_t row0, const Knobs &k,
              const PhiCaps &cap, PhiPlan *p);

// A full-matrix kernel scale is chosen after the plan was made and modifies
// the launch per call: no symmetric pass, the 4-wave row kernel (signature
// rows).  The tile paths launch the planned kernel on transformed operands.
inline PhiPlan matrix_scale_plan(PhiPlan p)
{
    if (p.path == PHI_SYM) p.path = PHI_ROWS;
    p.rows_kind = ROWS_4W;
    return p;
}

// The plan's kernel with its template arguments, as rocprofv3 prints it
// (svgd_phi_kernel_name): the only place that spells them.
void phi_plan_name(const PhiPlan &p, const PhiCaps &cap, char *buf, int len);

} // namespace svgd_amd
