"""The phi dispatch rule, stated independently of the library: which kernel
each (dtype, d) launches by default and under the A/B knobs.  One table,
checked against the plan on the CPU (tests/test_phi_plan_cpu.py) and against
the contexts on the GPU (tests/test_gpu_dim_sweep.py)."""

# Every knob the dispatch tests start from the default of.
KNOBS = ("SVGD_PHI_SYM", "SVGD_PHI_B3", "SVGD_PHI_B3_RG", "SVGD_PHI_S1V", "SVGD_PHI_TILE_GENERIC",
         "SVGD_COLLECT_FP64", "SVGD_MCOL_BF16", "SVGD_BUCKET_CAP", "SVGD_MEDIAN_SAMPLE",
         "SVGD_MEDIAN_SIGMA")

# (d_lo, d_hi, name); {d} is the dimension.  k_phi<T, KP, NCB, waves, prefetch,
# S1V>: the fp64 build has 8 waves and the register prefetch, the fp32 one 4
# waves and none (PhiCfg in svgd_kernels.hip).
F64_TABLE = [
    (1, 8, "k_phi_rows<{d}, 4, 8, 8192, 8>"),
    (9, 16, "k_phi_rows<{d}, 2, 8, 8192, 8>"),
    (17, 31, "k_phi<double, 32, 2, 8, true, false>"),
    (32, 32, "k_phi<double, 32, 2, 8, true, true>"),
    (33, 47, "k_phi<double, 64, 4, 8, true, false>"),
    (48, 48, "k_phi<double, 64, 3, 8, true, true>"),
    (49, 63, "k_phi<double, 64, 4, 8, true, false>"),
    (64, 64, "k_phi<double, 64, 4, 8, true, true>"),
]
F32_TABLE = [
    (1, 4, "k_phi<float, 4, 1, 4, false, false>"),
    (5, 8, "k_phi<float, 8, 1, 4, false, false>"),
    (9, 12, "k_phi<float, 12, 1, 4, false, false>"),
    (13, 15, "k_phi_f32s<16, 1>"),
    (16, 16, "k_phi_f32s<16, 2>"),
    (17, 31, "k_phi_b3<32, 2, 8, false, 1>"),
    (32, 32, "k_phi_b3<32, 2, 8, true, 1>"),
    (33, 47, "k_phi_b3<64, 4, 8, false, 1>"),
    (48, 48, "k_phi_b3<64, 3, 8, true, 1>"),
    (49, 63, "k_phi_b3<64, 4, 8, false, 1>"),
    (64, 64, "k_phi_b3<64, 4, 8, true, 1>"),
]


def expected_name(table, d):
    hits = [name.format(d=d) for lo, hi, name in table if lo <= d <= hi]
    assert len(hits) == 1, (d, hits)  # the table covers 1..64 once
    return hits[0]


# F32 phi cases (d, knob, name): every d at the defaults (name None: the
# table's), then the knob rows -- SVGD_PHI_B3=0, SVGD_PHI_S1V=0,
# SVGD_PHI_TILE_GENERIC=1.
F32_VARIANTS = ([(d, None, None) for d in range(1, 65)] +
                [(17, "SVGD_PHI_B3", "k_phi_f32s<32, 2>"), (31, "SVGD_PHI_B3", "k_phi_f32s<32, 2>"),
                 (32, "SVGD_PHI_B3", "k_phi_f32s<32, 3>"), (48, "SVGD_PHI_B3", "k_phi_f32s<64, 4>"),
                 (63, "SVGD_PHI_B3", "k_phi_f32s<64, 4>"), (64, "SVGD_PHI_B3", "k_phi_f32s<64, 5>"),
                 (32, "SVGD_PHI_S1V", "k_phi_b3<32, 3, 8, false, 1>"),
                 (48, "SVGD_PHI_S1V", "k_phi_b3<64, 4, 8, false, 1>"),
                 (64, "SVGD_PHI_S1V", "k_phi_b3<64, 5, 8, false, 1>"),
                 (12, "SVGD_PHI_TILE_GENERIC", "k_phi<float, 12, 1, 4, false, false>"),
                 (16, "SVGD_PHI_TILE_GENERIC", "k_phi<float, 16, 2, 4, false, false>"),
                 (32, "SVGD_PHI_TILE_GENERIC", "k_phi<float, 32, 3, 4, false, false>")])


def knob_value(knob):
    """The value the knob rows of F32_VARIANTS set."""
    return "1" if knob == "SVGD_PHI_TILE_GENERIC" else "0"
