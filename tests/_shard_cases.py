"""The sharded step on the tile paths, one table: every phi kernel behind the
fp64 tile path (d > 16) and behind SVGD_F32 with a shard that does not start
at row 0, at the smallest shape that still has a ragged last work-group on
some rank (the fp64 tile work-group is 128 rows, k_phi_f32s's 64), several
64-column tiles and a padded last column tile (n % 64 != 0).  Checked against
the plan on the CPU (tests/test_shard_cases_cpu.py) and run on the GPU
(tests/test_gpu_shard_paths.py, rank body tests/_gpu_shard_rank_worker.py).

A case is (id, dtype, world, n, d, env, names):
  dtype   "f64" / "f32"
  env     the knobs the case sets (every other knob of _dispatch.KNOBS unset)
  names   names[r]: what phi_kernel_name() / plan_phi_name() must start with
          on rank r
  shards  what the case claims about svgd_plan_rows: "unaligned" (some rank
          starts at a row that is no multiple of 16), "aligned" (every rank
          does, and the last one owns a ragged tail), "empty" (the last rank
          owns no row)

svgd_plan_rows gives ceil(n / world) rows to every rank but the last ones:
  n = 333 over 2: [0, 167) [167, 333)          rank 1 starts at 167 = 16 10 + 7
  n = 500 over 3: [0, 167) [167, 334) [334, 500)   167 / 167 / 166 rows
  n = 351 over 2: [0, 176) [176, 351)          176 = 16 11; 175 rows, a ragged tail
  n = 2 over 3:   [0, 1) [1, 2) [2, 2)         rank 2 owns no row
An F32 rank whose first row is no multiple of 16 runs the generic k_phi<float>
with the tile class the streamed plan chose -- at d = 32, 48 and 64 its S1V
form, which nothing else reaches.
"""
import collections

from svgdcpp_amd import _capi as C

Case = collections.namedtuple("Case", "id dtype world n d env names shards")


def _c(id, dtype, world, n, d, env, names, shards):
    names = (names,) * world if isinstance(names, str) else tuple(names)
    assert len(names) == world, id
    return Case(id, dtype, world, n, d, dict(env), names, shards)


def _t64(kp, ncb, s1v):
    return "k_phi<double, %d, %d, 8, true, %s>" % (kp, ncb, "true" if s1v else "false")


def _t32(kp, ncb, s1v):
    return "k_phi<float, %d, %d, 4, false, %s>" % (kp, ncb, "true" if s1v else "false")


CASES = [
    # fp64 tiles + k_opt_update, the same kernel on every rank
    _c("t64-d24", "f64", 2, 333, 24, {}, _t64(32, 2, False), "unaligned"),
    _c("t64-d32", "f64", 2, 333, 32, {}, _t64(32, 2, True), "unaligned"),
    _c("t64-d33-w3", "f64", 3, 500, 33, {}, _t64(64, 4, False), "unaligned"),
    _c("t64-d48", "f64", 2, 333, 48, {}, _t64(64, 3, True), "unaligned"),
    _c("t64-d64", "f64", 2, 333, 64, {}, _t64(64, 4, True), "unaligned"),
    # F32, rank 1 starts at row 167: rank 0 streamed, rank 1 generic
    _c("f32u-d6", "f32", 2, 333, 6, {}, "k_phi<float, 8, 1,", "unaligned"),
    _c("f32u-d14", "f32", 2, 333, 14, {}, ("k_phi_f32s<16, 1>", _t32(16, 1, False)), "unaligned"),
    _c("f32u-d16", "f32", 2, 333, 16, {}, ("k_phi_f32s<16, 2>", _t32(16, 2, False)), "unaligned"),
    _c("f32u-d20", "f32", 2, 333, 20, {}, ("k_phi_b3<32, 2, 8, false, 1>", _t32(32, 2, False)), "unaligned"),
    _c("f32u-d32", "f32", 2, 333, 32, {}, ("k_phi_b3<32, 2, 8, true, 1>", _t32(32, 2, True)), "unaligned"),
    _c("f32u-d48", "f32", 2, 333, 48, {}, ("k_phi_b3<64, 3, 8, true, 1>", _t32(64, 3, True)), "unaligned"),
    _c("f32u-d64", "f32", 2, 333, 64, {}, ("k_phi_b3<64, 4, 8, true, 1>", _t32(64, 4, True)), "unaligned"),
    _c("f32u-d50-w3", "f32", 3, 500, 50, {},
       ("k_phi_b3<64, 4, 8, false, 1>", _t32(64, 4, False), _t32(64, 4, False)), "unaligned"),
    # F32, rank 1 starts at row 176: every rank streamed
    _c("f32a-d14", "f32", 2, 351, 14, {}, "k_phi_f32s<16, 1>", "aligned"),
    _c("f32a-d24", "f32", 2, 351, 24, {}, "k_phi_b3<32, 2, 8, false, 1>", "aligned"),
    _c("f32a-d64", "f32", 2, 351, 64, {}, "k_phi_b3<64, 4, 8, true, 1>", "aligned"),
    _c("f32a-d64-rg2", "f32", 2, 351, 64, {"SVGD_PHI_B3_RG": "2"}, "k_phi_b3<64, 4, 8, true, 2>", "aligned"),
    _c("f32a-d24-f32s", "f32", 2, 351, 24, {"SVGD_PHI_B3": "0"}, "k_phi_f32s<32, 2>", "aligned"),
    # the last rank owns no row
    _c("empty-t64-d24", "f64", 3, 2, 24, {}, _t64(32, 2, False), "empty"),
    _c("empty-f32-d20", "f32", 3, 2, 20, {},
       ("k_phi_b3<32, 2, 8, false, 1>", _t32(32, 2, False), _t32(32, 2, False)), "empty"),
]
BY_ID = {c.id: c for c in CASES}

# c. a fixed SPD matrix scale, sharded
MATRIX_CASES = ["t64-d24", "f32u-d20", "f32a-d24"]
# d. median steps, sharded (each with the direct pass and with the bracket passes)
STEP_CASES = ["t64-d24", "t64-d64", "f32u-d20", "f32a-d64"]
# e. sharded equals one rank bit for bit: the fp64 tiles, and the F32 shards on
# which every rank runs the kernel the one-rank run does
BITWISE_CASES = ["t64-d24", "t64-d33-w3", "t64-d64"] + [c.id for c in CASES if c.shards == "aligned"]

OPTS = ("adam", "adagrad", "rmsprop")


def opt_of(case):
    """The optimizer of a case: Adam / AdaGrad / RMSProp rotated over the table."""
    return OPTS[CASES.index(case) % 3]


def dtype_of(case):
    return C.SVGD_F64 if case.dtype == "f64" else C.SVGD_F32
