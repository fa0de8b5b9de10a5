"""A context's life: everything it allocated goes back to the device when it
is closed, a context whose creation failed can be destroyed, and a later
context computes what the first one did.

Free device memory is hipMemGetInfo of the HIP runtime the library loaded.
The memory test detects an owner that does not free; it cannot see a leak of
a few hundred bytes (each buffer's release is by construction: every
allocation of the runtime is an owning member of the context)."""
import ctypes
import re

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

pytestmark = pytest.mark.gpu

MIB = 1 << 20
# the condition on six create / exercise / close cycles: a context that
# freed nothing would cost five times its symmetric pass's colpart alone,
# 22 * 12 * 1536 * 9 * 8 B = 29 MB -- not a measurement
DRIFT_CAP = 16 * MIB


def _hip():
    C.lib()
    for line in open("/proc/self/maps"):
        m = re.search(r"(/\S*libamdhip64\.so\S*)", line)
        if m:
            return ctypes.CDLL(m.group(1))
    raise RuntimeError("the library loaded no HIP runtime")


def _free_bytes(hip):
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _cycle(oracle):
    d, n, k = 8, 32768, 3
    X = oracle.splitmix((n, d), 2.0, 0xC1C1)
    mus = oracle.splitmix((k, d), 2.0, 0xC1C2)
    covs = [np.eye(d) * (1.0 + 0.5 * q) for q in range(k)]
    c = S.Context(d, n)
    assert c.phi_kernel_name().startswith("k_phi_sym")
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.set_device_model(S.GaussianSum(list(mus), covs))
    for _ in range(3):
        c.step_device()
    # a device GLM in the Gaussian sum's place: its buffers are re-allocated
    A = oracle.splitmix((16, d), 1.0, 0xC1C3)
    y = (oracle.splitmix((16,), 1.0, 0xC1C4) > 0).astype(np.float64)
    c.set_device_model(S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0))
    c.step_device()
    c.set_scale(C.SVGD_SCALE_HESSIAN)
    c.set_device_hessian(True)
    c.step_device()
    c.check(c.lib.svgd_set_timing(c.h, 2))  # phase and diagnostic events: the pool
    for _ in range(2):
        c.step_device()
    v, u = c.ksd(a=0.3)
    assert np.isfinite(v) and np.isfinite(u)
    # the sampled bracket with a larger sample and larger candidate regions
    # than the steps used: both buffers grow
    c.set_median_tuning(direct_max_pairs=0, sample_size=1 << 22, candidate_capacity=1 << 26)
    a, med = c.median_scale()
    assert a > 0 and med > 0
    c.close()


def test_cycles_return_device_memory(oracle):
    """Two warm-up cycles, then five measured ones.  Two, because the HIP
    runtime takes 64 MiB of its own during the second cycle of a process and
    keeps it (measured on an MI355X, equally with the library of the commit
    before the context owned its resources: free memory after cycles
    1, 2, ..., 6 was f, f - 64 MiB, f - 64 MiB, ..., f - 64 MiB); with one
    warm-up cycle that step would be counted as drift."""
    hip = _hip()
    _cycle(oracle)
    f0 = _free_bytes(hip)
    _cycle(oracle)
    f1 = _free_bytes(hip)
    print("lifecycle warm-up: first cycle to second %d bytes" % (f0 - f1))
    for i in range(5):
        _cycle(oracle)
        print("lifecycle cycle %d: free %d (warm - this = %d)" % (i + 3, _free_bytes(hip), f1 - _free_bytes(hip)))
    f6 = _free_bytes(hip)
    print("lifecycle drift: %d bytes over 5 cycles (cap %d)" % (f1 - f6, DRIFT_CAP))
    assert f1 - f6 <= DRIFT_CAP


def _step_matches_oracle(oracle):
    n, d = 77, 3
    X = oracle.splitmix((n, d), 2.0, 0xF00D)
    G = oracle.splitmix((n, d), 1.0, 0xF00E)
    a = 0.4
    c = S.Context(d, n)
    c.set_particles(X)
    ref = oracle.phi(X, G, a)
    assert np.max(np.abs(c.phi(G, a) - ref)) <= 1e-10
    c.set_scale(C.SVGD_SCALE_FIXED, a)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.1, 0.9, 0.999, 1e-8)
    c.check(c.lib.svgd_step(c.h, C.dptr(G)))
    Xr = X.copy()
    oracle.apply_update(Xr, oracle.Adam((n, d), 0.1, 0.9, 0.999).step(ref), None, None)
    assert np.max(np.abs(c.get_particles() - Xr)) <= 1e-10
    c.close()


def test_failed_create_is_destroyable(oracle):
    """Creation that stops early hands back a half-built context; destroying
    it is safe, and the next context works."""
    with pytest.raises(S.DimensionMismatchException, match=r"\[Dimension Error\]"):
        S.Context(65, 100)
    _step_matches_oracle(oracle)
    with pytest.raises(ValueError, match=r"\[Argument Error\] Invalid world/rank"):
        S.Context(3, 77, world=2, rank=0)
    _step_matches_oracle(oracle)


@pytest.mark.parametrize("d,kernel", [(3, "k_phi_rows"), (33, "k_phi<")])
def test_same_trajectory_in_every_cycle(oracle, d, kernel):
    """Five Adam steps from the same seed: the sixth context created and
    closed in this process gives the first one's particles, bit for bit."""
    n, k = 300, 2
    X = oracle.splitmix((n, d), 2.0, 0xABC0 + d)
    mus = oracle.splitmix((k, d), 2.0, 0xABD0 + d)
    covs = [np.eye(d) * (1.0 + 0.5 * q) for q in range(k)]

    def run():
        c = S.Context(d, n)
        assert c.phi_kernel_name().startswith(kernel)
        c.set_particles(X)
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.1, 0.9, 0.999, 1e-8)
        model = S.GaussianSum(list(mus), covs)
        for _ in range(5):
            c.step_with_model(model)
        out = c.get_particles()
        c.close()
        return out

    first = run()
    for _ in range(4):
        run()
    assert np.array_equal(run(), first)
