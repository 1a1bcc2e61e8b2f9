"""GPU test: the triangle chain batch with alpha sampled in the kernel (bb_set_tuning key 27,
k_tri_chains_mh) against the exact posterior law Q1 of tests/posterior_law.py.

tests/test_posterior_law_gpu.py::test_tri_q1 holds the general triangle path to this law with 8
chains of 12 000 sweeps, one chain per call; under the key the batch kernel takes the design, so
it gets what every batch kernel gets: 256 chains x 2000 sweeps, judged at the default resolution
with the must-miss assertion on.  Q1's design has one column: the p = 1 case of the kernel.
The triangle driver passes (alpha_a, alpha_b) in both loops, so under alpha_a = 1, alpha_b = 3 the
chain must match Beta(1, 3) d^2 and miss Beta(3, 3) d^2.  The beta traces are read again for
cross-chain independence.  The key is restored in a finally (tests/tuning.py).
"""
import pytest

from tests import posterior_law as pl
from tests.test_posterior_law_gpu import (K_BATCH, M_BATCH, SEED, assert_batch_kernel,
                                          assert_converged, q1_judge)
from tests.tuning import tuning

pytestmark = pytest.mark.gpu

TRI_ALPHA_KEY = 27


@pytest.mark.parametrize("ortho", [False, True], ids=["general", "ortho"])
@pytest.mark.parametrize("alpha_b", [1.0, 3.0], ids=["uniform", "b3"])
def test_tri_alpha_batch_q1(gpu_lib, ortho, alpha_b):
    bb = gpu_lib
    x, y, sig2, tau = pl.q1_data()
    what = f"tri alpha batch Q1 {'ortho' if ortho else 'general'}"
    with tuning(bb, TRI_ALPHA_KEY, 1):
        # a key that did not engage fails here instead of passing through the fallback
        assert_batch_kernel(bb, x[:, None], y, K_BATCH, method=4, true_alpha=0.0, alpha_a=1.0,
                            alpha_b=alpha_b, true_sig2=sig2, true_tau=tau, ortho=ortho)
        bb.set_seed(SEED + 60)
        g = bb.bridge_reg_tri_chains(y, x[:, None], nsamp=M_BATCH, nchains=K_BATCH, alpha=0.0,
                                     alpha_a=1.0, alpha_b=alpha_b, sig2_true=sig2, tau_true=tau,
                                     ortho=ortho)
    assert g["beta"].shape == (K_BATCH, M_BATCH, 1)
    assert_converged(g["beta"], what)
    q1_judge(what, "tri", alpha_b, g["beta"][..., 0], g["alpha"])
    zs = pl.neighbour_z(g["beta"])
    print(f"{what}: z of the neighbour correlation at shifts -2..2: "
          + ", ".join(f"{s:+d}: {z:+.2f}" for s, z in zs.items()))
    for s, z in zs.items():
        assert abs(z) <= pl.Z_SCALAR, (what, s, z)
