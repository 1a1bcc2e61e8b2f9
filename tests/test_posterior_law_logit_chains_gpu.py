"""GPU test: the logistic chain batch (bb_logit_chain.hip) against the exact posterior law.

S1 of tests/posterior_law.py for the logistic bridge at logit_problem(200, 5, seed=3), the
design of test_logistic_s1, but K = 256 chains of 4000 draws in ONE call: the integration-by-
parts identities with both power conditions, split R-hat and the resolution of the chain means.
The size is chosen so that the power condition is not marginal.  The oracle alone, at these
sizes under two seeds, gave for the family's max |z| against its bound 5.52:

    run                  as drawn   scaled (1 + 2^-8)   swapped
    256 x 4000, seed 1   1.29       8.66                > 1000
    256 x 4000, seed 2   2.08       11.05               > 1000
    256 x 2500           --         6.98                --

with R-hat 1.0006 and s.e. / sd 0.0019 in both 256 x 4000 runs; 6.98 at 256 x 2500 is too close
to the bound, hence 4000.  The batch kernel is pinned first (assert_batch_kernel): a refused
design would pass the law through the general path, one chain after another.
"""
import numpy as np
import pytest

from bayesbridge_amd.diagnostics import rhat
from tests import posterior_law as pl
from tests.test_logit_gpu import logit_problem
from tests.test_posterior_law_gpu import SEED, assert_batch_kernel

pytestmark = pytest.mark.gpu

K, M, BURN = 256, 4000, 100


def test_logistic_batch_s1(gpu_lib):
    bb = gpu_lib
    X, y, _ = logit_problem(200, 5, seed=3)
    assert_batch_kernel(bb, X, y, K, threads=512, method=6)
    bb.set_seed(SEED + 60)
    g = bb.bridge_reg_logit_chains(y, X, nsamp=M, nchains=K, burn=BURN)
    assert bb.get_rng_state() == (SEED + 60, K)
    beta = g["beta"]
    assert beta.shape == (K, M, 5) and np.all(np.isfinite(beta))
    r = float(np.max(rhat(beta)))
    means = beta.mean(axis=1)  # (K, p)
    sd = beta.reshape(-1, 5).std(axis=0, ddof=1)
    se = means.std(axis=0, ddof=1) / np.sqrt(K)
    print(f"logistic batch S1 200x5: split R-hat {r:.4f}, s.e. / sd of the chain means "
          f"{np.max(se / sd):.4f}")
    assert r <= pl.RHAT_MAX, r
    assert np.all(se <= pl.RESOLUTION * sd), (se, sd)
    z, bound = pl.stein_verdicts("logistic batch S1 200x5", beta,
                                 lambda b, c: pl.bs_logit(b, X, y, 0.5), pl.most_correlated(X))
    print(f"logistic batch S1 200x5: max |z| {z:.2f} (bound {bound:.2f})")
