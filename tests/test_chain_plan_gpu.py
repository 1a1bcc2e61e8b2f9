"""GPU tests that the engine and the chain batch follow chain_plan (bb_chain_kernel): an engine
runs five sweeps in one launch exactly where the plan names a kernel family for it, a ChainBatch
is created exactly where the plan names one for the batch, and the batch reports the threads of
the instance that family runs.  The shapes are the smallest on each side of every rule's edge:
p = 32 | 33 and 128 | 129 for the stable mixture, 32 | 33 for the triangle mixture, p > n with and
without the orthogonal draw, alpha unknown with and without keys 26 and 27."""
import numpy as np
import pytest

from tests.conftest import synthetic_problem
from tests.test_tri_alpha_chains_gpu import launch_brackets
from tests.tuning import tuning

pytestmark = pytest.mark.gpu

SWEEPS = 5
# (method, n, p, config fields, tuning keys)
CASES = [
    (0, 20, 3, {}, {}),
    (0, 40, 32, {}, {}),
    (0, 40, 33, {}, dict(k25=0)),
    (0, 40, 33, {}, dict(k25=1)),
    (0, 200, 128, {}, dict(k25=1)),
    (0, 200, 129, {}, dict(k25=1)),
    (0, 12, 20, dict(ortho=True), {}),
    (0, 12, 20, {}, {}),
    (0, 40, 12, dict(true_alpha=0.0), dict(k26=0)),
    (0, 40, 12, dict(true_alpha=0.0), dict(k26=1)),
    (0, 80, 40, dict(true_alpha=0.0), dict(k25=1, k26=1)),
    (4, 50, 6, {}, {}),
    (4, 150, 32, {}, {}),
    (4, 80, 33, {}, {}),
    (4, 100, 20, dict(ortho=True), {}),
    (4, 50, 6, dict(true_alpha=0.0), dict(k27=0)),
    (4, 50, 6, dict(true_alpha=0.0), dict(k27=1)),
    (6, 40, 5, {}, {}),
]
# what the rules of include/bayesbridge.h give for each case: (engine, batch)
KINDS = [(1, 1), (1, 1), (0, 0), (2, 2), (2, 2), (0, 0), (1, 1), (0, 0), (0, 0), (1, 1), (0, 0),
         (3, 3), (3, 3), (0, 0), (3, 3), (0, 0), (3, 3), (0, 4)]


def problem(method, n, p, ortho):
    if method == 6:
        rng = np.random.default_rng(3)
        X = np.asfortranarray(rng.standard_normal((n, p)))
        return X, (rng.random(n) < 0.5).astype(np.float64)
    if ortho and p <= n:  # orthogonal columns, as the flag promises
        rng = np.random.default_rng(9)
        Q, _ = np.linalg.qr(rng.standard_normal((n, p)))
        X = np.asfortranarray(Q * 4.0)
        return X, X @ np.r_[np.ones(3), np.zeros(p - 3)] + rng.standard_normal(n)
    X, y, _ = synthetic_problem(n, p, seed=11)
    return X, y


@pytest.mark.parametrize("case", range(len(CASES)))
def test_engine_and_batch_follow_the_plan(gpu_lib, case):
    bb = gpu_lib
    method, n, p, fields, keys = CASES[case]
    want_engine, want_batch = KINDS[case]
    X, y = problem(method, n, p, fields.get("ortho", False))
    cfg = bb.EngineConfig(n=n, p=p, method=method, **fields)
    with tuning(bb, **keys):
        assert bb.chain_kernel(cfg) == want_engine
        assert bb.chain_kernel(cfg, batch=True) == want_batch
        refusal = bb.library().bb_last_error().decode()
        e = bb.Engine(cfg, X, y)
        K = 2 if method == 6 else 3
        try:
            b = bb.ChainBatch(cfg, K, X, y)
        except RuntimeError as ex:
            assert want_batch == 0 and refusal and refusal in str(ex), (refusal, str(ex))
            b = None
    # the engine and the batch keep the path they were created with (the keys are back)
    assert launch_brackets(bb, e, SWEEPS) == (1 if want_engine else SWEEPS)
    assert (b is not None) == (want_batch != 0)
    if b is not None:
        wide = 256 if p <= 64 else 512  # wide_chains_threads (bb_kernels.h)
        assert b.nchains == K and b.threads() == (wide if want_batch == 2 else 512)
        assert b.resident_per_cu() >= 1


def test_packed_instance_reports_256_threads(gpu_lib):
    """Key 21 with K >= 2 x CUs: the small family's 256-thread instance, and only that family's
    (a logistic batch has one instance of 512 threads)."""
    bb = gpu_lib
    K = 2 * bb.compute_units()
    X, y = problem(0, 20, 3, False)
    Xl, yl = problem(6, 40, 5, False)
    with tuning(bb, 21, 1):
        small = bb.ChainBatch(bb.EngineConfig(n=20, p=3), K, X, y)
        few = bb.ChainBatch(bb.EngineConfig(n=20, p=3), K - 1, X, y)
        logit = bb.ChainBatch(bb.EngineConfig(n=40, p=5, method=6), K, Xl, yl)
    assert small.threads() == 256 and small.resident_per_cu() >= 2
    assert few.threads() == 512
    assert logit.threads() == 512
