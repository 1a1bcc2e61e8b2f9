"""chain_plan, the one place that decides which fused chain kernel runs a configuration, without a
GPU (bb_chain_kernel needs no device): over a grid of configurations its batch answer and refusal
text equal a table measured on the commit before the plan existed, bb_chains_create still reports
exactly those texts, and its engine answer follows the rules include/bayesbridge.h documents.

REFUSED was produced by running that earlier commit's bb_chains_create over GRID on a machine
without a GPU: a refusal is its message; a configuration that passes the rules fails later, for
want of a device, with a message that is none of the refusals ('.').  Each row is one (method, n,
p); its 128 characters are COMBOS in order."""
import ctypes
import itertools

import numpy as np
import pytest

import bayesbridge_amd as bb
from tests.test_abi import declared_functions

STABLE = [(40, 3), (40, 32), (40, 33), (200, 128), (200, 129), (12, 20)]
TRI = [(50, 6), (150, 32), (80, 33), (12, 20)]
LOGIT = [(40, 1), (40, 32), (40, 33), (8, 9), (4097, 4)]
ROWS = ([(m, n, p) for m in (0, 1, 2, 3) for n, p in STABLE] + [(4, n, p) for n, p in TRI] +
        [(6, n, p) for n, p in LOGIT])
# ortho, true_alpha, world, p_local == p // 2, key 25, key 26, key 27
COMBOS = list(itertools.product((0, 1), (0.5, 0.0), (1, 2), (False, True), (0, 1), (0, 1), (0, 1)))
KEYS = (25, 26, 27)

MESSAGES = {
    "a": "a chain batch holds every column (p_local == p)",
    "b": "a chain batch runs on one device (world == 1)",
    "c": "a chain batch needs alpha known (true_alpha > 0)",
    "d": "a chain batch needs p <= 32",
    "e": "a chain batch needs p <= 128 (wide fused chains on)",
    "f": "a chain batch needs p <= n (or the orthogonal design)",
    "g": "a chain batch runs the stable mixture's Cholesky or orthogonal draw (method 0 or 1), the "
         "triangle mixture (method 4) or the logistic bridge (method 6)",
    "h": "a triangle chain batch needs p <= 32",
    "i": "a triangle chain batch needs p <= n",
    "j": "a logistic chain batch needs p <= 32",
    "k": "a logistic chain batch needs p <= n",
    "l": "a logistic chain batch needs n <= 4096",
}

REFUSED = {
    (0, 40, 3): ("........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"
                 "........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"),
    (0, 40, 32): ("........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"
                  "........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"),
    (0, 40, 33): ("dddd....aaaaaaaabbbbbbbbbbbbbbbbddddccccaaaaaaaabbbbbbbbbbbbbbbb"
                  "dddd....aaaaaaaabbbbbbbbbbbbbbbbddddccccaaaaaaaabbbbbbbbbbbbbbbb"),
    (0, 200, 128): ("dddd....aaaaaaaabbbbbbbbbbbbbbbbddddccccaaaaaaaabbbbbbbbbbbbbbbb"
                    "dddd....aaaaaaaabbbbbbbbbbbbbbbbddddccccaaaaaaaabbbbbbbbbbbbbbbb"),
    (0, 200, 129): ("ddddeeeeaaaaaaaabbbbbbbbbbbbbbbbddddeeeeaaaaaaaabbbbbbbbbbbbbbbb"
                    "ddddeeeeaaaaaaaabbbbbbbbbbbbbbbbddddeeeeaaaaaaaabbbbbbbbbbbbbbbb"),
    (0, 12, 20): ("ffffffffaaaaaaaabbbbbbbbbbbbbbbbffffffffaaaaaaaabbbbbbbbbbbbbbbb"
                  "........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"),
    (1, 40, 3): ("........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"
                 "........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"),
    (1, 40, 32): ("........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"
                  "........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"),
    (1, 40, 33): ("dddd....aaaaaaaabbbbbbbbbbbbbbbbddddccccaaaaaaaabbbbbbbbbbbbbbbb"
                  "dddd....aaaaaaaabbbbbbbbbbbbbbbbddddccccaaaaaaaabbbbbbbbbbbbbbbb"),
    (1, 200, 128): ("dddd....aaaaaaaabbbbbbbbbbbbbbbbddddccccaaaaaaaabbbbbbbbbbbbbbbb"
                    "dddd....aaaaaaaabbbbbbbbbbbbbbbbddddccccaaaaaaaabbbbbbbbbbbbbbbb"),
    (1, 200, 129): ("ddddeeeeaaaaaaaabbbbbbbbbbbbbbbbddddeeeeaaaaaaaabbbbbbbbbbbbbbbb"
                    "ddddeeeeaaaaaaaabbbbbbbbbbbbbbbbddddeeeeaaaaaaaabbbbbbbbbbbbbbbb"),
    (1, 12, 20): ("ffffffffaaaaaaaabbbbbbbbbbbbbbbbffffffffaaaaaaaabbbbbbbbbbbbbbbb"
                  "........aaaaaaaabbbbbbbbbbbbbbbbcc..cc..aaaaaaaabbbbbbbbbbbbbbbb"),
    (2, 40, 3): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                 "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (2, 40, 32): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                  "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (2, 40, 33): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                  "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (2, 200, 128): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                    "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (2, 200, 129): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                    "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (2, 12, 20): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                  "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (3, 40, 3): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                 "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (3, 40, 32): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                  "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (3, 40, 33): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                  "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (3, 200, 128): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                    "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (3, 200, 129): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                    "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (3, 12, 20): ("ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"
                  "ggggggggaaaaaaaabbbbbbbbbbbbbbbbggggggggaaaaaaaabbbbbbbbbbbbbbbb"),
    (4, 50, 6): ("........aaaaaaaabbbbbbbbbbbbbbbbc.c.c.c.aaaaaaaabbbbbbbbbbbbbbbb"
                 "........aaaaaaaabbbbbbbbbbbbbbbbc.c.c.c.aaaaaaaabbbbbbbbbbbbbbbb"),
    (4, 150, 32): ("........aaaaaaaabbbbbbbbbbbbbbbbc.c.c.c.aaaaaaaabbbbbbbbbbbbbbbb"
                   "........aaaaaaaabbbbbbbbbbbbbbbbc.c.c.c.aaaaaaaabbbbbbbbbbbbbbbb"),
    (4, 80, 33): ("hhhhhhhhaaaaaaaabbbbbbbbbbbbbbbbhhhhhhhhaaaaaaaabbbbbbbbbbbbbbbb"
                  "hhhhhhhhaaaaaaaabbbbbbbbbbbbbbbbhhhhhhhhaaaaaaaabbbbbbbbbbbbbbbb"),
    (4, 12, 20): ("iiiiiiiiaaaaaaaabbbbbbbbbbbbbbbbiiiiiiiiaaaaaaaabbbbbbbbbbbbbbbb"
                  "iiiiiiiiaaaaaaaabbbbbbbbbbbbbbbbiiiiiiiiaaaaaaaabbbbbbbbbbbbbbbb"),
    (6, 40, 1): ("................bbbbbbbbbbbbbbbb................bbbbbbbbbbbbbbbb"
                 "................bbbbbbbbbbbbbbbb................bbbbbbbbbbbbbbbb"),
    (6, 40, 32): ("........aaaaaaaabbbbbbbbbbbbbbbb........aaaaaaaabbbbbbbbbbbbbbbb"
                  "........aaaaaaaabbbbbbbbbbbbbbbb........aaaaaaaabbbbbbbbbbbbbbbb"),
    (6, 40, 33): ("jjjjjjjjaaaaaaaabbbbbbbbbbbbbbbbjjjjjjjjaaaaaaaabbbbbbbbbbbbbbbb"
                  "jjjjjjjjaaaaaaaabbbbbbbbbbbbbbbbjjjjjjjjaaaaaaaabbbbbbbbbbbbbbbb"),
    (6, 8, 9): ("kkkkkkkkaaaaaaaabbbbbbbbbbbbbbbbkkkkkkkkaaaaaaaabbbbbbbbbbbbbbbb"
                "kkkkkkkkaaaaaaaabbbbbbbbbbbbbbbbkkkkkkkkaaaaaaaabbbbbbbbbbbbbbbb"),
    (6, 4097, 4): ("llllllllaaaaaaaabbbbbbbbbbbbbbbbllllllllaaaaaaaabbbbbbbbbbbbbbbb"
                   "llllllllaaaaaaaabbbbbbbbbbbbbbbbllllllllaaaaaaaabbbbbbbbbbbbbbbb"),
}


def config(m, n, p, combo):
    ortho, alpha, world, half = combo[:4]
    return bb.EngineConfig(n=n, p=p, method=m, ortho=bool(ortho), true_alpha=alpha, world=world,
                           p_local=p // 2 if half else p)


def batch_kind(m, p):
    """The family of a batch that is not refused."""
    return 3 if m == 4 else 4 if m == 6 else 1 if p <= 32 else 2


def engine_kind(m, n, p, combo):
    """bb_chain_kernel(cfg, 0) by the rules of include/bayesbridge.h (bb_chains_create, keys 25,
    26 and 27, bb_chain_kernel): an engine does not look at p_local, takes the orthogonal draw
    under methods 2 and 3 too, and has no logistic kernel."""
    ortho, alpha, world, _, k25, k26, k27 = combo
    if world != 1 or m == 6:
        return 0
    if m == 4:
        return 3 if p <= 32 and p <= n and (alpha > 0 or k27) else 0
    if not (ortho or (m in (0, 1) and p <= n)):
        return 0
    if p <= 32:
        return 1 if alpha > 0 or k26 else 0
    return 2 if k25 and p <= 128 and alpha > 0 else 0


@pytest.fixture(scope="module")
def keys_restored():
    old = [bb.set_tuning(k, -1) for k in KEYS]
    yield
    for k, v in zip(KEYS, old):
        bb.set_tuning(k, v)


def grid():
    for row in ROWS:
        assert len(REFUSED[row]) == len(COMBOS)
        for combo, mark in zip(COMBOS, REFUSED[row]):
            for k, v in zip(KEYS, combo[4:]):
                bb.set_tuning(k, v)
            yield row, combo, mark


def test_export_is_declared():
    assert hasattr(bb.library(), "bb_chain_kernel")
    assert "bb_chain_kernel" in declared_functions()
    assert "bb_chain_kernel" in bb.EXPORTED_SYMBOLS


def test_plan_matches_the_measured_batch_rules_and_the_documented_engine_rules(keys_restored):
    L = bb.library()
    seen = set()
    for (m, n, p), combo, mark in grid():
        cfg = config(m, n, p, combo)
        kind = bb.chain_kernel(cfg, batch=True)
        text = L.bb_last_error().decode()
        if mark == ".":
            assert (kind, text) == (batch_kind(m, p), ""), (m, n, p, combo, kind, text)
        else:
            assert (kind, text) == (0, MESSAGES[mark]), (m, n, p, combo, kind, text)
        assert bb.chain_kernel(cfg) == engine_kind(m, n, p, combo), (m, n, p, combo)
        assert L.bb_last_error().decode() == ""
        seen.add(mark)
    assert seen == set(MESSAGES) | {"."}  # the grid reaches every refusal and every family


def test_chains_create_reports_the_same_texts(keys_restored):
    """Every refused configuration; every accepted one without a device (it fails later, with
    none of the refusals), and with one the first of each row (it is created)."""
    L = bb.library()
    have_gpu = bb.device_count() >= 1
    created = set()
    for row, combo, mark in grid():
        if mark == "." and have_gpu and row in created:
            continue
        m, n, p = row
        rng = np.random.default_rng(1)
        X = np.asfortranarray(rng.standard_normal((n, p)))
        y = (rng.random(n) < 0.5).astype(np.float64)
        c = config(m, n, p, combo).to_c()
        h = ctypes.c_void_p()
        rc = L.bb_chains_create(ctypes.byref(c), 2, bb._p(X), bb._p(y), ctypes.byref(h))
        if rc == 0:
            L.bb_chains_destroy(h)
            assert mark == "." and have_gpu, (row, combo)
            created.add(row)
            continue
        text = L.bb_last_error().decode()
        if mark == ".":
            assert not have_gpu, (row, combo, text)
            assert not any(r in text for r in MESSAGES.values()), (row, combo, text)
        else:
            assert text == "bb_chains_create: " + MESSAGES[mark], (row, combo, text)
