"""The switch of alpha sampling inside the fused small chains (bb_set_tuning key 26,
bb.set_fused_alpha), without a GPU: it exists, is off by default, returns the value it replaces
and clamps to 1.

The key is 26 because tests/test_abi.py::test_tuning_table_without_gpu pins 22 and 23 as unknown
keys (they answer -1), and 24 and 25 are the fp32 beta pass and the wide fused chains."""
import bayesbridge_amd as bb

ALPHA_KEY = 26


def test_alpha_key_is_off_by_default():
    assert bb.set_tuning(ALPHA_KEY, -1) == 0


def test_alpha_key_returns_previous_and_clamps():
    old = bb.set_tuning(ALPHA_KEY, -1)
    try:
        assert bb.set_tuning(ALPHA_KEY, 1000) == old
        assert bb.set_tuning(ALPHA_KEY, -1) == 1
        assert bb.set_tuning(ALPHA_KEY, 0) == 1
        assert bb.set_tuning(ALPHA_KEY, -1) == 0
    finally:
        bb.set_tuning(ALPHA_KEY, old)


def test_set_fused_alpha_mirrors_the_key():
    old = bb.set_tuning(ALPHA_KEY, 0)
    try:
        assert bb.set_fused_alpha(True) is False
        assert bb.set_tuning(ALPHA_KEY, -1) == 1
        assert bb.set_fused_alpha(False) is True
        assert bb.set_tuning(ALPHA_KEY, -1) == 0
    finally:
        bb.set_tuning(ALPHA_KEY, old)


def test_neighbouring_keys_are_untouched():
    for key in (22, 23):
        assert bb.set_tuning(key, -1) == -1
    assert bb.set_tuning(25, -1) == 0 and bb.set_tuning(21, -1) == 0
