"""The switch of the wide fused chains (bb_set_tuning key 25, bb.set_wide_chains), without a
GPU: it exists, is off by default, returns the value it replaces and clamps to 1.

The key is 25 because tests/test_abi.py::test_tuning_table_without_gpu pins 22 and 23 as unknown
keys (they answer -1), as it was 24 for the fp32 beta pass."""
import bayesbridge_amd as bb

WIDE_KEY = 25


def test_wide_key_is_off_by_default():
    """-1 (unknown key) without the feature."""
    assert bb.set_tuning(WIDE_KEY, -1) == 0


def test_wide_key_returns_previous_and_clamps():
    old = bb.set_tuning(WIDE_KEY, -1)
    try:
        assert bb.set_tuning(WIDE_KEY, 1000) == old
        assert bb.set_tuning(WIDE_KEY, -1) == 1
        assert bb.set_tuning(WIDE_KEY, 0) == 1
        assert bb.set_tuning(WIDE_KEY, -1) == 0
        assert bb.set_wide_chains(True) is False
        assert bb.set_tuning(WIDE_KEY, -1) == 1
        assert bb.set_wide_chains(False) is True
        assert bb.set_tuning(WIDE_KEY, -1) == 0
    finally:
        bb.set_tuning(WIDE_KEY, old)


def test_keys_pinned_as_unknown_stay_unknown():
    for key in (22, 23):
        assert bb.set_tuning(key, -1) == -1
