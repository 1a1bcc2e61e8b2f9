"""The switch of alpha sampling inside the fused triangle-mixture chains (bb_set_tuning key 27,
bb.set_fused_tri_alpha), without a GPU: it exists, is off by default, returns the value it
replaces and clamps to 1.

The key is not 26: tests/test_alpha_chains_gpu.py::test_switch pins that a method-4 batch with
alpha unknown is refused with keys 25 and 26 both on."""
import bayesbridge_amd as bb

TRI_ALPHA_KEY = 27


def test_tri_alpha_key_is_off_by_default():
    assert bb.set_tuning(TRI_ALPHA_KEY, -1) == 0


def test_tri_alpha_key_returns_previous_and_clamps():
    old = bb.set_tuning(TRI_ALPHA_KEY, -1)
    try:
        assert bb.set_tuning(TRI_ALPHA_KEY, 1000) == old
        assert bb.set_tuning(TRI_ALPHA_KEY, -1) == 1
        assert bb.set_tuning(TRI_ALPHA_KEY, 0) == 1
        assert bb.set_tuning(TRI_ALPHA_KEY, -1) == 0
    finally:
        bb.set_tuning(TRI_ALPHA_KEY, old)


def test_set_fused_tri_alpha_mirrors_the_key():
    old = bb.set_tuning(TRI_ALPHA_KEY, 0)
    try:
        assert bb.set_fused_tri_alpha(True) is False
        assert bb.set_tuning(TRI_ALPHA_KEY, -1) == 1
        assert bb.set_fused_tri_alpha(False) is True
        assert bb.set_tuning(TRI_ALPHA_KEY, -1) == 0
    finally:
        bb.set_tuning(TRI_ALPHA_KEY, old)


def test_keys_26_and_27_are_separate_switches():
    """Key 27 is its own variable: each of the two alpha keys holds its value while the other is
    set and cleared, and the next key is still unknown."""
    old27, old26 = bb.set_tuning(TRI_ALPHA_KEY, 1), bb.set_tuning(26, 0)
    try:
        assert bb.set_tuning(TRI_ALPHA_KEY, -1) == 1 and bb.set_tuning(26, -1) == 0
        assert bb.set_tuning(26, 1) == 0
        assert bb.set_tuning(TRI_ALPHA_KEY, 0) == 1
        assert bb.set_tuning(26, -1) == 1 and bb.set_tuning(TRI_ALPHA_KEY, -1) == 0
        assert bb.set_tuning(28, -1) == -1
    finally:
        bb.set_tuning(TRI_ALPHA_KEY, old27)
        bb.set_tuning(26, old26)
