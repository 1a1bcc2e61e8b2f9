"""The one context manager the GPU tests set bb_set_tuning keys with: the keys hold inside the
`with` and are back at their old values after it, whatever the body raises."""
import contextlib


@contextlib.contextmanager
def tuning(bb, key=None, value=None, **keys):
    """tuning(bb, 25, 1) sets one key; tuning(bb, k21=1, k26=1) sets each k<key>."""
    want = {int(k[1:]): v for k, v in keys.items()}
    if key is not None:
        want[int(key)] = value
    old = {k: bb.set_tuning(k, v) for k, v in want.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            bb.set_tuning(k, v)
