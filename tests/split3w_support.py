"""Handles for the tests of the 384-channel tile of fp32 layer 5 (csrc/tdnn_split3w.hip).  Its two dispatch knobs are read in the
kernel's own translation unit (tdnn_split3w_knobs), not in read_policy, so tdnn_support.KNOBS does not list them and
tdnn_support.make_model neither accepts nor clears them; make_model here does both around it.  tests/test_split3w_knobs.py ties
WIDE_KNOBS to the source.  A plain module like tdnn_support.py; the test files import it."""
import os

import tdnn_support

WIDE_KNOBS = ("XVEC_SPLIT3_WIDE", "XVEC_SPLIT3_WIDE_MIN_ROWS")


def make_model(sd, env=None, **kw):
    """tdnn_support.make_model under the knobs `env` and no others, the wide tile's two included: whatever the calling
    environment sets for them does not reach the handle, and the environment is as it was afterwards."""
    env = env or {}
    old = {k: os.environ.pop(k, None) for k in WIDE_KNOBS}
    try:
        os.environ.update({k: v for k, v in env.items() if k in WIDE_KNOBS})
        return tdnn_support.make_model(sd, {k: v for k, v in env.items() if k not in WIDE_KNOBS}, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
