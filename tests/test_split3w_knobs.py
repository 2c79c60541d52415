"""The dispatch knobs a handle reads from the environment are listed, all of them: tdnn_support.KNOBS holds the ones read_policy
reads with env_int (tests/test_support_modules.py ties those), split3w_support.WIDE_KNOBS the two that csrc/tdnn_split3w.hip reads
for its own kernel.  Every XVEC_ name that the sources of the frame-level path take from the environment is in one of the two
lists and in only one, so a test that creates its handles through split3w_support.make_model creates them under the knobs it
names and no others."""
import glob
import os
import re

import hipcc_support
import split3w_support
import tdnn_support

OTHER_PATHS = {"mfcc.hip": {"XVEC_MFCC_FILTERBANK"}}      # read by another entry point, not at handle creation


def _env_names(path):
    return set(re.findall(r'(?:getenv|env_int)\("(XVEC_\w+)"', open(path).read()))


def test_wide_knobs_are_the_ones_the_kernel_reads():
    assert _env_names(os.path.join(hipcc_support.CSRC, "tdnn_split3w.hip")) == set(split3w_support.WIDE_KNOBS)
    assert not set(split3w_support.WIDE_KNOBS) & set(tdnn_support.KNOBS)


def test_every_environment_name_of_the_library_is_listed():
    listed = set(tdnn_support.KNOBS) | set(split3w_support.WIDE_KNOBS)
    for path in sorted(glob.glob(os.path.join(hipcc_support.CSRC, "*.hip")) + glob.glob(os.path.join(hipcc_support.CSRC, "*.h"))):
        names = _env_names(path) - OTHER_PATHS.get(os.path.basename(path), set())
        assert names <= listed, f"{os.path.basename(path)} reads {sorted(names - listed)} from the environment: in no knob list"


def test_make_model_restores_the_environment(monkeypatch):
    """The wrapper's own bookkeeping, without a GPU: the two knobs are set only while the handle is created."""
    seen = {}
    monkeypatch.setattr(tdnn_support, "make_model", lambda sd, env, **kw: seen.update(env=dict(env), wide={k: os.environ.get(k) for k in split3w_support.WIDE_KNOBS}))
    monkeypatch.setenv("XVEC_SPLIT3_WIDE", "0")
    monkeypatch.delenv("XVEC_SPLIT3_WIDE_MIN_ROWS", raising=False)
    split3w_support.make_model(None, {"XVEC_SPLIT3_MIN_ROWS": "0", "XVEC_SPLIT3_WIDE_MIN_ROWS": "7"})
    assert seen["env"] == {"XVEC_SPLIT3_MIN_ROWS": "0"}
    assert seen["wide"] == {"XVEC_SPLIT3_WIDE": None, "XVEC_SPLIT3_WIDE_MIN_ROWS": "7"}
    assert os.environ.get("XVEC_SPLIT3_WIDE") == "0" and "XVEC_SPLIT3_WIDE_MIN_ROWS" not in os.environ
