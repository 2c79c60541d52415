"""csrc/rec_plan.h: the one check of rec_start behind clustering (diar_plan.h), VBx (vbx_plan.h) and DER scoring (der_plan.h).
The same requests go to the three dump programs of tests/abi/; what they answer is one text per refusal (written once below),
with the unit's noun and its per-recording cap filled in (DER has no cap), and the size queries of the library answer 0 exactly
where the check refuses.  No GPU: the checks are host code."""
import ctypes as C

import numpy as np
import pytest

from hipcc_support import header_constants, host_program, needs_host_cxx

# unit: (the dump, the noun, the cap's constant in the unit's header or None, the counts of recordings that add up to exactly 2^31)
UNITS = {
    "diar": ("diar_plan_dump", "segment", "MAX_SEGMENTS", [2048] * 2 ** 20),
    "vbx": ("vbx_plan_dump", "frame", "MAX_FRAMES", [16384] * 131072),
    "der": ("der_plan_dump", "tick", None, [2 ** 30, 2 ** 30]),
}
AT_CAP = 16384      # what a unit without a cap is asked instead of its cap

# The one text of every answer; a unit fills in its noun, its cap's macro and value, and the last recording of its 2^31 list.
OVER = "refused recording 1 has {over} {noun}s, more than {cap_name} = {cap}"      # (DER has no cap: it answers ok)
EMPTY = "refused recording 1 is empty or rec_start decreases: every recording needs a {noun}"
NONE = "refused n_rec = 0: need at least one recording"
TOTAL = "refused 2147483648 {noun}s up to recording {last}: the total must stay below 2^31"


def _cases(unit):
    """[(request line, rec_start or None for a null pointer, n_rec, the answer)] in the order of the check's tests."""
    _, noun, const, full = UNITS[unit]
    prefix = f"XVEC_{unit.upper()}_"
    cap = header_constants(f"xvec_{unit}.h", prefix)[const] if const else None
    at = cap or AT_CAP
    fill = lambda text: text.format(noun=noun, cap_name=f"{prefix}{const}", cap=cap, over=at + 1, last=len(full) - 1)
    counts = lambda *n: (np.concatenate([[0], np.cumsum(np.asarray(n, dtype=np.int64))]), len(n))
    last = full[:-1] + [full[-1] - 1]              # one short of 2^31: the largest total
    return [
        ("check 3 4 5", *counts(3, 4, 5), "ok"),
        (f"check {at}", *counts(at), "ok"),
        (f"check 2 {at + 1}", *counts(2, at + 1), fill(OVER) if cap else "ok"),
        ("check 3 0 2", *counts(3, 0, 2), fill(EMPTY)),
        ("start 0 5 3", np.array([0, 5, 3]), 2, fill(EMPTY)),
        ("start 1 5", np.array([1, 5]), 1, "refused rec_start must begin at 0 (got 1)"),
        ("check", *counts(), NONE),
        ("nullstart 2", None, 2, "refused null pointer: rec_start"),
        ("nullstart 0", None, 0, NONE),            # the count is tested before the pointer
        ("check " + " ".join(map(str, full)), *counts(*full), fill(TOTAL)),
        ("check " + " ".join(map(str, last)), *counts(*last), "ok"),
    ]


@needs_host_cxx
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_every_answer_is_the_one_text_with_the_units_noun_and_cap(unit, tmp_path):
    cases = _cases(unit)
    assert host_program(UNITS[unit][0], tmp_path)([row[0] for row in cases]) == [row[3] for row in cases]
    # the texts a unit's own tests hold, spelt out once
    if unit == "vbx":
        assert cases[2][3] == "refused recording 1 has 16385 frames, more than XVEC_VBX_MAX_FRAMES = 16384"
        assert cases[9][3] == "refused 2147483648 frames up to recording 131071: the total must stay below 2^31"
    if unit == "der":
        assert cases[3][3] == "refused recording 1 is empty or rec_start decreases: every recording needs a tick"


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_size_query_answers_zero_exactly_where_the_check_refuses(unit):
    from xvector_amd import hip
    tail = {"diar": (), "vbx": (16, 5), "der": (0, 0)}[unit]
    query = getattr(hip.lib, {"diar": "xvec_ahc_workspace_bytes", "vbx": "xvec_vbx_workspace_bytes", "der": "xvec_der_workspace_bytes"}[unit])
    for line, rs, n_rec, answer in _cases(unit):
        host = None if rs is None else np.ascontiguousarray(rs, dtype=np.int64)
        need = query(None if host is None else host.ctypes.data_as(C.POINTER(C.c_int64)), n_rec, *tail)
        assert (need == 0) == answer.startswith("refused") and need % 256 == 0, line[:40]
