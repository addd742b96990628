"""run_test_environments_team, run_test_environments_cnn_team and run_test_environments_cnn_team_sized against the records of the
commit at which each still had its own copy of the lock-step loop (tests/golden/eval_team_parent.npz, recorded by
tests/golden/make_eval_team_parent.py): the one loop under the three policy rounds computes the same, bit for bit, fused and composed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu

PARENT = K.maker("make_eval_team_parent")         # the recorder: its cases and its run()


def test_the_fixture_holds_every_case_in_both_forms():
    want = np.load(PARENT.OUT)
    assert {k.split(".")[0] for k in want.files} == set(PARENT.CASES)
    assert os.path.getsize(PARENT.OUT) < 1_000_000


@pytest.mark.parametrize("case", list(PARENT.CASES))
def test_team_runs_equal_the_parent_commits(case):
    """Today's results equal the fixture member by member -- keys, dtype, shape, bytes: every field of the records, the returns as
    float32 bits and the int8 action log, for fused=True and for fused=False.  Every log holds at least one non-idle row."""
    want = np.load(PARENT.OUT)
    keys = sorted(k for k in want.files if k.startswith(case + "."))
    got = PARENT.run(case)
    assert sorted(got) == keys and case + ".fused.id" in keys and case + ".composed.id" in keys
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    logs = [k for k in keys if k.endswith(".log")]
    assert len(logs) == (0 if case.endswith("-nolog") else 2)
    for k in logs:
        assert got[k].dtype == np.int8 and (got[k] < 8).all(axis=(1, 2)).any(), k
