"""The policy kernels' step outputs -- actions, log-probabilities, values, GRU states, y1_out, the collectors' [A][3][N] rows -- against
the records of the commit at which every kernel still carried its own copy of the action draw and of the heads behind it
(tests/golden/policy_step_parent.npz, recorded by tests/golden/make_policy_step_parent.py): whichever kernels share a piece
(csrc/rs_action.hpp, csrc/rs_cnn_head.hpp) or keep their text, all compute the same, bit for bit, with and without a mask."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu

PARENT = K.maker("make_policy_step_parent")       # the recorder: its cases and its run()


def test_the_fixture_holds_every_case_in_both_forms_and_every_action():
    want = np.load(PARENT.OUT)
    assert {k.split(".")[0] for k in want.files} == set(PARENT.CASES)
    assert {k.split(".")[1] for k in want.files} == set(PARENT.FORMS)
    assert os.path.getsize(PARENT.OUT) < 1_000_000
    drawn = PARENT.actions_drawn({k: want[k] for k in want.files})
    assert set(drawn) == set(PARENT.DRAWS)
    for entry, acts in drawn.items():
        assert acts == list(range(8)), entry


def test_the_float64_references_alone_draw_every_action():
    """the seeds and scales of the recorder were chosen on the references, not on the kernels' output"""
    for entry, acts in PARENT.reference_coverage().items():
        assert acts == list(range(8)), entry


@pytest.mark.parametrize("case", list(PARENT.CASES))
def test_step_outputs_equal_the_parent_commits(case):
    """Today's outputs equal the fixture member by member -- keys, dtype, shape, bytes.  run() itself asserts that a masked form leaves
    the masked-out lanes of every output as they were."""
    want = np.load(PARENT.OUT)
    keys = sorted(k for k in want.files if k.startswith(case + "."))
    got = PARENT.run(case)
    assert sorted(got) == keys and len(keys) > 0
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
