"""RNNCollector and CNNCollector against the epochs they collected before each collector's two lock-steps became one step over the two
forms of ppo.CollectGlue (tests/golden/collect_parent.npz, recorded by tests/golden/make_collect_parent.py: its cases, its members and
what is stored whole or as a checksum are described there).  Every form that was bit-identical to the recorded one then is replayed
against the same recording: the HIP glue and the torch glue of RAD-A2C (one and two agents) and of RAD-TEAM's module path, the HIP glue
of RAD-TEAM's default form at 27 x 27 and walls off."""
import numpy as np
import pytest

import _k7_bits as K

pytestmark = pytest.mark.gpu
PARENT = K.maker("make_collect_parent")       # the recorder: its cases and its run()
GOLD = K.golden("collect_parent.npz")
RUNS = [(case, glue) for case, (_, _, forms) in PARENT.CASES.items() for glue in forms]


def test_the_recording_cuts_and_bootstraps_in_every_case():
    PARENT.covers(GOLD)
    assert sorted({k.split(".")[0] for k in GOLD.files}) == sorted(PARENT.CASES)


@pytest.mark.parametrize("case,glue", RUNS, ids=[f"{case}-{'hip' if glue else 'torch'}-glue" for case, glue in RUNS])
def test_collected_epochs_equal_the_parents(case, glue):
    got = PARENT.run(case, glue)
    want = {k: GOLD[k] for k in GOLD.files if k.startswith(case + ".")}
    assert sorted(got) == sorted(want) and len(want) >= 2 * 20
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w, equal_nan=True), k
