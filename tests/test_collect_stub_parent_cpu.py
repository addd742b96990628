"""RNNCollector's one lock-step over the torch form of ppo.CollectGlue, without a GPU, against the bits the composed lock-step of the
parent commit left (tests/golden/collect_stub_parent.npz, recorded by tests/golden/make_collect_stub_parent.py over its scripted env):
every buffer column, the epoch statistics, the carried state (observation, returns, step counters, Welford state, GRU states, particle
sets, draw counters, t) after each of two epochs, and the reset masks and action rows the env was given.  Glued-equals-composed cannot
see a change made to both forms alike, such as a call counter advanced one launch early; this can."""
import numpy as np
import torch

import _k7_bits as K

PARENT = K.maker("make_collect_stub_parent")


def test_rnn_lock_step_on_the_torch_glue_reproduces_the_parents_composed_step():
    want = K.golden("collect_stub_parent.npz")
    PARENT.covers(want)
    col = PARENT.collector()
    got = PARENT.drive(col)
    assert col._cg.impl == "torch"
    assert sorted(got) == sorted(want.files) and len(got) == 2 * 30 + 3
    for k in want.files:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(np.asarray(want[k]))), k
