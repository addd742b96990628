"""Resources of the two kernels of the recurrent agent's evaluation lock-step (csrc/rs_eval.hip), read from the built code object
(tests/_kernel_meta.py).  Conditions, not measurements: both are one-thread-per-lane bookkeeping kernels that run between launches
which are themselves a few microseconds long, so neither may keep anything in scratch or in static LDS."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

KERNELS = ["rs_rnn_eval_post_step_kernel", "rs_rnn_eval_post_refresh_kernel"]
#          key            bound
EXACT = [("scratch",      0),
         ("vgpr_spill",   0),
         ("sgpr_spill",   0),
         ("lds",          0)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key,bound", EXACT, ids=[k for k, _ in EXACT])
def test_rnn_eval_kernels_exact(kernel, key, bound):
    k = M.one(M.library_kernels(), kernel)
    assert k[key] == bound, k
