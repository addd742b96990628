"""Resources of the policy kernels that end in the action draw -- those that run the shared pieces (csrc/rs_action.hpp,
csrc/rs_cnn_head.hpp: rs_cnn_head_kernel, sk_heads_kernel) and those that keep the same text written out --
read from the built code object (tests/_kernel_meta.py).  Conditions, not measurements: the bounds are the numbers of the library built
at the commit before any piece was shared (cec4a92); moving a kernel onto a shared piece, or back, may cost it no scratch, no spill,
no LDS and no wave of occupancy."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

#   kernel                                    scratch  vgpr_spill  sgpr_spill  lds  waves per SIMD by registers    (the parent's)
PARENT = [
    ("rs_rnn_policy_kernel",                      68,   0,  298,      0, 2),   # 195 + 0 registers
    ("rs_rnn_team_step_kernel",                    0,   0,    0,      0, 2),   # 196 + 0 registers
    ("rs_rnn_team_collect_kernel",                 0,   0,    4,      0, 2),   # 201 + 0 registers
    ("rs_rnn_sized_step_kernelILi16E",             0,   0,   76,      0, 4),   # 115 + 0 registers
    ("rs_rnn_sized_step_kernelILi32E",             0,   0,  112,      0, 3),   # 163 + 0 registers
    ("rs_rnn_sized_step_kernelILi48E",             0,   0,  144,      0, 2),   # 210 + 0 registers
    ("rs_rnn_sized_step_kernelILi64E",             0,   0,  180,      0, 1),   # 257 + 1 registers
    ("rs_rnn_sized_team_kernelILi16E",             0,   0,   10,      0, 4),   # 119 + 0 registers
    ("rs_rnn_sized_team_kernelILi32E",             0,   0,   14,      0, 3),   # 167 + 0 registers
    ("rs_rnn_sized_team_kernelILi48E",             0,   0,   18,      0, 2),   # 215 + 0 registers
    ("rs_rnn_sized_team_kernelILi64E",             0,   0,   22,      0, 1),   # 264 + 8 registers
    ("rs_cnn_head_kernelILi8E",                    0,   0,    0,      0, 8),   # 53 + 0 registers
    ("rs_cnn_head_kernelILi1E",                    0,   0,    0,      0, 8),   # 51 + 0 registers
    ("rs_cnn_team_eval_head_kernel",               0,   0,    0,  36864, 2),   # 164 + 48 registers
    ("rs_cnn_sized_team_eval_head_kernel",         0,   0,    0,  36864, 1),   # 196 + 64 registers
    ("rs_cnn_team_step_head_kernel",               0,   0,    0,  36864, 2),   # 164 + 48 registers
    ("sk_first_layer_kernel",                      0,   0,    0,  36864, 2),   # 148 + 32 registers
    ("sk_heads_kernel",                            0,   0,    0,   9216, 8),   # 62 + 0 registers
    ("rs_ff_team_step_kernel",                     0,   0,    0,      0, 3),   # 168 + 0 registers
    ("rs_ff_eval_step_kernel",                     0,   0,    0,      0, 3),   # 155 + 0 registers
]
NO_MORE = ("scratch", "vgpr_spill", "sgpr_spill", "lds")


@pytest.mark.parametrize("row", PARENT, ids=[r[0] for r in PARENT])
def test_a_kernel_on_the_shared_pieces_needs_no_more_than_its_own_copy_did(row):
    k = M.one(M.library_kernels(), row[0])
    for key, bound in zip(NO_MORE, row[1:5]):
        assert k[key] <= bound, (key, bound, k)
    assert M.waves_by_vgpr(k["vgpr"] + k["agpr"]) >= row[5], (row[5], k)
