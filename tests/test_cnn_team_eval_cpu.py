"""rs_cnn_team_trunk_infer and rs_cnn_team_eval_head without a GPU (their signatures, rs_cnn_head_params' layout and their export:
tests/test_abi_cpu.py): every invalid argument is refused with RS_ERR_INVALID_ARG before any HIP call (this machine has no device: a launch would have come
back as RS_ERR_HIP), the kernels' resources as the code objects state them, and the self-check of the float64 rule of
tests/_cnn_team_ref.py: the float32 torch composition passes it, and the mutations it must see fail it by a wide margin."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_team_ref as T  # noqa: E402
import _kernel_meta as M  # noqa: E402

from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG, RS_OK  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


# a valid call over fake (never dereferenced) addresses, then one argument spoilt per case
TRUNK_GOOD = dict(maps=0x1000, cells=0x2000, pcells=0x3000, num_agents=2, num_samples=64, wscratch=0x4000, a2=0x5000)
TRUNK_CASES = ([(f"{k} NULL", {k: None}) for k in ("maps", "cells", "pcells", "wscratch", "a2")]
               + [("no agent", dict(num_agents=0)), ("negative agents", dict(num_agents=-1)), ("nine agents", dict(num_agents=9)),
                  ("negative samples", dict(num_samples=-1)), ("no sample, a2 NULL", dict(num_samples=0, a2=None))])


@pytest.mark.parametrize("name,spoil", TRUNK_CASES, ids=[c[0] for c in TRUNK_CASES])
def test_team_trunk_refuses_invalid_arguments_before_any_hip_call(lib, name, spoil):
    a = dict(TRUNK_GOOD, **spoil)
    rc = lib.rs_cnn_team_trunk_infer(a["maps"], a["cells"], a["pcells"], a["num_agents"], a["num_samples"], a["wscratch"], a["a2"], None)
    assert rc == RS_ERR_INVALID_ARG, (name, rc)


def test_team_trunk_with_no_sample_is_ok_and_launches_nothing(lib):
    a = TRUNK_GOOD
    assert lib.rs_cnn_team_trunk_infer(a["maps"], a["cells"], a["pcells"], a["num_agents"], 0, a["wscratch"], a["a2"], None) == RS_OK


HEAD_GOOD = dict(heads=True, num_agents=2, a2=0x1000, u=0x2000, alive=0x3000, act8=0x4000, act=0x5000, logp=0x6000, y1_out=0x7000, num_envs=64)
HEAD_CASES = ([("heads NULL", dict(heads=False))] + [(f"{k} NULL", {k: None}) for k in ("a2", "u", "alive", "act8")]
              + [("no agent", dict(num_agents=0)), ("negative agents", dict(num_agents=-1)), ("nine agents", dict(num_agents=9)),
                 ("no env", dict(num_envs=0)), ("negative envs", dict(num_envs=-5)),
                 ("optional outputs NULL, a2 NULL", dict(act=None, logp=None, y1_out=None, a2=None))])


@pytest.mark.parametrize("name,spoil", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_team_head_refuses_invalid_arguments_before_any_hip_call(lib, name, spoil):
    from radiation_ppo_amd import _lib
    a = dict(HEAD_GOOD, **spoil)
    heads = (_lib.RsCnnHeadParams * _lib.RS_MAX_AGENTS)(*[_lib.RsCnnHeadParams(*[0x10000 * (i + 1) + 0x100 * k for k in range(6)])
                                                          for i in range(_lib.RS_MAX_AGENTS)])
    rc = lib.rs_cnn_team_eval_head(heads if a["heads"] else None, a["num_agents"], a["a2"], a["u"], a["alive"], a["act8"], a["act"], a["logp"],
                                   a["y1_out"], a["num_envs"], None)
    assert rc == RS_ERR_INVALID_ARG, (name, rc)


def test_team_head_refuses_a_null_pointer_inside_a_head(lib):
    from radiation_ppo_amd import _lib
    a = HEAD_GOOD
    heads = (_lib.RsCnnHeadParams * 2)(_lib.RsCnnHeadParams(1 << 12, 2 << 12, 3 << 12, 4 << 12, 5 << 12, 6 << 12),
                                       _lib.RsCnnHeadParams(1 << 12, 2 << 12, None, 4 << 12, 5 << 12, 6 << 12))
    assert lib.rs_cnn_team_eval_head(heads, 2, a["a2"], a["u"], a["alive"], a["act8"], None, None, None, 64, None) == RS_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ resources
def test_team_trunk_keeps_four_waves_per_simd_and_k9_stays_one_kernel():
    kernels = M.library_kernels()
    k = M.one(kernels, "rs_cnn_team_fwd_kernel")
    assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    k9 = M.one(kernels, "rs_cnn_fwd_kernelILi6E")                    # the refactoring left K9 one kernel under its name
    assert k9["vgpr"] <= 128 and k9["scratch"] == 0 and k9["vgpr_spill"] == 0, k9


def test_team_head_has_no_scratch_and_no_spills():
    k = M.one(M.library_kernels(), "rs_cnn_team_eval_head_kernel")
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["lds"] == 4 * 64 * 36 * 4, k                           # the four k-quarters of 64 images x 32 sums, rows padded to 36


# ------------------------------------------------------------------------------------------------ the rule's self-check
@pytest.fixture(scope="module")
def round_cpu():
    """One agent team on the CPU: a2 from torch's convolutions, the float64 reference of every agent, the float32 composition."""
    t = T.team(3)
    a2 = T.trunk_cpu(t)
    assert float(a2.min()) >= 0.0 and float((a2 == 0).float().mean()) > 0.2       # non-negative and sparse, as in a run
    N = T.MASTER
    alive = T.alive_for(t, N)
    assert 0 < int(alive.sum()) < N
    refs = [T.reference(t.actors[a].actor, a2[a], t.u[:, a]) for a in range(t.A)]
    return t, a2, alive, refs


def test_float32_torch_composition_passes_the_rule(round_cpu):
    t, a2, alive, refs = round_cpu
    for a in range(t.A):
        assert T.distinct_actions(refs[a]) >= 3, a
        y1, act, logp, act8 = T.torch32(t.actors[a].actor, a2[a], t.u[:, a], alive)
        q = T.ratios(refs[a], t.u[:, a], alive, act, logp, act8, y1=y1)
        print(f"float32 torch agent {a} | " + " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in q.items()))
        assert T.passes(q), (a, q)


def _seen(q):
    """a mutation is seen when it exceeds 100 x an allowance or differs in more draws (or action rows) than the cap"""
    return q["y1"] > 100.0 or q["logp"] > 100.0 or q["differing"] > T.DRAW_CAP or q["act8"] > T.DRAW_CAP


@pytest.mark.parametrize("quarter", range(4))
def test_the_rule_sees_a_dropped_k_quarter_of_the_first_layer(round_cpu, quarter):
    import copy
    t, a2, alive, refs = round_cpu
    for a in range(t.A):
        seq = copy.deepcopy(t.actors[a].actor)
        with torch.no_grad():
            seq[6].weight[:, 676 * quarter:676 * (quarter + 1)] = 0.0
        y1, act, logp, act8 = T.torch32(seq, a2[a], t.u[:, a], alive)
        q = T.ratios(refs[a], t.u[:, a], alive, act, logp, act8, y1=y1)
        assert q["y1"] > 100.0 and _seen(q) and not T.passes(q), (a, quarter, q)


def test_the_rule_sees_the_neighbour_lanes_uniform(round_cpu):
    t, a2, alive, refs = round_cpu
    for a in range(t.A):
        y1, act, logp, act8 = T.torch32(t.actors[a].actor, a2[a], torch.roll(t.u[:, a], 1), alive)
        q = T.ratios(refs[a], t.u[:, a], alive, act, logp, act8, y1=y1)
        assert q["differing"] > T.DRAW_CAP and q["unexcused"] > T.DRAW_CAP and not T.passes(q), (a, q)
    # ... and the neighbour AGENT's column
    y1, act, logp, act8 = T.torch32(t.actors[0].actor, a2[0], t.u[:, 1], alive)
    q = T.ratios(refs[0], t.u[:, 0], alive, act, logp, act8, y1=y1)
    assert q["differing"] > T.DRAW_CAP and not T.passes(q), q


def test_the_rule_sees_an_ignored_alive_flag(round_cpu):
    t, a2, alive, refs = round_cpu
    for a in range(t.A):
        y1, act, logp, _ = T.torch32(t.actors[a].actor, a2[a], t.u[:, a], alive)
        q = T.ratios(refs[a], t.u[:, a], alive, act, logp, act.to(torch.int8), y1=y1)
        assert q["act8"] == int((alive == 0).sum()) > T.DRAW_CAP and _seen(q) and not T.passes(q), (a, q)
