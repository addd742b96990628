"""Fixture of collected epochs: what RNNCollector and CNNCollector left after each of two epochs at commit d42dfd2 ("C binding: derive the
ctypes signatures and structs from the header"), the commit BEFORE each collector's two lock-steps (the glued one and its torch composition)
became one step over the two forms of ppo.CollectGlue.  The tests that hold the glued step to the composed one cannot see a change made to
both alike, such as a draw counter advanced one launch early; this recording can.  Only the collectors' public switches are used
(use_glue; glue, heads), so the recorder runs on that commit's tree and on every later one.

    rnn-A2, rnn-A1    RNNCollector, N = 80, T = 26, L = 8: two agents without obstacles, one agent with two (the shapes of
                      test_rada2c_gpu.py::test_glued_lock_step_equals_the_torch_composition); use_glue on and off
    cnn27-modules     CNNCollector at 27 x 27, N = 32, A = 3, T = 24, L = 7, global critic, heads = False; glue on and off
    cnn27, cnn34      the same in the default form, walls on (27 x 27) and off (34 x 34); glue on
Where a case lists two forms they were bit-identical at that commit, which main() asserts before it writes the one recording both are
replayed against (tests/test_collect_parent_gpu.py).

Recorded whole: act, rew, val, logp, last_val, cut, source_tar, the epoch statistics and the carried state (observation, returns, step
counters, Welford state, GRU states, draw counters, episodes_begun, complete_len, the stored cells, t).  Recorded as a bit-pattern checksum
(the int64 sum of the int32 view), because whole they would take several MB: the buffer's observation rows per (step, env), the stored maps
per step, the particle sets per (owner, env).  adv / ret are left out: rs_gae's outputs of recorded columns.  cnn27-modules has no
source_tar: at that commit the module path never wrote the column (nothing reads it in RAD-TEAM); the default form always did.

    python tests/golden/make_collect_parent.py [OUT.npz]   # on the MI355X; on a later tree it must reproduce the committed file
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "collect_parent.npz")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED, EPOCHS = 289714752, 2
COLUMNS = ("act", "rew", "val", "logp", "last_val", "cut", "source_tar")
# case: (kind, parameters, the forms of the glue that equal each other)
CASES = {
    "rnn-A2": ("rnn", dict(A=2, obst=0), (True, False)),
    "rnn-A1": ("rnn", dict(A=1, obst=2), (True, False)),
    "cnn27-modules": ("cnn", dict(walls=True, heads=False), (True, False)),
    "cnn27": ("cnn", dict(walls=True, heads=True), (True,)),
    "cnn34": ("cnn", dict(walls=False, heads=True), (True,)),
}


def checksum(t: torch.Tensor, lead: int) -> torch.Tensor:
    """int64 sum of the int32 view over everything behind the first `lead` dimensions"""
    t = t.contiguous()
    return t.view(torch.int32).reshape(*t.shape[:lead], -1).long().sum(dim=-1)


def _rnn(A, obst, glue):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector
    N, T, L = 80, 26, 8
    torch.manual_seed(4)
    env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=SEED, env_id_base=32)
    agents = {a: RNNAgentPPO(id=a, steps_per_epoch=T, steps_per_episode=L, seed=3 + a, train_pi_iters=1, train_pfgru_iters=1) for a in range(A)}
    with torch.no_grad():
        for ag in agents.values():
            for p in ag.agent.pi.parameters():
                p.mul_(2.0)
    col = RNNCollector(env, agents, T, L, use_graph=False)
    assert col.use_glue and col.use_k14 and col.bank.impl == "hip"
    col.use_glue = glue
    carried = lambda: {"c_h": col.h, "w_count": col.stat.count, "w_mean": col.stat.mean, "w_sq": col.stat.sq, "w_std": col.stat.std,
                       "pf_h.sum": checksum(col.bank.h, 2), "pf_p.sum": checksum(col.bank.p, 2), "pf_episode": col.bank.episode,
                       "pf_calls": col.bank.calls, "begun": col.episodes_begun}
    return col, COLUMNS, carried


def _cnn(walls, heads, glue):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic, heat_map_geometry
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    N, A, T, L = 32, 3, 24, 7
    torch.manual_seed(8)
    env = RadSearchVec(N, number_agents=A, obstruction_count=2, enforce_grid_boundaries=walls, seed=SEED, env_id_base=32)
    kw = dict(map_dim=tuple(heat_map_geometry(env, L, walls)[2]))
    gc = CNNCritic(**kw).cuda()
    agents = {i: CNNAgentPPO(id=i, GlobalCritic=gc, GlobalCriticOptimizer=torch.optim.Adam(gc.parameters(), lr=1e-3), **kw) for i in range(A)}
    with torch.no_grad():
        for ag in agents.values():
            for p in list(ag.pi.actor[6:].parameters()):
                p.mul_(3.0)                                   # visibly non-uniform policies
    col = CNNCollector(env, agents, T, L, global_critic_flag=True, use_graph=False)
    assert col.use_glue and tuple(col.maps.map_dimensions) == ((27, 27) if walls else (34, 34))
    col.glue, col.heads = glue, heads
    assert col.use_team_round == (walls and heads and glue) and col.use_sized_team_round == (not walls and heads and glue)
    carried = lambda: {"shared.sum": checksum(col.shared, 1), "cells": col.cells, "pcells": col.pcells, "complete_len": col.complete_len,
                       "pf_h.sum": checksum(col.predictor.h, 2), "pf_p.sum": checksum(col.predictor.p, 2),
                       "pf_episode": col.predictor.episode, "pf_calls": col.predictor.calls}
    return col, (COLUMNS if heads else COLUMNS[:-1]), carried


def run(case: str, glue: bool):
    """{member: array} of one case on cuda:0 with the glue in its HIP (True) or torch (False) form"""
    kind, c, forms = CASES[case]
    assert glue in forms
    col, columns, carried = (_rnn if kind == "rnn" else _cnn)(glue=glue, **c)
    out = {}
    for ep in range(EPOCHS):
        st = col.collect()
        got = {**{k: getattr(col.buf, k) for k in columns}, "obs.sum": checksum(col.buf.obs, 2), **{"stat_" + k: v for k, v in st.items()},
               "c_obs": col.obs, "c_ret": col.ep_ret, "c_steps": col.steps_in_ep, "t": col._t, **carried()}
        torch.cuda.synchronize()
        out.update({f"{case}.ep{ep}.{k}": v.detach().cpu().numpy().copy() for k, v in got.items()})
    assert col.env.error_flags() == 0
    return out


def covers(members) -> None:
    """every case cuts episodes before the epoch's end (timeouts at least) and bootstraps them"""
    for case in CASES:
        cut, last = members[f"{case}.ep0.cut"][:, :, 0], members[f"{case}.ep0.last_val"]
        assert cut[-1].all() and cut[:-1].any() and not cut[:-1].all() and (last[:-1] != 0).any(), case


def main():
    out = {}
    for case, (_, _, forms) in CASES.items():
        got = run(case, forms[0])
        for other in forms[1:]:
            again = run(case, other)
            for k in got:
                assert np.array_equal(got[k], again[k], equal_nan=True), (k, "the two forms differ")
        print(case, len(got), "members", sum(v.nbytes for v in got.values()), "bytes", flush=True)
        out.update(got)
    covers(out)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 893_657                                # the largest parent fixture before this one


if __name__ == "__main__":
    main()
