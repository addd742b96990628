"""The gradient-search controller on the GPU: rs_gs_eval_step against the reference controller over the oracle
(tests/_lookahead_ref.py), whole evaluation runs replayed action by action, the controller's success against a random walk, and
evaluate_PPO with 'gs' on a saved set of the reference's."""
import functools
import os
import sys
import tarfile

import numpy as np
import pytest
import torch

from oracle.radsearch_oracle import PhiloxDraws, RadSearchOracle

sys.path.insert(0, os.path.dirname(__file__))
import _eval_runs as V  # noqa: E402
import _lookahead_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 51
NMAX = 130
STEP_CASES = {1: (0, 1.0), 2: (3, 0.5), 8: (2, 4.0)}                # agents -> (obstructions, q)
CAP = 0.001                                                        # share of the draws that may be excluded near a CDF edge


def _alive(N):
    return (np.arange(N) % 5 != 3).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _step_reference(A):
    """NMAX oracle envs after 3 joint moves, and for each the reference controller's gradients, action and near-edge flag for the
    env's own uniforms.  Computed once: env n of a smaller RadSearchVec is env n of this one."""
    obst, q = STEP_CASES[A]
    rng = np.random.default_rng(A)
    acts = rng.integers(0, 8, size=(3, NMAX, A)).astype(np.int8)
    grad, act, edge = np.zeros((NMAX, A, 8), np.float32), np.zeros((NMAX, A), np.int64), np.zeros((NMAX, A), bool)
    for n in range(NMAX):
        e = RadSearchOracle(PhiloxDraws(SEED, n), number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True)
        for t in range(3):
            o = e.step({a: int(acts[t, n, a]) for a in range(A)})[0]
        obs0 = [float(np.float32(o[a][0])) for a in range(A)]
        act[n], edge[n], grad[n] = R.controller_action(e, obs0, R.action_uniforms(e), q)
    return acts, grad, act, edge


@pytest.mark.parametrize("A", [1, 2, 8])
@pytest.mark.parametrize("N", [1, 63, 64, 65, NMAX])
def test_gs_eval_step_matches_the_reference_controller(N, A):
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.envs import RadSearchVec
    obst, q = STEP_CASES[A]
    acts, rgrad, ract, redge = _step_reference(A)
    vec = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=SEED)
    vec.reset()
    for t in range(3):
        vec.step(torch.from_numpy(np.ascontiguousarray(acts[t, :N])).cuda())
    u = vec.action_uniforms(torch.empty(N, A, device="cuda"))
    alive = torch.from_numpy(_alive(N)).cuda()
    a8 = torch.full((N, A), -7, dtype=torch.int8, device="cuda")
    grad = torch.full((N, A, 8), float("nan"), device="cuda")
    p = lambda t: t.data_ptr()
    _lib.check(vec.lib.rs_gs_eval_step(vec._h, p(vec.obs), 1 / q, p(u), p(alive), p(a8), p(grad), vec._stream()), "rs_gs_eval_step")
    torch.cuda.synchronize()
    a8, grad, live = a8.cpu().numpy(), grad.cpu().numpy(), _alive(N).astype(bool)
    assert np.array_equal(grad[live].view(np.uint32), rgrad[:N][live].view(np.uint32))
    assert (grad[~live] == 0).all() and (a8[~live] == 8).all()                 # finished lanes: rows of 8, nothing looked at
    miss = a8[live] != ract[:N][live]
    print(f"N={N} A={A}: {int(miss.sum())} of {miss.size} actions differ from the float64 draw, {int(redge[:N][live].sum())} draws near an edge")
    assert (~miss | redge[:N][live]).all() and miss.sum() <= CAP * miss.size
    # the composed round of the evaluation (rs_peek + torch) on the same state: the same gradients
    _, moved, _, meas = vec.peek(lam=False)
    g = ((meas.double() - vec.obs[..., 0:1].double()) * 0.01 * (1 / q)).float()
    g = torch.where(moved.bool(), g, torch.zeros_like(g)).cpu().numpy()
    assert np.array_equal(g[live].view(np.uint32), rgrad[:N][live].view(np.uint32))


_REPLAYS = {}


def _replay(sets, actions, A, obst, seed, q, R_, L):
    """Every lane's logged actions followed in the oracle (tests/_eval_runs.py).  Returns per lane (steps, found, return) and the
    counts [draws, draws where the reference controller chose another action, of those the ones not near a CDF edge]; the same log is
    replayed once."""
    key = (A, obst, seed, q, actions.tobytes())
    if key in _REPLAYS:
        return _REPLAYS[key]
    counts = np.zeros(3, dtype=np.int64)

    def on_step(ref, o, t, n):
        want, edge, _ = R.controller_action(ref, [float(np.float32(o[a][0])) for a in range(A)], R.action_uniforms(ref), q)
        other = actions[t, n] != want
        counts[:] += (A, int(other.sum()), int((other & ~edge).sum()))

    lanes = V.replay_lane_per_run(sets, actions, A, R_, L, seed, obst, on_step=on_step)
    _REPLAYS[key] = (lanes, *counts.tolist())
    return _REPLAYS[key]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("obst", [0, 3])
def test_whole_runs_replay_through_the_oracle(obst, A, fused):
    from radiation_ppo_amd.evaluate import run_test_environments_gradient_search, sample_test_environments
    E, R_, L, seed, q = 8, 8, 30, 17, 1.0
    sets = sample_test_environments(E, obstruction_count=obst, seed=29)
    results, summary, actions = run_test_environments_gradient_search(sets, number_of_agents=A, q=q, montecarlo_runs=R_, steps_per_episode=L,
                                                                      obstruction_count=obst, seed=seed, return_actions=True, fused=fused)
    assert actions.shape[1:] == (E * R_, A) and actions.dtype == np.int8 and summary["completed_runs"] == E * R_
    lanes, draws, differ, unexplained = _replay(sets, actions, A, obst, seed, q, R_, L)
    print(f"obst={obst} A={A} fused={fused}: {differ} of {draws} logged actions differ from the float64 draw, {unexplained} away from a CDF edge")
    assert unexplained == 0 and differ <= CAP * draws
    V.check_records(results, lanes, R_)


def test_the_controller_searches():
    """8 obstacle-free environments x 16 runs, 120 steps: the gradient search finds at least half of the sources and at least twice
    as many as the uniform random walk the same runner gives at q = 1e30."""
    from radiation_ppo_amd.evaluate import run_test_environments_gradient_search, sample_test_environments
    sets = sample_test_environments(8, obstruction_count=0, seed=101)
    rate = {q: run_test_environments_gradient_search(sets, q=q, montecarlo_runs=16, steps_per_episode=120, seed=7)[1]["success_rate"]
            for q in (1.0, 1e30)}
    print("success rate:", rate)
    assert rate[1.0] >= 0.5 and rate[1.0] >= 2 * rate[1e30]


@pytest.mark.parametrize("A,name", [(1, "test_env_dict_obs0_high_v4"), (2, "test_env_dict_obs3_high_v4")])
def test_evaluate_ppo_with_gs_on_a_saved_set(tmp_path, A, name):
    from radiation_ppo_amd.evaluate import evaluate_PPO
    with tarfile.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testset_files.tar.xz"), "r:xz") as tar:
        (tmp_path / name).write_bytes(tar.extractfile(name).read())
    obst = int(name.split("_obs")[1].split("_")[0])
    ev = evaluate_PPO(dict(test_env_path=str(tmp_path), obstruction_count=obst, snr="high", episodes=6, montecarlo_runs=4,
                           actor_critic_architecture="gs", number_of_agents=A, steps_per_episode=40, enforce_boundaries=True, seed=2, q=1.0))
    results, summary = ev.evaluate()
    assert len(results) == 6 and summary["completed_runs"] == 24 and 0.0 <= summary["success_rate"] <= 1.0
    assert all(len(r.total_episode_length) == 4 and all(1 <= l <= 40 for l in r.total_episode_length) for r in results)
