"""rs_ridfim_eval_step on the GPU against the numpy restatement of the reference's FIC.optim_action (tests/_bpf_ref.py), whole
evaluation lock-steps checked step by step in both forms, and the controller's search against a random walk.

The controller rows are a generator's on top of a real env (which supplies detector positions, background rates in its own
range, the source and the true reading): intensity in the filter's units from the env's source (1e2..1e3), half the clouds the uniform
prior, half concentrated about the source (sigma 60 cm, sigma_I 50), Dirichlet(1) weights, the reading Poisson at the true rate (the
env's own observation), with readings of 0, 40 and 5000 forced on three rows and a lane parked in a corner, where five moves are blocked.

J_fish is held to its summation bound.  J is held to the summation bound -- (NP + 3 Z) * 2^-52 relative on each p_z and p_za, carried
through the logs -- and to nothing else, except for pmf terms exp(xlogy(z, lam) - gammaln(z + 1) - lam) whose exponent's terms have a
magnitude M so large that the reference's own half-ulp rounding of it exceeds that bound (u M > (NP + 3 Z) 2^-52: RULE in
tests/_bpf_ref.py; with 100 particles that is a reading above about 110): those get 6 u M on top, the uncertainty of the formula under
two math libraries, weighted by the term's share of its sum (about 1e-11 relative at a reading of 5000).  A row with no such term is
held to the summation bound alone; the test prints how the kernel stands against that bound on both kinds of row.  Nothing in the
allowance is fitted to the kernel's output.
The action must be the float64 argmax except on rows whose float64 top-two gap is inside twice the row's allowance (at most 1 % of the
rows); the latch must follow the float64 rule on every row."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _bpf_ref as R  # noqa: E402
from _bpf_drive import check_act, check_track, open_filter as _open  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 64, 0), (5, 1, 100, 3), (35, 2, 257, 0), (70, 1, 100, 3), (35, 2, 64, 3)]


def _craft(vec, bpf, rng):
    """the generator's clouds, weights and latches into bpf's state; returns the observation with the forced readings"""
    N, A, NP = bpf.N, bpf.A, bpf.NP
    src = np.stack([vec.state("src_x").cpu().numpy().reshape(-1), vec.state("src_y").cpu().numpy().reshape(-1)], axis=-1).astype(np.float64)
    inten = vec.state("intensity").cpu().numpy().reshape(-1) / 1e4
    xp = np.empty((N, A, 3, NP))
    for n in range(N):
        for a in range(A):
            if (n + a) % 2:
                xp[n, a, 0], xp[n, a, 1:] = rng.uniform(1e2, 1e3, NP), rng.uniform(0, 25e2, (2, NP))
            else:
                xp[n, a, 0] = np.clip(rng.normal(inten[n], 50, NP), 0, np.inf)
                xp[n, a, 1:] = src[n][:, None] + rng.normal(0, 60, (2, NP))
    w = rng.dirichlet(np.ones(NP), size=(N, A))
    bpf.xp.copy_(torch.from_numpy(xp))
    bpf.w.copy_(torch.from_numpy(w))
    bpf.logw.copy_(torch.from_numpy(np.log(w)))
    bpf.rdiv.copy_(torch.from_numpy(rng.integers(0, 2, size=(N, A)).astype(np.uint8)))
    obs = vec.obs.clone()
    for i, reading in enumerate((0.0, 40.0, 5000.0)):
        if i < N * A:
            obs.view(N * A, -1)[(i * 7) % (N * A), 0] = reading
            bpf.rdiv.view(-1)[(i * 7) % (N * A)] = 1
    return obs


def _alive(N):
    return torch.from_numpy((np.arange(N) % 5 != 3).astype(np.uint8)).cuda()


@pytest.mark.parametrize("N,A,NP,obst", CASES)
def test_controller_round_matches_the_float64_controller(N, A, NP, obst):
    vec, bpf = _open(N, A, obst, NP)
    rng = np.random.default_rng(N * 1000 + NP)
    for t in range(2):
        vec.step(torch.from_numpy(rng.integers(0, 8, size=(N, A)).astype(np.int8)).cuda())
    vec.state("x")[0, 0] = 50                                      # agent 0 of env 0 in the corner: moves 0, 1, 5, 6 and 7 are blocked
    vec.state("y")[0, 0] = 50
    obs = _craft(vec, bpf, rng)
    moved = vec.peek(lam=False, meas=False)[1].cpu().numpy()
    assert not moved[0, 0, [0, 1, 5, 6, 7]].any()
    rows, excused, act, worst = check_act(vec, bpf, obs, _alive(N), bpf.act)
    print(f"N={N} A={A} NP={NP} obst={obst}: {rows} rows, {excused} undecided in float64; worst J error {worst[0]:.3f} of the summation bound "
          f"on the {worst[2]} rows held to it alone, {worst[1]:.3f} of it on the others")
    assert excused <= 0.01 * rows
    assert act[0, 0] in (0, 2, 3, 4)                               # the five blocked moves tie; the lowest of them is 0


def test_the_latch_falls_and_ties_go_to_the_lowest_index():
    """Every detector in the corner at (50, 50), where moves 0, 1, 5, 6 and 7 stay put and give one J.  Lanes 0, 1: latch down (Fisher
    information) and the cloud in the corner behind the detector, so staying is best and the lowest of the five tied moves, 0, wins.
    Lanes 2, 3: latch up, a wide cloud over [0, 600]^2 and a reading of 100: the Renyi divergence is near 1 for every move (the
    restatement says so, on the CPU), above fim_thresh, and the latch falls."""
    N, A, NP = 4, 1, 128
    vec, bpf = _open(N, A, 0, NP)
    rng = np.random.default_rng(5)
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    vec.state("x")[0, :] = 50
    vec.state("y")[0, :] = 50
    xp = np.empty((N, A, 3, NP))
    xp[:2, :, 0] = rng.normal(800, 20, (2, A, NP))
    xp[:2, :, 1:] = 20.0 + rng.normal(0, 5, (2, A, 2, NP))
    xp[2:, :, 0] = rng.uniform(100, 1000, (2, A, NP))
    xp[2:, :, 1:] = rng.uniform(0, 600, (2, A, 2, NP))
    bpf.xp.copy_(torch.from_numpy(xp))
    bpf.w.fill_(1.0 / NP)
    bpf.logw.fill_(float(np.log(1.0 / NP)))
    bpf.rdiv.copy_(torch.tensor([[0], [0], [1], [1]], dtype=torch.uint8))
    obs = vec.obs.clone()
    obs[:, :, 0] = 100.0
    rows, excused, act, _ = check_act(vec, bpf, obs, alive, bpf.act)
    assert rows == 4 and excused == 0
    assert (act[:2, 0] == 0).all(), act
    assert (bpf.rdiv.cpu().numpy()[2:] == 0).all()


def test_a_nan_j_is_numpy_s_argmax_in_both_forms():
    """A particle exactly at the candidate position of move 4 (latch down): its Fisher term is nan, so J[4] is nan.  np.argmax returns
    the first nan index and np.max is nan, so the action is 4 and the latch stays -- fused and composed alike.  Lane 1 has no such
    particle and takes the ordinary argmax."""
    N, A, NP = 2, 1, 64
    vec, bpf = _open(N, A, 0, NP)
    rng = np.random.default_rng(9)
    vec.state("x")[0, :] = 1000
    vec.state("y")[0, :] = 1000
    xp = np.empty((N, A, 3, NP))
    xp[:, :, 0], xp[:, :, 1:] = rng.uniform(100, 1000, (N, A, NP)), rng.uniform(0, 2500, (N, A, 2, NP))
    xp[0, 0, 1, 5], xp[0, 0, 2, 5] = 1100.0, 1000.0
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    for call in (bpf.act, bpf.act_composed):
        bpf.xp.copy_(torch.from_numpy(xp))
        bpf.w.fill_(1.0 / NP)
        bpf.rdiv.zero_()
        a8 = torch.full((N, A), -7, dtype=torch.int8, device="cuda")
        J = torch.zeros(N, A, 8, dtype=torch.float64, device="cuda")
        call(vec.obs, alive, a8, J, None)
        J, a8 = J.cpu().numpy(), a8.cpu().numpy()
        assert np.isnan(J[0, 0]).tolist() == [False] * 4 + [True] + [False] * 3 and a8[0, 0] == 4 == int(np.argmax(J[0, 0]))
        assert np.isfinite(J[1, 0]).all() and a8[1, 0] == int(np.argmax(J[1, 0])) and (bpf.rdiv.cpu().numpy() == 0).all()


@pytest.mark.parametrize("fused", [True, False])
def test_eight_lock_steps_step_by_step_and_through_the_runner(fused):
    """4 environments x 3 runs, NP = 128: every track and every controller round of 8 lock-steps against the restatement, then the
    runner itself must log exactly these actions"""
    from radiation_ppo_amd import evaluate
    from radiation_ppo_amd.bpf import BootstrapParticleFilter
    E, R_, L, NP, seed, obst = 4, 3, 8, 128, 23, 3
    sets = evaluate.sample_test_environments(E, obstruction_count=obst, seed=31)
    vec, keys, saved, obs, _ = evaluate._open(sets, R_, 1, obst, True, seed, "cuda:0", welford=False, env_id_base=0)
    N = E * R_
    bpf = BootstrapParticleFilter(vec, nParticles=NP)
    track, act = (bpf.track, bpf.act) if fused else (bpf.track_composed, bpf.act_composed)
    alive = torch.ones(N, dtype=torch.bool, device="cuda")
    log, excused, rows = [], 0, 0
    for t in range(L):
        a8v = alive.view(torch.uint8)
        check_track(vec, bpf, obs, a8v, t == 0, track)
        r, e, a, _ = check_act(vec, bpf, obs, a8v, act)
        rows, excused = rows + r, excused + e
        log.append(a.copy())
        obs_n, rew, team, done, _ = vec.step(torch.from_numpy(a).cuda())
        alive &= ~done.bool().any(dim=1)
        obs = obs_n.clone()
    assert excused <= 0.01 * rows
    results, summary, actions = evaluate.run_test_environments_rid_fim(sets, montecarlo_runs=R_, steps_per_episode=L, obstruction_count=obst,
                                                                        seed=seed, return_actions=True, fused=fused, nParticles=NP)
    assert np.array_equal(actions, np.stack(log)), (actions[:, :, 0], np.stack(log)[:, :, 0])
    assert summary["completed_runs"] == N
    # the split into passes changes nothing: every lane keeps its key
    split = evaluate.run_test_environments_rid_fim(sets, montecarlo_runs=R_, steps_per_episode=L, obstruction_count=obst, seed=seed,
                                                   return_actions=True, fused=fused, nParticles=NP, lanes_per_pass=2 * R_, return_estimates=True)
    assert np.array_equal(split[2], actions) and split[3]["rmse"].shape == (N,) and np.isfinite(split[3]["final"]).all()


def test_the_controller_searches():
    """The 8 obstacle-free environments x 16 runs of tests/test_gs_eval_gpu.py, NP = 1000: RID-FIM finds more sources than the uniform
    random walk (gradient search at q = 1e30), and its median final localisation error is below that of the prior's mean (the centre
    of the prior box) on the same environments.  Both runs use the env's inverse-square falloff, the law the filter's measurement model
    states (core.py:594-596); under the env's reference falloff I / r the filter is mis-specified (see run_test_environments_rid_fim)."""
    from radiation_ppo_amd import evaluate
    sets = evaluate.sample_test_environments(8, obstruction_count=0, seed=101)
    _, summary, est = evaluate.run_test_environments_rid_fim(sets, montecarlo_runs=16, steps_per_episode=120, seed=7, nParticles=1000,
                                                             return_estimates=True, falloff="inverse_square")
    walk = evaluate.run_test_environments_gradient_search(sets, q=1e30, montecarlo_runs=16, steps_per_episode=120, seed=7,
                                                          falloff="inverse_square")[1]["success_rate"]
    src = np.repeat(np.array([sets[f"env_{i}"][0] for i in range(8)]), 16, axis=0)
    prior = np.sqrt(((src - 1250.0) ** 2).sum(axis=1))
    print(f"found: rid-fim {summary['success_rate']:.3f}, random walk {walk:.3f}; median final error {np.median(est['final']):.1f} cm, "
          f"prior mean {np.median(prior):.1f} cm, median rmse {np.median(est['rmse']):.1f} cm")
    assert summary["success_rate"] > walk
    assert np.median(est["final"]) < np.median(prior)


def test_evaluate_ppo_with_rid_fim_on_a_saved_set(tmp_path):
    import tarfile
    from radiation_ppo_amd.evaluate import evaluate_PPO
    name = "test_env_dict_obs3_high_v4"
    with tarfile.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testset_files.tar.xz"), "r:xz") as tar:
        (tmp_path / name).write_bytes(tar.extractfile(name).read())
    ev = evaluate_PPO(dict(test_env_path=str(tmp_path), obstruction_count=3, snr="high", episodes=4, montecarlo_runs=3, nParticles=200,
                           actor_critic_architecture="rid-fim", number_of_agents=2, steps_per_episode=12, enforce_boundaries=True, seed=2))
    results, summary = ev.evaluate()
    assert len(results) == 4 and summary["completed_runs"] == 12 and 0.0 <= summary["success_rate"] <= 1.0
