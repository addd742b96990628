"""Whole BPF-A2C evaluation lock-steps on the GPU, fused and composed: 4 environments x 3 runs with 3 obstructions, a team of 2,
NP = 128, 8 lock-steps driven by hand -- every track through tests/_bpf_drive.py's check_track, every Fisher matrix and every policy
round against the restatement (tests/_bpf_a2c_ref.py) --, then the runner itself must log exactly these actions and return these
scores and bounds; the two forms agree; evaluate_PPO takes 'bpf-a2c'; and run_test_environments_rid_fim is what it was.

The policy round's restatement: the observation and the location are the numpy expressions bit for bit; the GRU state and the logits
are the package's float32 torch actor on them (rtol 1e-5 / atol 2e-6 on the state, as tests/test_rada2c_gpu.py holds K14); the
action must be the inverse-CDF draw of those probabilities from the step's uniform, give or take 1e-5 of cumulative probability (a uniform within
rounding of a CDF step may fall either side, as in tests/test_rada2c_gpu.py); the predicted position is the detector's plus the
controller's table, exactly; the score is the trace of the restatement's matrix there under the summation bound."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _bpf_a2c_ref as R2  # noqa: E402
from _bpf_drive import check_track  # noqa: E402

pytestmark = pytest.mark.gpu

E, R_, L, NP, A, SEED, OBST = 4, 3, 8, 128, 2, 23, 3
N = E * R_
AREA_MAX = 2200.0


@functools.lru_cache(maxsize=None)
def _sets():
    from radiation_ppo_amd import evaluate
    return evaluate.sample_test_environments(E, obstruction_count=OBST, seed=31)


@functools.lru_cache(maxsize=None)
def _agents():
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    out = {}
    for a in range(A):
        torch.manual_seed(400 + a)
        out[a] = RNNAgentPPO(id=a)
    return out


@functools.lru_cache(maxsize=None)
def _runner(fused, lanes_per_pass=None):
    from radiation_ppo_amd import evaluate
    return evaluate.run_test_environments_bpf_a2c(_agents(), _sets(), montecarlo_runs=R_, steps_per_episode=L, obstruction_count=OBST, seed=SEED,
                                                  return_actions=True, fused=fused, nParticles=NP, fisher=True, return_scores=True,
                                                  lanes_per_pass=lanes_per_pass)


def _check_fim(vec, bpf, alive8, pos, prior, F, tr=None):
    """the matrices F [N, A, 3, 3] (and traces) of one launch against the restatement, on the live lanes"""
    P = bpf.params
    xp, w, u = bpf.xp.cpu().numpy(), bpf.w.cpu().numpy(), bpf.draws()[0].cpu().numpy()
    det = pos.cpu().numpy() if pos is not None else np.stack([vec.state("x").t().cpu().numpy(), vec.state("y").t().cpu().numpy()], axis=-1).astype(np.float64)
    bkg, live, F = vec.state("bkg").cpu().numpy().reshape(-1), alive8.cpu().numpy() != 0, F.cpu().numpy()
    for n in np.flatnonzero(live):
        for a in range(A):
            if prior:
                want, mag = R2.fim_prior(R2.prior_particles(u[n, a].T, P.intensity, P.coord), det[n, a], float(bkg[n]), P.intensity, P.coord)
            else:
                want, mag = R2.fim(xp[n, a].T, w[n, a], det[n, a], float(bkg[n]))
            assert (np.abs(F[n, a] - want) <= R2.tol(NP, mag)).all(), (n, a, prior, F[n, a] - want, R2.tol(NP, mag))
            if tr is not None:
                assert abs(float(tr[n, a]) - R2.trace(want)) <= R2.tol(NP, R2.trace(mag)), (n, a)


@pytest.mark.parametrize("fused", [True, False])
def test_eight_lock_steps_step_by_step_and_through_the_runner(fused):
    import ctypes as C
    from radiation_ppo_amd import _lib, evaluate
    from radiation_ppo_amd.bpf import BootstrapParticleFilter
    from radiation_ppo_amd.pfgru import lane_base
    lib, agents, dev = _lib.load(), _agents(), torch.device("cuda:0")
    vec, keys, saved, obs, stat = evaluate._open(_sets(), R_, A, OBST, True, SEED, "cuda:0", welford=True, env_id_base=0)
    bpf = BootstrapParticleFilter(vec, nParticles=NP)
    track, fim = (bpf.track, bpf.fim) if fused else (bpf.track_composed, bpf.fim_composed)
    hid = evaluate._gru_team_h0(agents, lane_base(N, A, SEED, 0, dev), dev)
    if fused:                                                      # the start recurrent_team_start draws, without its bank
        assert torch.equal(hid, evaluate.recurrent_team_start(agents, N, SEED, dev, "hip")[1])
    wts = [agents[a].policy_weights() for a in range(A)]
    wp = (C.c_void_p * A)(*[w.data_ptr() for w in wts])
    p = lambda t: t.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    table = torch.from_numpy(R2.ACTION).cuda()
    alive = torch.ones(N, dtype=torch.bool, device=dev)
    u = torch.empty(N, A, dtype=torch.float32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    log, mats, scores = [], torch.full((L, N, A, 3, 3), float("nan"), **f64), torch.full((L, N, A), float("nan"), **f64)
    for t in range(L):
        a8v = alive.view(torch.uint8)
        vec.action_uniforms(u)
        check_track(vec, bpf, obs, a8v, t == 0, track)
        fim(a8v, prior=t == 0, F=mats[t])
        _check_fim(vec, bpf, a8v, None, t == 0, mats[t])
        # the policy round
        h0 = hid.clone()
        x, loc = torch.zeros_like(obs), torch.zeros(N, A, 2, dtype=torch.float32, device=dev)
        a8 = torch.full((N, A), 8, dtype=torch.int8, device=dev)
        sim = torch.zeros(N, A, 2, **f64)
        if fused:
            _lib.check(lib.rs_bpf_a2c_eval_step(vec._h, wp, A, p(obs), p(stat.mean), p(stat.std), p(bpf.estimate), AREA_MAX, p(hid), p(u), p(a8v),
                                                p(a8), p(sim), p(x), p(loc), st), "rs_bpf_a2c_eval_step")
        else:
            x.copy_(obs)
            x[..., 0] = ((obs[..., 0].double() - stat.mean) / stat.std).float().clamp(-8.0, 8.0)
            loc.copy_((bpf.estimate[..., 1:] / AREA_MAX).float())
            _lib.check(lib.rs_rnn_team_eval_step(wp, A, p(x), p(loc), p(hid), p(u), p(a8v), p(a8), N, st), "rs_rnn_team_eval_step")
            pos = torch.stack([vec.state("x").t(), vec.state("y").t()], dim=-1).double()
            sim.copy_(pos + table[a8.long().clamp(0, 7)])
        F = torch.zeros(N, A, 3, 3, **f64)
        fim(a8v, pos=sim, F=F, trace=scores[t])
        torch.cuda.synchronize()
        live = alive.cpu().numpy()
        xs = R2.standardise(obs[..., 0].cpu().numpy(), stat.mean.cpu().numpy(), stat.std.cpu().numpy())
        assert np.array_equal(x[..., 0].cpu().numpy()[live].view(np.int32), xs[live].view(np.int32))
        assert torch.equal(x[..., 1:][alive], obs[..., 1:][alive])
        ls = (bpf.estimate[..., 1:].cpu().numpy() / AREA_MAX).astype(np.float32)
        assert np.array_equal(loc.cpu().numpy()[live].view(np.int32), ls[live].view(np.int32))
        for a in range(A):
            logits, _, h1 = agents[a].agent.policy_step(x[:, a], loc[:, a], h0[a])
            assert torch.allclose(hid[a][alive], h1[alive], rtol=1e-5, atol=2e-6), (t, a)
            assert torch.equal(hid[a][~alive], h0[a][~alive])
            cdf = torch.cumsum(torch.softmax(logits.double(), dim=-1), dim=-1)
            k = a8[:, a].long().clamp(0, 7)
            lo = torch.where(k > 0, cdf.gather(1, (k - 1).clamp(min=0).view(-1, 1)).view(-1), torch.zeros_like(cdf[:, 0]))
            hi = torch.where(k < 7, cdf.gather(1, k.view(-1, 1)).view(-1), torch.full_like(cdf[:, 0], 2.0))
            ud = u[:, a].double()
            assert bool(((lo - 1e-5 <= ud) & (ud < hi + 1e-5))[alive].all()), (t, a)
        assert bool((a8[~alive] == 8).all()) and bool((a8[alive] < 8).all())
        pos = torch.stack([vec.state("x").t(), vec.state("y").t()], dim=-1).double()
        assert torch.equal(sim[alive], (pos + table[a8.long().clamp(0, 7)])[alive])
        _check_fim(vec, bpf, a8v, sim, False, F, scores[t].cpu().numpy())
        log.append(a8.cpu().numpy().copy())
        obs_n, rew, team, done, _ = vec.step(a8)
        alive &= ~done.bool().any(dim=1)
        stat.update(obs_n[..., 0], mask=alive)
        obs = obs_n.clone()
    m = mats.cpu().numpy()
    bounds = np.full((N, A, L, 3, 3), np.nan)
    for n in range(N):
        for a in range(A):
            T = int(np.isfinite(m[:, n, a]).all(axis=(1, 2)).sum())                    # the lane's lock-steps
            bounds[n, a, :T] = R2.pcrb(m[0, n, a], m[1:T, n, a], bpf_noise())
    results, summary, actions, extra = _runner(fused)
    assert np.array_equal(actions, np.stack(log)), (actions[:, :, 0], np.stack(log)[:, :, 0])
    assert summary["completed_runs"] == N
    assert extra["scores"].shape == (L, N, A) and np.allclose(extra["scores"], scores.cpu().numpy(), rtol=1e-12, atol=0.0, equal_nan=True)
    assert extra["bounds"].shape == (N, A, L, 3, 3) and np.allclose(extra["bounds"], bounds, rtol=1e-9, atol=0.0, equal_nan=True)
    assert np.isfinite(extra["bounds"][:, :, 0]).all() and np.isfinite(extra["scores"][0]).all()
    # the split into passes changes nothing: every lane keeps its key
    split = _runner(fused, 2 * R_)
    assert np.array_equal(split[2], actions) and split[0] == results
    assert all(np.array_equal(split[3][k], extra[k], equal_nan=True) for k in ("scores", "bounds"))


def bpf_noise():
    return (15.0, 1.0, 1.0)


def test_the_fused_and_the_composed_form_agree():
    f, c = _runner(True), _runner(False)
    assert np.array_equal(f[2], c[2])                              # action logs
    assert f[0] == c[0]                                            # records
    assert f[1]["success_rate"] == c[1]["success_rate"] and f[1]["completed_runs"] == c[1]["completed_runs"] == N


def test_other_widths_run_composed_only():
    from radiation_ppo_amd import evaluate
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    torch.manual_seed(77)
    ag = {0: RNNAgentPPO(id=0, actor_critic_args=dict(hidden=((16,),), hidden_sizes_pol=((8,),), hidden_sizes_val=((8,),)))}
    with pytest.raises(ValueError):
        evaluate.run_test_environments_bpf_a2c(ag, _sets(), montecarlo_runs=1, steps_per_episode=2, obstruction_count=OBST, fused=True, nParticles=16)
    out = evaluate.run_test_environments_bpf_a2c(ag, _sets(), montecarlo_runs=1, steps_per_episode=3, obstruction_count=OBST, seed=SEED,
                                                 return_actions=True, nParticles=16)
    assert out[2].shape == (3, E, 1) and out[1]["completed_runs"] == E and (out[2][0] < 8).all()


def test_evaluate_ppo_with_bpf_a2c_on_a_saved_set(tmp_path):
    import tarfile
    from radiation_ppo_amd.evaluate import evaluate_PPO
    name = "test_env_dict_obs3_high_v4"
    with tarfile.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "testset_files.tar.xz"), "r:xz") as tar:
        (tmp_path / name).write_bytes(tar.extractfile(name).read())
    for a, ag in _agents().items():
        ag.save(str(tmp_path / "models" / f"{a}_agent"))
    ev = evaluate_PPO(dict(test_env_path=str(tmp_path), obstruction_count=3, snr="high", episodes=4, montecarlo_runs=3, nParticles=200,
                           actor_critic_architecture="bpf-a2c", number_of_agents=2, steps_per_episode=12, enforce_boundaries=True, seed=2,
                           model_path=str(tmp_path / "models"), fisher=True))
    results, summary = ev.evaluate()
    assert len(results) == 4 and summary["completed_runs"] == 12 and 0.0 <= summary["success_rate"] <= 1.0
    bounds = ev.extras["bounds"]
    assert bounds.shape == (12, 2, 12, 3, 3) and np.isfinite(bounds[:, :, 0]).all()
    lens = np.array([l for r in results for l in r.total_episode_length])
    steps = np.isfinite(bounds).all(axis=(3, 4)).sum(axis=2)                       # a lane's bounds end with its run
    assert (steps == lens[:, None]).all(), (steps, lens)


def test_rid_fim_without_fisher_is_what_it_was():
    """the fisher launches change no action and no record; without them the return is the tuple it always was"""
    from radiation_ppo_amd import evaluate
    kw = dict(montecarlo_runs=R_, steps_per_episode=L, obstruction_count=OBST, seed=SEED, return_actions=True, nParticles=NP)
    plain = evaluate.run_test_environments_rid_fim(_sets(), **kw)
    assert len(plain) == 3
    off = evaluate.run_test_environments_rid_fim(_sets(), fisher=False, **kw)
    on = evaluate.run_test_environments_rid_fim(_sets(), fisher=True, **kw)
    assert len(off) == 3 and off[0] == plain[0] and np.array_equal(off[2], plain[2])
    assert len(on) == 4 and on[0] == plain[0] and np.array_equal(on[2], plain[2])
    assert sorted(on[3]) == ["bounds"] and on[3]["bounds"].shape == (N, 1, L, 3, 3) and np.isfinite(on[3]["bounds"][:, :, 0]).all()
