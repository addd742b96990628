"""Monte-Carlo evaluation on saved test environments: the device-side mirror of `EpisodeRunner.run`
(algos/multiagent/evaluate.py:333-476) for the RAD-A2C-style branch (2x64 MLP policy, per-episode standardisation
of the reading).

The reference walks one saved environment at a time: `refresh_environment` (rad_search_env.py:799-874), act until
the source is found or `steps_per_episode` is reached, record, refresh again, `montecarlo_runs` times.  Here every
(saved environment, Monte-Carlo run) pair is one env of a `RadSearchVec` -- E x R episodes advance in lock-step, each
with its own Philox stream -- and the same per-environment records come out (`MonteCarloResults`, same field names).

Saved sets use the reference's layout `env_dict["env_<i>"] = (src_coords, det_coords, intensity, bkg[, obstacles])`
(algos/test_environment/eval/test_env_gen.py:13-24).  `sample_test_environments` draws such a set from the
environment's own spawn rules; the reference's own pickled sets are read by radiation_ppo_amd.testsets WITHOUT unpickling.
`run_test_environments_cnn` is the same runner for RAD-TEAM (CNN) policies, `run_test_environments_cnn_team` its HIP lock-step for teams
of up to 8 on 27 x 27 maps (csrc/rs_cnn.hip, csrc/rs_cnn_eval.hip), `run_test_environments_cnn_team_sized` the same for square maps of
any side 8..256 (walls off: 147 x 147; csrc/rs_cnn_sized.hip, csrc/rs_cnn_eval.hip), `run_test_environments_team` for feed-forward agents and
teams of up to 8 -- these three are fronts to one lock-step loop, `_run_lane_per_run_team` --, `run_test_environments_rnn_team` for recurrent (RAD-A2C) teams of 1 to 8 -- it holds the recurrent lock-step, fused in
HIP (csrc/rs_eval.hip, csrc/rs_rnn_policy.hip) and composed; `run_test_environments_rnn` is its front for one agent, and
`run_test_environments` sends a recurrent agent there --, `run_test_environments_gradient_search` the reference's non-learned
gradient-search controller over the env's look-ahead (csrc/rs_lookahead.hip), a fourth front to `_run_lane_per_run_team` --,
`run_test_environments_rid_fim` the reference's bootstrap particle filter with the RID-FIM controller (csrc/rs_bpf.hip,
radiation_ppo_amd/bpf.py), a fifth --, `run_test_environments_bpf_a2c` the reference's 'bpf-a2c', the trained recurrent actor fed that
filter's location estimate (csrc/rs_rnn_policy.hip: rs_bpf_a2c_eval_step), a sixth; both take `fisher` for the posterior Cramer-Rao
bound (rs_bpf_fim, bpf.pcrb) --,
`summarize` the result statistics
(evaluate.py:645-880), `evaluate_PPO` the driver with the reference's eval_kwargs (:581-643).
"""
import ctypes as C
import inspect
import os
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Any, Dict, List

import numpy as np
import torch

from . import _lib
from .envs import RadSearchVec
from .ppo import DeviceWelford, VecAgentPPO, mlp_params


@dataclass
class Results:                           # evaluate.py:34-40
    episode_length: List[int] = field(default_factory=list)
    episode_return: List[float] = field(default_factory=list)
    intensity: List[int] = field(default_factory=list)
    background_intensity: List[int] = field(default_factory=list)


@dataclass
class MonteCarloResults:                 # evaluate.py:60-68
    id: int
    completed_runs: int = 0
    success_counter: int = 0
    total_episode_length: List[int] = field(default_factory=list)
    successful: Results = field(default_factory=Results)
    unsuccessful: Results = field(default_factory=Results)


def median(data) -> np.float32:          # evaluate.py:78-80
    return np.median(data) if len(data) > 0 else np.nan


def sample_test_environments(count: int, obstruction_count: int = 0, enforce_grid_boundaries: bool = True, seed: int = 0,
                             device: str = "cuda:0", **env_kwargs: Any) -> Dict[str, tuple]:
    """A set of saved test environments in the reference's format, drawn by the environment's own reset."""
    vec = RadSearchVec(count, number_agents=1, obstruction_count=obstruction_count,
                       enforce_grid_boundaries=enforce_grid_boundaries, seed=seed, device=device, **env_kwargs)
    vec.reset()
    sx, sy = vec.state("src_x")[0].cpu().numpy(), vec.state("src_y")[0].cpu().numpy()
    x, y = vec.state("x")[0].cpu().numpy(), vec.state("y")[0].cpu().numpy()
    inten, bkg = vec.state("intensity")[0].cpu().numpy(), vec.state("bkg")[0].cpu().numpy()
    nob = vec.state("num_obs")[0].cpu().numpy()
    rect = vec.state("rect").cpu().numpy()                       # [28, G]
    out = {}
    for i in range(count):
        e = [np.array([float(sx[i]), float(sy[i])]), np.array([float(x[i]), float(y[i])]), int(inten[i]), int(bkg[i])]
        if obstruction_count != 0:
            obs = []
            for k in range(int(nob[i])):
                x0, y0, x1, y1 = (float(rect[4 * k + j, i]) for j in range(4))
                obs.append([np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]])])
            e.append(obs)
        out["env_" + str(i)] = tuple(e)
    return out


def _pack(env_sets: Dict[str, tuple], runs: int, with_obstacles: bool, device):
    keys = sorted(env_sets, key=lambda k: int(k.split("_")[1]))
    E = len(keys)
    src = np.zeros((E, 2), dtype=np.int32); det = np.zeros((E, 2), dtype=np.int32)
    inten = np.zeros(E, dtype=np.int32); bkg = np.zeros(E, dtype=np.int32)
    nob = np.zeros(E, dtype=np.int32); rects = np.zeros((E, _lib.RS_MAX_OBS, 4), dtype=np.int32)
    for i, k in enumerate(keys):
        e = env_sets[k]
        for arr, p in ((src, e[0]), (det, e[1])):
            q = np.asarray(p, dtype=np.float64)
            if not np.all(q == np.round(q)):
                raise ValueError("saved coordinates must lie on the 1 cm lattice")
            arr[i] = q.astype(np.int32)
        inten[i], bkg[i] = int(e[2]), int(e[3])
        if with_obstacles:
            obstacles = e[4]
            if len(obstacles) > _lib.RS_MAX_OBS:
                raise ValueError("more than 7 obstructions")
            nob[i] = len(obstacles)
            for j, ob in enumerate(obstacles):
                pts = np.asarray(ob[0], dtype=np.float64)
                rects[i, j] = (pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max())
    rep = lambda a: torch.from_numpy(np.repeat(a, runs, axis=0)).to(device).contiguous()      # env e*runs + r
    return keys, rep(src), rep(det), rep(inten), rep(bkg), (rep(nob) if with_obstacles else None), (rep(rects) if with_obstacles else None)


def _open(env_sets, lanes_per_env, number_agents, obstruction_count, enforce_grid_boundaries, seed, device, welford=True, **vec_kwargs):
    """The opening of every runner: a RadSearchVec of `lanes_per_env` lanes per saved environment with every lane's episode loaded.
    Returns (vec, keys, saved, obs, stat): the set's keys in order, saved = (src, det, inten, bkg, nob, rects) per lane -- what
    vec.refresh takes --, the first observation and, with welford, every agent's statistics buffer holding its first reading."""
    dev = torch.device(device)
    N = len(env_sets) * lanes_per_env
    vec = RadSearchVec(N, number_agents=number_agents, obstruction_count=obstruction_count, enforce_grid_boundaries=enforce_grid_boundaries,
                       seed=seed, device=device, **vec_kwargs)
    keys, *saved = _pack(env_sets, lanes_per_env, obstruction_count != 0, dev)
    vec.reset()                                                   # a valid handle state; every episode is then loaded
    obs = vec.refresh(*saved)[0].clone()
    stat = None
    if welford:
        stat = DeviceWelford((N, number_agents), dev)             # evaluate.py:362-367: one statistics buffer per agent
        stat.update(obs[..., 0])
    return vec, keys, saved, obs, stat


def _has_policy_kernel(ac, dev) -> bool:
    """The recurrent agent's policy step (GRU cell, heads, draw) has a HIP kernel on this device: K14 at the default widths, the sized
    step at the others."""
    return ac.fused_policy or (ac.sized_policy and dev.type == "cuda")


def _has_pfgru_kernel(ac, dev) -> bool:
    """The same for the agent's PFGRU location predictor: K11 at 24 hidden units, the sized step at the other widths."""
    return ac.fused_pfgru or (ac.sized_pfgru and dev.type == "cuda")


def recurrent_team_start(agents, N, seed, dev, impl):
    """`hiddens` of N lanes of a team {id: RNNAgentPPO} of equal widths as an evaluation creates them, once (evaluate.py:353, :357):
    ONE PredictorBank of A owners around the agents' own PFGRUs with its particle sets drawn, and every agent's GRU state from the hash
    of ITS row of the bank's lane keys (every agent has its own `hiddens` entry).  The composed and the fused runners start from this one
    definition, so their initial states cannot drift apart.  Returns (bank, hid [A, N, hid])."""
    from .pfgru import PredictorBank
    A = len(agents)
    ac0 = agents[0].agent
    bank = PredictorBank(N, A, hidden_size=ac0.rec, seed=seed, carry_hidden=True, device=dev, impl=impl)
    for a in range(A):
        bank.cells[a] = agents[a].agent.model
    bank.reset()
    return bank, _gru_team_h0(agents, bank._base, dev)


def _gru_team_h0(agents, base, dev):
    """hid [A, N, hid]: every agent's GRU state from the hash of ITS row of the lane keys `base` [A, N] (pfgru.lane_base)."""
    from .pfgru import hash_uniform
    unit = torch.arange(agents[0].agent.hid, dtype=torch.int64, device=dev).view(1, -1)
    hid = torch.stack([agents[a].agent.gru_h0(hash_uniform((base[a] * 1000003 + 5).view(-1, 1) * 1048583 + unit)) for a in range(len(agents))])
    return hid.contiguous()


def recurrent_start(ac, N, seed, dev, impl):
    """recurrent_team_start for the one actor-critic `ac` (an RNNModelActorCritic, not its RNNAgentPPO).  Returns (bank, hid [N, hid])."""
    bank, hid = recurrent_team_start({0: SimpleNamespace(agent=ac)}, N, seed, dev, impl)
    return bank, hid[0]


def _lane_records(N, dev):
    """(alive, ep_len, ep_ret, success) of N lanes that run one episode each."""
    return (torch.ones(N, dtype=torch.bool, device=dev), torch.zeros(N, dtype=torch.int32, device=dev),
            torch.zeros(N, dtype=torch.float32, device=dev), torch.zeros(N, dtype=torch.bool, device=dev))


def _book_step(alive, ep_len, ep_ret, success, r, done) -> None:
    """One lock-step of the lane-per-run records, in place: reward r and the episode-over flag `done` count on the lanes still alive
    (finished lanes keep stepping; their records are frozen)."""
    ep_ret += torch.where(alive, r, torch.zeros_like(r))          # evaluate.py:400-406 (float32 accumulation)
    ep_len += alive.int()
    found = done & alive
    success |= found
    alive &= ~found


def _close(vec, keys, saved, R, ep_len, ep_ret, success, log=None, ignore_flags=0):
    """The closing of every runner: the env's error flags (those in ignore_flags excepted) raise, the records of the E * R runs, in
    (environment, run) order, become the per-environment results and their summary; a runner that kept an action log passes it as a
    device tensor.  keys and saved are _open's."""
    flags = vec.error_flags() & ~ignore_flags
    if flags:
        raise RuntimeError(f"RadSearch env error flags 0x{flags:x}")
    inten, bkg = (t.repeat_interleave(len(ep_len) // len(t)) for t in saved[2:4])     # a lane that ran several runs: once per run
    out = _collect_results(keys, len(keys), R, ep_len, ep_ret, success, inten, bkg)
    if log is None:
        return out, summarize(out)
    return out, summarize(out), log.cpu().numpy()


@torch.no_grad()
def run_test_environments(agent: VecAgentPPO, env_sets: Dict[str, tuple], montecarlo_runs: int = 100, steps_per_episode: int = 120,
                          obstruction_count: int = 0, enforce_grid_boundaries: bool = True, seed: int = 0,
                          device: str = "cuda:0", return_actions: bool = False, falloff: str = "reference",
                          carry_hidden_across_runs: bool = False):
    """EpisodeRunner.run for every saved environment at once.  Returns (List[MonteCarloResults] in set order, summary
    dict with the statistics `evaluate.py:776-828` prints); with return_actions also the [steps, E*R] action log.

    A recurrent agent (RAD-A2C) goes to run_test_environments_rnn(fused=False), the composed lock-step of the team runner with one
    agent, and carry_hidden_across_runs is that runner's: the reference creates `hiddens` ONCE per EpisodeRunner.run (evaluate.py:357)
    and between Monte-Carlo runs resets only the statistics buffer (:455-470), so run k + 1 of an environment starts from the GRU /
    PFGRU state run k ended in.  True reproduces that (one lane per saved environment, its runs one after the other); False gives
    every (environment, run) pair its own lane and a fresh hidden state -- R times fewer lock-steps, a deviation from the reference.
    `evaluate_PPO` uses True.  With return_actions the log of a recurrent agent is that runner's: int8 [lock-steps run, lanes], the
    action rows the env received, 8 (idle) wherever a lane had no run going.  A feed-forward policy has no hidden state, the flag means
    nothing to it, and its log is int64 and keeps the unused draws of finished lanes."""
    if hasattr(agent.agent, "gru_cell"):
        return run_test_environments_rnn(agent, env_sets, montecarlo_runs=montecarlo_runs, steps_per_episode=steps_per_episode,
                                         obstruction_count=obstruction_count, enforce_grid_boundaries=enforce_grid_boundaries, seed=seed,
                                         device=device, return_actions=return_actions, falloff=falloff,
                                         carry_hidden_across_runs=carry_hidden_across_runs, fused=False)
    R, L = montecarlo_runs, steps_per_episode
    N = len(env_sets) * R
    dev = torch.device(device)
    ac = agent.agent
    vec, keys, saved, obs, stat = _open(env_sets, R, 1, obstruction_count, enforce_grid_boundaries, seed, device, falloff=falloff)
    alive, ep_len, ep_ret, success = _lane_records(N, dev)
    u = torch.empty(N, 1, dtype=torch.float32, device=dev)
    act8 = torch.empty(N, 1, dtype=torch.int8, device=dev)
    log = []
    for _ in range(L):
        x = obs.clone()
        stat.standardize(obs[..., 0], out=x[..., 0])
        vec.action_uniforms(u)
        a, _, _ = ac.act(x[:, 0], u[:, 0])                        # ac.step: sample from the policy (evaluate.py:373-383)
        act8[:, 0] = torch.where(alive, a, torch.full_like(a, 8)).to(torch.int8)      # finished episodes idle in place
        if return_actions:
            log.append(a.clone())
        obs_n, rew, _, done, _ = vec.step(act8)
        _book_step(alive, ep_len, ep_ret, success, rew[:, 0], done[:, 0].bool())
        stat.update(obs_n[..., 0], mask=alive)
        obs = obs_n.clone()
        if not bool(alive.any()):
            break
    return _close(vec, keys, saved, R, ep_len, ep_ret, success, log=torch.stack(log) if return_actions else None)


def run_test_environments_rnn(agent, env_sets: Dict[str, tuple], montecarlo_runs: int = 100, steps_per_episode: int = 120,
                              obstruction_count: int = 0, enforce_grid_boundaries: bool = True, seed: int = 0, device: str = "cuda:0",
                              return_actions: bool = False, falloff: str = "reference", carry_hidden_across_runs: bool = True,
                              fused=None):
    """EpisodeRunner.run (evaluate.py:333-476) for the recurrent agent (RAD-A2C): run_test_environments_rnn_team with the team
    {0: agent} -- its lanes, its hidden-state lifetimes (carry_hidden_across_runs), its fused and composed lock-steps, its records.
    fused=True needs a cuda device and a kernel for both halves of the agent (fused_policy or sized_policy, fused_pfgru or sized_pfgru);
    ValueError otherwise.  fused=None: the fused form where it can run.

    Returns (List[MonteCarloResults], summary); with return_actions also the [lock-steps run, N] int8 log of rs_step's action rows, 8
    (idle) where a lane had no run going -- N = E with carried hidden states, else E * R."""
    dev = torch.device(device)
    ac = getattr(agent, "agent", None)
    can = (dev.type == "cuda" and hasattr(ac, "gru_cell") and hasattr(agent, "policy_weights")
           and _has_policy_kernel(ac, dev) and _has_pfgru_kernel(ac, dev))
    if fused is None:
        fused = can
    if fused and not can:
        raise ValueError("the fused evaluation needs a cuda device, a GRU of 1..64 units with single-layer heads of 2..64 units and a "
                         "PFGRU of 8, 16, .., 64 hidden units")
    res = run_test_environments_rnn_team({0: agent}, env_sets, montecarlo_runs=montecarlo_runs, steps_per_episode=steps_per_episode,
                                         obstruction_count=obstruction_count, enforce_grid_boundaries=enforce_grid_boundaries, seed=seed,
                                         device=device, return_actions=return_actions, falloff=falloff,
                                         carry_hidden_across_runs=carry_hidden_across_runs, fused=fused)
    return res[:2] + (res[2][:, :, 0],) if return_actions else res


@torch.no_grad()
def run_test_environments_rnn_team(agents: Dict[int, Any], env_sets: Dict[str, tuple], montecarlo_runs: int = 100, steps_per_episode: int = 120,
                                   obstruction_count: int = 0, enforce_grid_boundaries: bool = True, seed: int = 0, device: str = "cuda:0",
                                   return_actions: bool = False, falloff: str = "reference", carry_hidden_across_runs: bool = True,
                                   fused=None):
    """EpisodeRunner.run (evaluate.py:333-476) for a team of 1..8 recurrent agents (RAD-A2C, team_mode "individual": :279-280) with
    its lock-step in HIP.  agents: {id: RNNAgentPPO}, ids 0..A-1, all of the same widths.  Every agent has its own network (:305-318),
    its own GRU state and particle set, created once (:353), and its own statistics buffer (:361-364, :395-397, :461-466); a run ends
    when any agent's terminal flag rises (:411-423) or at `steps_per_episode`; agent 0's return is recorded (:441-444).
    carry_hidden_across_runs: True = N = E lanes with R runs each, one after the other on carried hidden states (the reference's
    lifetime of `hiddens`, :353); False = N = E R lanes with one run each and a fresh hidden state.

    fused=True: a lock-step is rs_action_uniforms, the PFGRU step of every owner on the lanes with runs left (one launch), the policy
    round -- one launch for the team: rs_rnn_team_eval_step at the default widths, rs_rnn_sized_team_step at the others --,
    rs_step, rs_rnn_team_eval_post_step and, with more than one run per lane, rs_refresh on the lanes that begin their next run and
    rs_rnn_team_eval_post_refresh: 5 or 7 launches, on one stream.  The host reads the finished-lane count once
    every 16 lock-steps; nothing else synchronises.  It needs a cuda device and kernels for both halves of the agents; ValueError
    otherwise.  fused=False: the same lock-step composed from DeviceWelford, PredictorBank.predict, one policy step per agent and
    torch bookkeeping in the reference's order, with the same stopping rule: the A/B baseline, identical records and log.
    fused=None: the fused form where it can run.

    Returns (List[MonteCarloResults], summary); with return_actions also the [lock-steps run, N, A] int8 log of rs_step's action rows,
    8 (idle) where a lane had no run going."""
    A = len(agents)
    if sorted(agents) != list(range(A)) or not 1 <= A <= _lib.RS_MAX_AGENTS:
        raise ValueError(f"agents must carry the ids 0..A-1 with A in 1..{_lib.RS_MAX_AGENTS}")
    acs = [getattr(agents[a], "agent", None) for a in range(A)]
    if not all(hasattr(ac, "gru_cell") for ac in acs):
        raise ValueError("run_test_environments_rnn_team evaluates recurrent (RAD-A2C) agents")
    if len({(ac.hid, tuple(ac.pol), tuple(ac.val), ac.rec) for ac in acs}) != 1:
        raise ValueError("the agents of a team must have the same GRU, head and PFGRU widths: the bank and the state tensor hold one width")
    E, R, L = len(env_sets), montecarlo_runs, steps_per_episode
    dev = torch.device(device)
    pol_kernel = all(_has_policy_kernel(ac, dev) for ac in acs)
    pf_kernel = all(_has_pfgru_kernel(ac, dev) for ac in acs)
    can = dev.type == "cuda" and pol_kernel and pf_kernel and all(hasattr(agents[a], "policy_weights") for a in range(A))
    if fused is None:
        fused = can
    if fused and not can:
        raise ValueError("the fused evaluation needs a cuda device, a GRU of 1..64 units with single-layer heads of 2..64 units and a "
                         "PFGRU of 8, 16, .., 64 hidden units")
    Rl = R if carry_hidden_across_runs else 1                     # runs per lane
    N = E * R // Rl
    vec, keys, saved, obs, stat = _open(env_sets, R // Rl, A, obstruction_count, enforce_grid_boundaries, seed, device, falloff=falloff)
    bank, hid = recurrent_team_start(agents, N, seed, dev, "hip" if pf_kernel else "torch")   # particle sets and h0 are drawn here only
    run = torch.zeros(N, dtype=torch.int32, device=dev)
    steps = torch.zeros(N, dtype=torch.int32, device=dev)
    ret = torch.zeros(N, dtype=torch.float32, device=dev)
    rec_len = torch.zeros(N, Rl, dtype=torch.int32, device=dev)
    rec_ret = torch.zeros(N, Rl, dtype=torch.float32, device=dev)
    rec_suc = torch.zeros(N, Rl, dtype=torch.uint8, device=dev)
    u = torch.empty(N, A, dtype=torch.float32, device=dev)
    bound = L * Rl
    # with return_actions the action rows of lock-step t are written straight into row t of the log, which rs_step then reads; a lane
    # that is masked out is never written and reads 8.  Otherwise one fixed buffer, where the post-step parks a finished lane on 8
    log = torch.full((bound, N, A), 8, dtype=torch.int8, device=dev) if return_actions else None
    act8 = None if return_actions else torch.full((N, A), 8, dtype=torch.int8, device=dev)
    it = 0
    if fused:
        lib = _lib.load()
        x = obs.clone()
        stat.standardize(obs[..., 0], out=x[..., 0])
        active = torch.ones(N, dtype=torch.uint8, device=dev)
        again = torch.zeros(N, dtype=torch.uint8, device=dev)
        finished = torch.zeros(1, dtype=torch.int32, device=dev)
        p = lambda t: t.data_ptr()
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        state = _lib.RsRnnTeamEvalState(N, A, Rl, L, p(vec.obs), p(vec.reward), p(vec.done), p(obs), p(x), p(stat.count), p(stat.mean),
                                        p(stat.sq), p(stat.std), p(active), p(again), p(run), p(steps), p(ret), p(rec_len), p(rec_ret),
                                        p(rec_suc), p(bank.calls), None if return_actions else p(act8), p(finished))
        default = all(ac.fused_policy for ac in acs)
        wts = [agents[a].policy_weights() for a in range(A)]      # kept alive for the run: the kernel reads them by address
        wp = (C.c_void_p * A)(*[p(w) for w in wts])
        while it < bound:
            if it and it % 16 == 0 and int(finished.item()) == N: # one host read per 16 lock-steps
                break
            a8 = log[it] if return_actions else act8
            vec.action_uniforms(u)
            loc = bank.predict_kernel(x, mask8=active)            # every owner in one launch; the draw counters are the post-step's
            if default:
                _lib.check(lib.rs_rnn_team_eval_step(wp, A, p(x), p(loc), p(hid), p(u), p(active), p(a8), N, st), "rs_rnn_team_eval_step")
            else:                                                 # the same round at the other widths: no value, no log-probability
                _lib.check(lib.rs_rnn_sized_team_step(wp, A, acs[0].hid, acs[0].pol[0], acs[0].val[0], p(x), p(loc), p(hid), p(u), None, None,
                                                      p(a8), p(active), N, st), "rs_rnn_sized_team_step")
            vec.step(a8)
            _lib.check(lib.rs_rnn_team_eval_post_step(C.byref(state), st), "rs_rnn_team_eval_post_step")
            if Rl > 1:                                            # :455-466: the lanes that begin their next run
                vec.refresh(*saved, mask=again)
                _lib.check(lib.rs_rnn_team_eval_post_refresh(C.byref(state), st), "rs_rnn_team_eval_post_refresh")
            it += 1
    else:
        lane = torch.arange(N, device=dev)
        k_act = torch.zeros(A, N, dtype=torch.int64, device=dev)
        val = torch.empty(N, dtype=torch.float32, device=dev)     # policy_step_rows always writes the value; it is dropped
        while it < bound:
            active = run < Rl
            if it and it % 16 == 0 and not bool(active.any()):    # the fused form's stopping rule
                break
            a8 = log[it] if return_actions else act8
            x = obs.clone()
            stat.standardize(obs[..., 0], out=x[..., 0])
            vec.action_uniforms(u)
            loc = bank.predict(x, mask=active)
            active8 = active.to(torch.uint8)
            for a in range(A):
                if pol_kernel:
                    agents[a].policy_step_rows(x, loc, hid[a], u, a, val, act=k_act[a], mask8=active8)
                else:
                    logits, _, h1 = acs[a].policy_step(x[:, a], loc[:, a], hid[a])
                    hid[a] = torch.where(active.view(N, 1), h1, hid[a])
                    cdf = torch.cumsum(torch.softmax(logits, dim=-1), dim=-1)
                    k_act[a] = (cdf[:, :-1] <= u[:, a].unsqueeze(-1)).sum(dim=-1)
            a8.copy_(torch.where(active.view(N, 1), k_act.t(), torch.full_like(k_act.t(), 8)).to(torch.int8))   # lanes without a run idle
            obs_n, rew, _, done, _ = vec.step(a8)
            ret += torch.where(active, rew[:, 0], torch.zeros_like(rew[:, 0]))       # `episode_return[0]`
            steps += active.int()
            found = done.bool().any(dim=1) & active
            over = found | ((steps == L) & active)
            stat.update(obs_n[..., 0], mask=active)                                  # :395-397 (before the episode-over test)
            slot = run.long().clamp(max=Rl - 1)
            rec_len[lane, slot] = torch.where(over, steps, rec_len[lane, slot])
            rec_ret[lane, slot] = torch.where(over, ret, rec_ret[lane, slot])
            rec_suc[lane, slot] = torch.where(over, found.to(torch.uint8), rec_suc[lane, slot])
            run += over.int()
            again = over & (run < Rl)                                                # :455-466: refresh, statistics restart
            if Rl > 1:
                obs_r = vec.refresh(*saved, mask=again.to(torch.uint8))[0]
                stat.reset(again)
                stat.update(obs_r[..., 0], mask=again)
                obs = torch.where(again.view(N, 1, 1), obs_r, obs_n).clone()
            else:
                obs = obs_n.clone()
            steps.masked_fill_(over, 0)
            ret.masked_fill_(over, 0.0)
            it += 1
    # lanes whose runs are over idle on purpose; stacked agents may "stall".  One agent's idle step is a move by (0, 0): it never stalls
    return _close(vec, keys, saved, R, rec_len.reshape(-1), rec_ret.reshape(-1), rec_suc.reshape(-1).bool(),
                  log=log[:it] if return_actions else None, ignore_flags=_lib.RS_ENVERR_IDLE_STALL if A > 1 else 0)


# ---------------------------------------------------------------------------------------------------------------------
# RAD-TEAM (CNN) policies, result summaries and the evaluate_PPO driver
@torch.no_grad()
def run_test_environments_cnn(agents: Dict[int, Any], env_sets: Dict[str, tuple], montecarlo_runs: int = 100,
                              steps_per_episode: int = 120, team_mode: str = "individual", obstruction_count: int = 0,
                              enforce_grid_boundaries: bool = True, seed: int = 0, device: str = "cuda:0",
                              use_predictor: bool = True, return_actions: bool = False):
    """EpisodeRunner.run (evaluate.py:333-476) for the 'cnn' architecture: every (saved environment, Monte-Carlo run) pair is one
    env; per step the heat maps are updated from all agents' observations (with every owner's PFGRU prediction in channel 0),
    each CNN actor samples its action (`ac.step(observations, hiddens)`, :383), the env steps, and an episode ends when any
    agent's terminal flag is raised or at `steps_per_episode`; the maps restart with each episode (`agent.reset()`, :471-473).
    team_mode "individual": agent 0's own reward is accumulated (`episode_return[0]`, :400-447), otherwise the team reward.
    agents: {id: CNNAgentPPO}.  Returns (List[MonteCarloResults], summary)."""
    from .maps import HeatMaps
    from .pfgru import PredictorBank
    A = len(agents)
    R, L = montecarlo_runs, steps_per_episode
    N = len(env_sets) * R
    dev = torch.device(device)
    vec, keys, saved, obs, _ = _open(env_sets, R, A, obstruction_count, enforce_grid_boundaries, seed, device, welford=False)
    maps = HeatMaps(vec, L, enforce_boundaries=bool(enforce_grid_boundaries))
    bank = None
    if use_predictor:
        bank = PredictorBank(N, A, seed=seed, device=dev)
        for a, ag in agents.items():
            if getattr(ag, "model", None) is not None:                # the agent's own (saved) predictor weights
                bank.load_state_dict(a, ag.model.state_dict())
        bank.reset()
    alive, ep_len, ep_ret, success = _lane_records(N, dev)
    u = torch.empty(N, A, dtype=torch.float32, device=dev)
    act8 = torch.empty(N, A, dtype=torch.int8, device=dev)
    log = []
    for _ in range(L):
        pred = bank.predict(obs) if bank is not None else None
        maps.update(obs, pred=pred)
        shared, cells, pcells = maps.shared_maps(), maps.field("cell").long(), maps.field("pred_cell").long()
        vec.action_uniforms(u)
        for a, ag in agents.items():
            act, _ = ag.act((shared, cells, pcells, a), u[:, a])
            act8[:, a] = torch.where(alive, act, torch.full_like(act, 8)).to(torch.int8)       # finished episodes idle in place
        if return_actions:
            log.append(act8.clone())
        obs_n, rew, team, done, _ = vec.step(act8)
        _book_step(alive, ep_len, ep_ret, success, rew[:, 0] if team_mode == "individual" else team, done.bool().any(dim=1))
        obs = obs_n.clone()
        if not bool(alive.any()):
            break
    # finished episodes idle on purpose; stacked agents may "stall"
    return _close(vec, keys, saved, R, ep_len, ep_ret, success, log=torch.stack(log) if return_actions else None,
                  ignore_flags=_lib.RS_ENVERR_IDLE_STALL)


@torch.no_grad()
def _run_lane_per_run_team(rounds, agents, env_sets, montecarlo_runs, steps_per_episode, team_mode, obstruction_count,
                           enforce_grid_boundaries, seed, device, return_actions, fused, welford, id_hint="", cuda_front="", setup=None,
                           **vec_kwargs):
    """The loop under run_test_environments_team, run_test_environments_cnn_team, run_test_environments_cnn_team_sized and
    run_test_environments_gradient_search (whose `agents` are placeholders: it has no networks): E * R lanes
    of one episode each; a lane ends when any agent's terminal flag rises or at steps_per_episode and then idles (rows of 8), its
    records frozen.  Ids other than 0..A-1 (id_hint ends that message) and, for the front named in cuda_front, a device that is not
    cuda are refused before the library is loaded or an environment is built.  setup(run), where given, runs right after the opening
    and returns what the architecture keeps for the run; rounds(run, fused, *that) -- run.obs [N, A, 11] holds the current observation
    throughout, run.stat is None without welford, run.alive8 is run.alive as bytes --, called once, returns (before, policy_round):
    before(), or None, is the same in both forms; policy_round(a8) writes every lane's action row into a8 [N, A] int8, 8 on finished
    lanes -- by the kernel's own rule in the fused form, by the torch idle rule in the composed one.
    A lock-step is rs_action_uniforms, before(), policy_round(a8), rs_step and then, fused, rs_eval_post_step (returns, lengths, the
    terminal rule, the Welford update where there are statistics, the new observation, the finished-lane count) on the same stream;
    composed, the same in torch.  The host reads the finished-lane count at every 16th lock-step and nowhere else."""
    A = len(agents)
    if sorted(agents) != list(range(A)) or not 1 <= A <= _lib.RS_MAX_AGENTS:
        raise ValueError(f"agents must carry the ids 0..A-1 with A in 1..{_lib.RS_MAX_AGENTS}{id_hint}")
    dev = torch.device(device)
    if cuda_front and dev.type != "cuda":
        raise ValueError(f"{cuda_front} needs a cuda device; run_test_environments_cnn runs elsewhere")
    R, L, N = montecarlo_runs, steps_per_episode, len(env_sets) * montecarlo_runs
    lib = _lib.load()
    vec, keys, saved, obs, stat = _open(env_sets, R, A, obstruction_count, enforce_grid_boundaries, seed, device, welford=welford, **vec_kwargs)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    run = SimpleNamespace(lib=lib, vec=vec, obs=obs, stat=stat, N=N, A=A, L=L, seed=seed, dev=dev, st=st)
    own = setup(run) if setup else ()                             # before the records: device memory is laid out as it always was
    alive, ep_len, ep_ret, success = _lane_records(N, dev)
    u = torch.empty(N, A, dtype=torch.float32, device=dev)
    # with return_actions the action rows of lock-step t are written straight into row t of the log, which rs_step then reads
    log = torch.full((L, N, A), 8, dtype=torch.int8, device=dev) if return_actions else None
    act8 = None if return_actions else torch.empty(N, A, dtype=torch.int8, device=dev)
    use_team, p = team_mode != "individual", lambda t: t.data_ptr()
    run.u, run.alive, run.alive8 = u, alive, alive.view(torch.uint8)
    before, policy_round = rounds(run, fused, *own)
    if fused:
        finished = torch.zeros(1, dtype=torch.int32, device=dev)
        w = [None] * 4 if stat is None else [p(t) for t in (stat.count, stat.mean, stat.sq, stat.std)]
        state = _lib.RsEvalState(N, A, 1 if use_team else 0, p(vec.obs), p(vec.reward), p(vec.team), p(vec.done), p(obs), *w,
                                 p(run.alive8), p(success.view(torch.uint8)), p(ep_len), p(ep_ret), p(finished))
        post_step, state_ref = lib.rs_eval_post_step, C.byref(state)      # once, not per lock-step: it pays for the policy round's call
    it = 0
    while it < L:
        if it and it % 16 == 0:                                   # one host read per 16 lock-steps
            if (int(finished.item()) if fused else N - int(alive.sum().item())) == N:
                break
        a8 = log[it] if return_actions else act8
        vec.action_uniforms(u)
        if before is not None:
            before()
        policy_round(a8)
        if fused:
            vec.step(a8)
            _lib.check(post_step(state_ref, st), "rs_eval_post_step")
        else:
            obs_n, rew, team, done, _ = vec.step(a8)
            _book_step(alive, ep_len, ep_ret, success, team if use_team else rew[:, 0], done.bool().any(dim=1))
            if stat is not None:
                stat.update(obs_n[..., 0], mask=alive)            # after _book_step: the lanes that have just finished are out
            obs.copy_(obs_n)
        it += 1
    # finished episodes idle on purpose; stacked agents may "stall"
    return _close(vec, keys, saved, R, ep_len, ep_ret, success, log=log[:it] if return_actions else None,
                  ignore_flags=_lib.RS_ENVERR_IDLE_STALL)


def _ff_rounds(run, fused, agents):
    """The feed-forward policy round.  fused: rs_ff_eval_step (standardisation, every agent's actor, the draw, idle rows).  composed:
    DeviceWelford.standardize, rs_ff_team_step's step round (value and log-probability dropped) and the idle rule."""
    lib, obs, stat, N, A, u, alive, alive8, st = run.lib, run.obs, run.stat, run.N, run.A, run.u, run.alive, run.alive8, run.st
    p = lambda t: t.data_ptr()
    arr = _lib.RsMlpParams * A
    pa = arr(*[mlp_params(agents[a].agent.actor) for a in range(A)])
    if fused:
        step, fixed = lib.rs_ff_eval_step, (A, p(obs), p(stat.mean), p(stat.std), p(u), p(alive8))     # buffers that stay where they are

        def policy_round(a8):
            _lib.check(step(pa, *fixed, p(a8), N, st), "rs_ff_eval_step")
    else:
        pc = arr(*[mlp_params(agents[a].agent.critic) for a in range(A)])
        x = torch.empty_like(obs)
        k_act = torch.empty(A, N, dtype=torch.int64, device=run.dev)
        k_f = torch.empty(A, 3, N, dtype=torch.float32, device=run.dev)

        def policy_round(a8):
            x.copy_(obs)
            stat.standardize(obs[..., 0], out=x[..., 0])
            _lib.check(lib.rs_ff_team_step(pa, pc, A, p(x), p(u), p(k_act), p(k_f), None, None, N, st), "rs_ff_team_step")
            a8.copy_(torch.where(alive.view(N, 1), k_act.t(), torch.full_like(k_act.t(), 8)).to(torch.int8))   # finished episodes idle
    return None, policy_round


def _cnn_team_setup(run, front, agents, use_predictor, refuse_sides):
    """What the two RAD-TEAM rounds share, for the runner `front`: the HeatMaps -- refuse_sides(map dimensions) raises the front's own
    message about sides it does not serve --, the HIP PredictorBank with the agents' saved predictor weights, the views of the maps'
    cell fields, the actors, and the step before either round: the PFGRU step of every owner with the bank's call counter,
    rs_maps_update, rs_maps_stack.  Returns (shared, cells, pcells, actors, before); shared [N, 4, X, Y] is what rs_maps_stack fills."""
    from .maps import HeatMaps
    from .pfgru import PredictorBank
    obs, N, A = run.obs, run.N, run.A
    maps = HeatMaps(run.vec, run.L, enforce_boundaries=bool(run.vec.cfg.enforce_grid_boundaries))
    refuse_sides(tuple(maps.map_dimensions))
    bank = None
    if use_predictor:
        bank = PredictorBank(N, A, seed=run.seed, device=run.dev)
        if bank.impl != "hip":
            raise ValueError(f"{front} needs PredictorBank(impl='hip'); use run_test_environments_cnn")
        for a in range(A):
            if getattr(agents[a], "model", None) is not None:         # the agent's own (saved) predictor weights
                bank.load_state_dict(a, agents[a].model.state_dict())
        bank.reset()
    cells, pcells = maps.field("cell"), maps.field("pred_cell")       # views of the heat maps' own state: [N, A] int32, -1 = none
    assert cells.dtype == torch.int32 and pcells.dtype == torch.int32 and cells.shape == (N, A) and pcells.shape == (N, A)

    def before():
        pred = None
        if bank is not None:
            pred = bank.predict_kernel(obs)                       # bank.predict without its copy of the prediction
            bank.calls.add_(1)
        maps.update(obs, pred=pred)
        maps.shared_maps()                                        # fills maps.critic_stack in place and returns it: `shared` below
    return maps.critic_stack, cells, pcells, [agents[a].pi.actor for a in range(A)], before


def _cnn_rounds(run, fused, shared, cells, pcells, actors, before):
    """The RAD-TEAM policy round on 27 x 27 maps behind _cnn_team_setup; the agents' convolution weights are re-arranged
    once.  fused: rs_cnn_team_trunk_infer and rs_cnn_team_eval_head over one a2 [A, N, 2704].  composed: per agent
    rs_cnn_trunk_infer, torch.nn.functional.linear, rs_cnn_head and the idle rule."""
    from .maps import cnn_head_params, cnn_trunk_prepare
    lib, N, A, dev, u, alive, alive8, st = run.lib, run.N, run.A, run.dev, run.u, run.alive, run.alive8, run.st
    p = lambda t: t.data_ptr()
    wt = torch.empty(A, lib.rs_cnn_trunk_scratch_floats(6), dtype=torch.float32, device=dev)     # in K9's layout, once per run
    for a, m in enumerate(actors):
        cnn_trunk_prepare(m, 6, wt[a], st)
    if fused:
        a2 = torch.empty(A, N, 2704, dtype=torch.float32, device=dev)
        heads = (_lib.RsCnnHeadParams * A)(*[cnn_head_params(m) for m in actors])

        def policy_round(a8):
            _lib.check(lib.rs_cnn_team_trunk_infer(p(shared), p(cells), p(pcells), A, N, p(wt), p(a2), st), "rs_cnn_team_trunk_infer")
            _lib.check(lib.rs_cnn_team_eval_head(heads, A, p(a2), p(u), p(alive8), p(a8), None, None, None, N, st), "rs_cnn_team_eval_head")
    else:
        a2 = torch.empty(N, 2704, dtype=torch.float32, device=dev)
        k_act = torch.empty(A, N, dtype=torch.int64, device=dev)

        def policy_round(a8):
            cl, pl = cells.long(), pcells.long()
            for a, m in enumerate(actors):
                _lib.check(lib.rs_cnn_trunk_infer(p(shared), p(cl), p(pl), A, a, N, p(wt[a]), p(a2), st), "rs_cnn_trunk_infer")
                y1 = torch.nn.functional.linear(a2, m[6].weight, m[6].bias)
                _lib.check(lib.rs_cnn_head(p(y1), p(m[8].weight), p(m[8].bias), p(m[10].weight), p(m[10].bias), 8, p(u) + 4 * a, A, p(k_act[a]),
                                           None, None, 1, None, 1, 0, None, N, st), "rs_cnn_head")
                a8[:, a] = torch.where(alive, k_act[a], torch.full_like(k_act[a], 8)).to(torch.int8)    # finished episodes idle in place
    return before, policy_round


def _cnn_sized_rounds(run, fused, a2_bytes, shared, cells, pcells, actors, before):
    """The RAD-TEAM policy round on square maps of side M behind _cnn_team_setup, chunk lanes at a time through one scratch
    a2 of at most a2_bytes (never less than 64 lanes').  fused: rs_cnn_sized_team_infer and rs_cnn_sized_team_eval_head per chunk.
    composed: per agent and chunk rs_cnn_sized_infer, torch.nn.functional.linear and rs_cnn_head, then the idle rule."""
    from .maps import cnn_conv_params, cnn_head_params
    lib, N, A, dev, u, alive, alive8, st = run.lib, run.N, run.A, run.dev, run.u, run.alive, run.alive8, run.st
    p = lambda t: t.data_ptr()
    M = shared.shape[-1]
    flat = 16 * (M // 2) ** 2
    chunk = min(max(64, int(a2_bytes) // (4 * A * flat) // 64 * 64), N)
    if fused:
        a2 = torch.empty(A * chunk * flat, dtype=torch.float32, device=dev)
        convs = (_lib.RsCnnConvParams * A)(*[cnn_conv_params(m) for m in actors])
        heads = (_lib.RsCnnHeadParams * A)(*[cnn_head_params(m) for m in actors])

        def policy_round(a8):
            for lo in range(0, N, chunk):                         # the same scratch for every chunk: one stream keeps them in order
                n = min(chunk, N - lo)
                _lib.check(lib.rs_cnn_sized_team_infer(p(shared) + 16 * M * M * lo, p(cells) + 4 * A * lo, p(pcells) + 4 * A * lo, A, n, M, convs,
                                                       p(a2), st), "rs_cnn_sized_team_infer")
                _lib.check(lib.rs_cnn_sized_team_eval_head(heads, A, flat, p(a2), p(u) + 4 * A * lo, p(alive8) + lo, p(a8) + A * lo, None, None,
                                                           None, n, st), "rs_cnn_sized_team_eval_head")
    else:
        a2 = torch.empty(chunk * flat, dtype=torch.float32, device=dev)
        k_act = torch.empty(A, N, dtype=torch.int64, device=dev)

        def policy_round(a8):
            cl, pl = cells.long(), pcells.long()
            for a, m in enumerate(actors):
                for lo in range(0, N, chunk):
                    n = min(chunk, N - lo)
                    x = a2[:n * flat].view(n, flat)
                    _lib.check(lib.rs_cnn_sized_infer(p(shared) + 16 * M * M * lo, p(cl) + 8 * A * lo, p(pl) + 8 * A * lo, A, a, n, M, p(m[0].weight),
                                                      p(m[0].bias), p(m[3].weight), p(m[3].bias), p(x), st), "rs_cnn_sized_infer")
                    y1 = torch.nn.functional.linear(x, m[6].weight, m[6].bias)
                    _lib.check(lib.rs_cnn_head(p(y1), p(m[8].weight), p(m[8].bias), p(m[10].weight), p(m[10].bias), 8, p(u) + 4 * (A * lo + a), A,
                                               p(k_act[a]) + 8 * lo, None, None, 1, None, 1, 0, None, n, st), "rs_cnn_head")
                a8[:, a] = torch.where(alive, k_act[a], torch.full_like(k_act[a], 8)).to(torch.int8)    # finished episodes idle in place
    return before, policy_round


def run_test_environments_cnn_team(agents: Dict[int, Any], env_sets: Dict[str, tuple], montecarlo_runs: int = 100,
                                   steps_per_episode: int = 120, team_mode: str = "individual", obstruction_count: int = 0,
                                   enforce_grid_boundaries: bool = True, seed: int = 0, device: str = "cuda:0",
                                   use_predictor: bool = True, return_actions: bool = False, fused: bool = True):
    """run_test_environments_cnn for RAD-TEAM teams of 1..8 agents on 27 x 27 maps (enforce_grid_boundaries=True, the size every CLI of
    the reference trains with) with its lock-step in HIP: the same arguments, the same records.  agents: {id: CNNAgentPPO}, ids 0..A-1.
    It needs a cuda device and the HIP predictor bank; another map side, another device or other ids raise ValueError -- those
    configurations stay with run_test_environments_cnn.

    fused=True: a lock-step is rs_action_uniforms, the PFGRU step of every owner (and the bank's call counter), rs_maps_update,
    rs_maps_stack, rs_cnn_team_trunk_infer (every agent's actor trunk, straight from the heat maps' int32 cell fields),
    rs_cnn_team_eval_head (Linear(2704, 32) on the matrix cores, heads, draw, idle rows for finished lanes), rs_step and
    rs_eval_post_step -- nothing per agent, on one stream; the agents' convolution weights are re-arranged once before the loop and the
    host reads the finished-lane count once every 16 lock-steps.  The trunk's output travels through ONE scratch tensor a2 [A, N, 2704],
    allocated once: A * N * 10 816 bytes, about 8.7 GB at 100 000 lanes and 8 agents.
    fused=False: the same loop and stopping rule composed from what the collector uses -- per agent rs_cnn_trunk_infer,
    torch.nn.functional.linear, rs_cnn_head and the idle rule, shared torch bookkeeping and the observation copy: the A/B baseline.

    Returns (List[MonteCarloResults], summary); with return_actions also the [lock-steps run, N, A] int8 log of rs_step's action rows
    (8 where a lane had finished)."""
    front = "run_test_environments_cnn_team"

    def refuse_sides(dims):
        if dims != (27, 27) or any(tuple(ag.map_dim) != (27, 27) for ag in agents.values()):
            raise ValueError(f"{front} serves 27 x 27 heat maps, this configuration has {dims}; use run_test_environments_cnn")
    return _run_lane_per_run_team(
        _cnn_rounds, agents, env_sets, montecarlo_runs, steps_per_episode, team_mode, obstruction_count, enforce_grid_boundaries, seed,
        device, return_actions, fused, welford=False, id_hint="; run_test_environments_cnn takes any ids", cuda_front=front,
        setup=lambda run: _cnn_team_setup(run, front, agents, use_predictor, refuse_sides))


def run_test_environments_cnn_team_sized(agents: Dict[int, Any], env_sets: Dict[str, tuple], montecarlo_runs: int = 100,
                                         steps_per_episode: int = 120, team_mode: str = "individual", obstruction_count: int = 0,
                                         enforce_grid_boundaries: bool = True, seed: int = 0, device: str = "cuda:0",
                                         use_predictor: bool = True, return_actions: bool = False, fused: bool = True,
                                         a2_bytes: int = 4 << 30):
    """run_test_environments_cnn_team for square heat maps of any side 8..256 that every agent was built for (agent.map_dim): the maps
    without enforced walls are 27 + steps_per_episode cells a side, 147 x 147 for 120-step episodes.  The same arguments, the same
    records; ids 0..A-1, a cuda device and the HIP predictor bank, anything else raises ValueError -- those configurations stay with
    run_test_environments_cnn.

    fused=True: a lock-step is rs_action_uniforms, the PFGRU step of every owner, rs_maps_update, rs_maps_stack, then per chunk of lanes
    rs_cnn_sized_team_infer (every agent's trunk from the heat maps' int32 cell fields; conv1 is not evaluated over empty input
    windows) and rs_cnn_sized_team_eval_head (Linear(16 P P, 32) on the matrix cores, heads, draw, idle rows), then rs_step and
    rs_eval_post_step, on one stream; the host reads the finished-lane count once every 16 lock-steps.  The trunk's output is 16 P P
    floats per lane and agent (341 KB at 147), so it travels through ONE scratch tensor of at most a2_bytes (never less than 64 lanes'):
    chunk = max(64, a2_bytes // (4 A 16 P P) // 64 * 64) lanes at a time.  The head's bits depend on neither the lane count nor the
    grid, so the records do not depend on a2_bytes.
    fused=False: the same loop and stopping rule composed per agent from rs_cnn_sized_infer, torch.nn.functional.linear, rs_cnn_head
    and the idle rule with the torch bookkeeping (the A/B baseline), chunked in the same way.

    Returns (List[MonteCarloResults], summary); with return_actions also the [lock-steps run, N, A] int8 log of rs_step's action rows
    (8 where a lane had finished)."""
    front = "run_test_environments_cnn_team_sized"

    def refuse_sides(dims):
        X, Y = dims
        if X != Y or not 8 <= X <= 256 or any(tuple(ag.map_dim) != (X, Y) for ag in agents.values()):
            raise ValueError(f"{front} serves square heat maps of side 8..256 that every agent was built for; this configuration has "
                             f"{(X, Y)} maps and agents for {[tuple(agents[a].map_dim) for a in range(len(agents))]}; "
                             "use run_test_environments_cnn")
    return _run_lane_per_run_team(
        lambda run, f, *cnn: _cnn_sized_rounds(run, f, a2_bytes, *cnn), agents, env_sets, montecarlo_runs, steps_per_episode, team_mode,
        obstruction_count, enforce_grid_boundaries, seed, device, return_actions, fused, welford=False,
        id_hint="; run_test_environments_cnn takes any ids", cuda_front=front,
        setup=lambda run: _cnn_team_setup(run, front, agents, use_predictor, refuse_sides))


def run_test_environments_team(agents: Dict[int, VecAgentPPO], env_sets: Dict[str, tuple], montecarlo_runs: int = 100,
                               steps_per_episode: int = 120, team_mode: str = "individual", obstruction_count: int = 0,
                               enforce_grid_boundaries: bool = True, seed: int = 0, device: str = "cuda:0", return_actions: bool = False,
                               falloff: str = "reference", fused: bool = True):
    """EpisodeRunner.run (evaluate.py:355-475) for feed-forward agents and teams of 1..8: every agent has its own network and its own
    statistics buffer, an episode ends when any agent's terminal flag is raised or at `steps_per_episode`.  One lane per (saved
    environment, Monte-Carlo run), as run_test_environments does for 'ff' -- exact, because a feed-forward policy has no hidden state
    and the statistics buffer restarts with every run.  team_mode "individual": agent 0's own reward is accumulated, otherwise the
    team reward.  agents: {id: VecAgentPPO}, ids 0..A-1.

    fused=True: a lock-step is four launches on one stream -- rs_action_uniforms, rs_ff_eval_step (standardisation, every agent's
    actor, the draw, idle rows for finished lanes), rs_step, rs_eval_post_step (returns, lengths, terminal rule, Welford update, new
    observation, finished-lane count) -- and the host reads the finished-lane count once every 16 lock-steps; nothing else
    synchronises.  fused=False: the same lock-step composed from DeviceWelford, rs_ff_team_step's step round (value and
    log-probability dropped) and torch bookkeeping, with the same stopping rule: the A/B baseline, identical results.

    Returns (List[MonteCarloResults], summary); with return_actions also the [lock-steps run, N, A] int8 log of rs_step's action rows
    (8 where a lane had finished)."""
    return _run_lane_per_run_team(lambda run, f: _ff_rounds(run, f, agents), agents, env_sets, montecarlo_runs, steps_per_episode,
                                  team_mode, obstruction_count, enforce_grid_boundaries, seed, device, return_actions, fused, welford=True,
                                  falloff=falloff)


def _gs_rounds(run, fused, q):
    """The gradient-search policy round (GradSearch.step, algos/test_environment/eval/core.py:636-653).  fused: rs_gs_eval_step (the
    look-ahead over 8 moves, the gradient, the draw, idle rows).  composed: rs_peek, then in torch the gradient in float64 rounded
    once to float32, log-softmax, cumsum, compare and the idle rule."""
    lib, vec, obs, N, u, alive, alive8, st = run.lib, run.vec, run.obs, run.N, run.u, run.alive, run.alive8, run.st
    p = lambda t: t.data_ptr()
    q_rec = 1 / q                                                 # core.py:624
    if fused:
        step, fixed = lib.rs_gs_eval_step, (vec._h, p(obs), q_rec, p(u), p(alive8))

        def policy_round(a8):
            _lib.check(step(*fixed, p(a8), None, st), "rs_gs_eval_step")
    else:
        def policy_round(a8):
            _, moved, _, meas = vec.peek(lam=False)
            g = ((meas.double() - obs[..., 0:1].double()) * 0.01 * q_rec).float()
            g = torch.where(moved.bool(), g, torch.zeros_like(g))
            cdf = torch.cumsum(torch.exp(torch.log_softmax(g, dim=-1)), dim=-1)
            act = (cdf[..., :-1] <= u.unsqueeze(-1)).sum(dim=-1)
            a8.copy_(torch.where(alive.view(N, 1), act, torch.full_like(act, 8)).to(torch.int8))      # finished episodes idle
    return None, policy_round


def run_test_environments_gradient_search(env_sets: Dict[str, tuple], number_of_agents: int = 1, q: float = 1.0, montecarlo_runs: int = 100,
                                          steps_per_episode: int = 120, team_mode: str = "individual", obstruction_count: int = 0,
                                          enforce_grid_boundaries: bool = True, seed: int = 0, device: str = "cuda:0",
                                          return_actions: bool = False, falloff: str = "reference", fused: bool = True):
    """The reference's gradient-search controller ('gs' in algos/test_environment/eval/test_policy.py:73-108; GradSearch,
    eval/core.py:622-653) on saved test environments: the non-learned baseline the learned policies' success rates are reported
    against.  At every step every agent looks ahead over the 8 moves, takes a measurement at each candidate position,
    grad[k] = (meas_k - meas_now) * 0.01 / q (0 where the move is blocked by a wall or an obstruction) and samples its action from
    softmax(grad).  q = 1e30 makes every gradient vanish (below 1e-24, so softmax(grad) is 1/8 eight times in float32) -- a uniform
    random walk over the 8 moves, the second baseline this runner gives.
    Teams of 1..8: every agent searches on its own (nothing is shared) and rs_step applies the real collision rule; an episode ends
    when any agent's terminal flag rises or at steps_per_episode.  One lane per (saved environment, Monte-Carlo run); no statistics
    buffer -- the controller reads raw counts.  team_mode "individual": agent 0's own reward is accumulated, otherwise the team reward.

    fused=True: a lock-step is rs_action_uniforms, rs_gs_eval_step (look-ahead, gradient, draw, idle rows: one launch for every agent
    of every lane), rs_step, rs_eval_post_step on one stream; the host reads the finished-lane count once every 16 lock-steps.
    fused=False: the same lock-step composed from rs_peek and torch (gradient, log-softmax, cumsum, compare, idle rule) with the torch
    bookkeeping: the A/B baseline.

    "Blocked" is the look-ahead's own `moved` flag where the reference compares observation coordinates (core.py:641); the two agree
    except under coord_noise.  Returns (List[MonteCarloResults], summary); with return_actions also the [lock-steps run, N, A] int8 log
    of rs_step's action rows (8 where a lane had finished)."""
    if not q > 0:
        raise ValueError("q must be positive")
    return _run_lane_per_run_team(lambda run, f: _gs_rounds(run, f, float(q)), {i: None for i in range(int(number_of_agents))}, env_sets,
                                  montecarlo_runs, steps_per_episode, team_mode, obstruction_count, enforce_grid_boundaries, seed, device,
                                  return_actions, fused, welford=False, falloff=falloff)


def _filter_before(run, bpf, fused, rec):
    """before() of the two particle-filter runners, and the pass's records in the dict `rec` (on entry: the flags "estimates" and
    "fisher").  before() is ParticleFilter.track on the current reading -- the first call of a run draws the prior and sets the latch
    --; with "fisher" one Fisher-matrix launch into row it of rec["fim"] [L, N, A, 3, 3] (nan where a lane had finished): the initial
    bound from the prior's particles at lock-step 0, the matrix at the agent's position afterwards (test_policy.py:403, 434); with
    "estimates" the squared distance of agent 0's estimate from the source is added to the lane's sum.  rec["it"] counts the calls."""
    obs, alive, alive8 = run.obs, run.alive, run.alive8
    track, fim = (bpf.track, bpf.fim) if fused else (bpf.track_composed, bpf.fim_composed)
    f64 = dict(dtype=torch.float64, device=run.dev)
    rec["it"] = 0
    if rec.get("estimates"):
        src = torch.stack([run.vec.state("src_x").view(-1), run.vec.state("src_y").view(-1)], dim=-1).double()
        rec.update(sq=torch.zeros(run.N, **f64), n=torch.zeros(run.N, **f64), last=torch.zeros(run.N, **f64))
    if rec.get("fisher"):
        rec["fim"] = torch.full((run.L, run.N, run.A, 3, 3), float("nan"), **f64)

    def before():
        it = rec["it"]
        track(obs, alive8, it == 0)
        rec["it"] = it + 1
        if rec.get("fisher"):
            fim(alive8, prior=it == 0, F=rec["fim"][it])
        if rec.get("estimates"):
            d2 = ((bpf.estimate[:, 0, 1:] - src) ** 2).sum(dim=-1)
            rec["sq"] += torch.where(alive, d2, torch.zeros_like(d2))
            rec["n"] += alive.double()
            rec["last"].copy_(torch.where(alive, d2.sqrt(), rec["last"]))
    return before


def _rid_fim_rounds(run, fused, bpf_kwargs, rec):
    """The RID-FIM lock-step's two rounds over one BootstrapParticleFilter per (lane, agent) (radiation_ppo_amd/bpf.py).  before():
    _filter_before.  policy_round: FIC.optim_action.  fused: rs_bpf_track and rs_ridfim_eval_step; composed: rs_bpf_draws, rs_peek and
    float64 torch ops."""
    from .bpf import BootstrapParticleFilter
    bpf = BootstrapParticleFilter(run.vec, **bpf_kwargs)
    obs, alive8 = run.obs, run.alive8
    act = bpf.act if fused else bpf.act_composed

    def policy_round(a8):
        act(obs, alive8, a8)
    run.bpf = bpf
    return _filter_before(run, bpf, fused, rec), policy_round


# the controller's own table of moves (algos/test_environment/eval/test_policy.py:18-27), which sim_step (:241) adds to the detector's
# position: not the env's step -- the diagonals are 71 cm here --, and no blocking test
BPF_A2C_ACTION = ((-100.0, 0.0), (-71.0, 71.0), (0.0, 100.0), (71.0, 71.0), (100.0, 0.0), (71.0, -71.0), (0.0, -100.0), (-71.0, -71.0))


def _bpf_a2c_rounds(run, fused, agents, bpf_kwargs, rec, env_id_base):
    """The BPF-A2C lock-step's two rounds (test_policy.py:109-156): before() is _filter_before; policy_round feeds every agent's
    recurrent actor its standardised, clipped observation and the filter's location estimate over the search area's side, draws the
    action, and takes the step's score J_tot: the trace of the particles' Fisher matrix at the detector's position after that move by
    the controller's own table (row it of rec["scores"] [L, N, A] where the caller keeps them).
    fused: rs_bpf_a2c_eval_step, then rs_bpf_fim.  composed: the standardisation, the clip and the scaling in torch, rs_rnn_team_eval_step
    (rs_rnn_sized_team_step at other widths than the default), the torch idle rule, the table in torch and fim_composed.
    GRU states: what recurrent_team_start draws, from the lanes' own keys (env_id_base + lane), fresh for every run; no PFGRU bank."""
    from .bpf import BootstrapParticleFilter
    from .pfgru import lane_base
    lib, vec, obs, stat, N, A, u, alive, alive8, st, dev = run.lib, run.vec, run.obs, run.stat, run.N, run.A, run.u, run.alive, run.alive8, run.st, run.dev
    p = lambda t: t.data_ptr()
    bpf = BootstrapParticleFilter(vec, **bpf_kwargs)
    acs = [agents[a].agent for a in range(A)]
    hid = _gru_team_h0(agents, lane_base(N, A, run.seed, env_id_base, dev), dev)
    wts = [agents[a].policy_weights() for a in range(A)]          # kept alive for the run: the kernels read them by address
    wp = (C.c_void_p * A)(*[p(w) for w in wts])
    area_max = float(vec.cfg.bbox[3] - vec.cfg.observation_area[1])               # search_area[2][1] (test_policy.py:392)
    f64 = dict(dtype=torch.float64, device=dev)
    sim_pos, F = torch.zeros(N, A, 2, **f64), torch.zeros(N, A, 3, 3, **f64)
    if rec.get("want_scores"):
        rec["scores"] = torch.full((run.L, N, A), float("nan"), **f64)
    score = torch.zeros(N, A, **f64)
    row = lambda: rec["scores"][rec["it"] - 1] if "scores" in rec else score      # before() has counted this lock-step already
    if fused:
        def policy_round(a8):
            _lib.check(lib.rs_bpf_a2c_eval_step(vec._h, wp, A, p(obs), p(stat.mean), p(stat.std), p(bpf.estimate), area_max, p(hid), p(u),
                                                p(alive8), p(a8), p(sim_pos), None, None, st), "rs_bpf_a2c_eval_step")
            bpf.fim(alive8, pos=sim_pos, F=F, trace=row())
    else:
        default = all(ac.fused_policy for ac in acs)
        x, loc = torch.empty_like(obs), torch.empty(N, A, 2, dtype=torch.float32, device=dev)
        k8 = torch.full((N, A), 8, dtype=torch.int8, device=dev)
        table = torch.tensor(BPF_A2C_ACTION, **f64)

        def policy_round(a8):
            x.copy_(obs)
            x[..., 0] = ((obs[..., 0].double() - stat.mean) / stat.std).float().clamp(-8.0, 8.0)     # test_policy.py:400, 422
            loc.copy_((bpf.estimate[..., 1:] / area_max).float())
            if default:
                _lib.check(lib.rs_rnn_team_eval_step(wp, A, p(x), p(loc), p(hid), p(u), p(alive8), p(k8), N, st), "rs_rnn_team_eval_step")
            else:
                _lib.check(lib.rs_rnn_sized_team_step(wp, A, acs[0].hid, acs[0].pol[0], acs[0].val[0], p(x), p(loc), p(hid), p(u), None, None,
                                                      p(k8), p(alive8), N, st), "rs_rnn_sized_team_step")
            a8.copy_(torch.where(alive.view(N, 1), k8, torch.full_like(k8, 8)))                      # finished episodes idle
            pos = torch.stack([vec.state("x").t(), vec.state("y").t()], dim=-1).double()
            sim_pos.copy_(torch.where(alive.view(N, 1, 1), pos + table[a8.long().clamp(0, 7)], sim_pos))
            bpf.fim_composed(alive8, pos=sim_pos, F=F, trace=row())
    run.bpf, run.hid, run.sim_pos = bpf, hid, sim_pos
    return _filter_before(run, bpf, fused, rec), policy_round


def _filter_passes(rounds, agents, who, env_sets, montecarlo_runs, steps_per_episode, team_mode, obstruction_count, enforce_grid_boundaries,
                   seed, device, return_actions, falloff, fused, welford, lanes_per_pass, return_estimates, fisher, return_scores, bpf_kwargs):
    """What the two particle-filter runners (`who`: the caller's name, for messages) share around _run_lane_per_run_team: the refusals,
    the split of the saved environments into passes of at most lanes_per_pass lanes -- whole environments; every lane keeps the Philox
    key of its place in the whole set, so the split does not change a result -- and the results put together.  rounds(run, fused, rec,
    env_id_base) returns the pass's (before, policy_round)."""
    A, R = len(agents), int(montecarlo_runs)
    if sorted(agents) != list(range(A)) or not 1 <= A <= _lib.RS_MAX_AGENTS:
        raise ValueError(f"agents must carry the ids 0..A-1 with A in 1..{_lib.RS_MAX_AGENTS}")
    if torch.device(device).type != "cuda":
        raise ValueError(f"{who} needs a cuda device")
    NP = int(bpf_kwargs.get("nParticles", 6000))
    if NP < 2:
        raise ValueError("nParticles must be at least 2")
    if lanes_per_pass is not None and lanes_per_pass < R:
        raise ValueError("lanes_per_pass must hold one environment's runs at least (montecarlo_runs lanes): a pass runs whole environments")
    from .bpf import BootstrapParticleFilter, pcrb
    if lanes_per_pass is None:
        free = torch.cuda.mem_get_info(torch.device(device))[0]
        lanes_per_pass = max(1, int(free // 3 // (BootstrapParticleFilter.bytes_per_pair(NP) * A)))
    keys = sorted(env_sets, key=lambda k: int(k.split("_")[1]))
    per = max(1, int(lanes_per_pass) // R)                        # the free-memory default may be below R: one environment is the minimum
    results, logs, extra = [], [], {}
    for e0 in range(0, len(keys), per):
        part = {f"env_{i}": env_sets[k] for i, k in enumerate(keys[e0:e0 + per])}
        rec = dict(estimates=return_estimates, fisher=fisher, want_scores=return_scores)
        out = _run_lane_per_run_team(lambda run, f: rounds(run, f, rec, e0 * R), agents, part, R, steps_per_episode, team_mode,
                                     obstruction_count, enforce_grid_boundaries, seed, device, return_actions, fused, welford=welford,
                                     falloff=falloff, env_id_base=e0 * R)
        for res, k in zip(out[0], keys[e0:e0 + per]):
            res.id = int(k.split("_")[1])
        results += out[0]
        if return_actions:
            logs.append(out[2])
        if return_estimates:
            extra.setdefault("rmse", []).append((rec["sq"] / rec["n"].clamp(min=1.0)).sqrt().cpu().numpy())
            extra.setdefault("final", []).append(rec["last"].cpu().numpy())
        if fisher:                                                # the bound's recursion, on the host, on the recorded matrices
            m = rec["fim"].cpu().numpy()
            extra.setdefault("bounds", []).append(pcrb(m[0], m[1:], bpf_kwargs.get("noise_params", (15.0, 1.0, 1.0))).transpose(1, 2, 0, 3, 4))
        if return_scores:
            extra.setdefault("scores", []).append(rec["scores"].cpu().numpy())
    ret = [results, summarize(results)]
    if return_actions:
        L = max(l.shape[0] for l in logs)
        logs = [np.concatenate([l, np.full((L - l.shape[0],) + l.shape[1:], 8, dtype=np.int8)]) for l in logs]
        ret.append(np.concatenate(logs, axis=1))
    if extra:
        ret.append({k: np.concatenate(v, axis=1 if k == "scores" else 0) for k, v in extra.items()})
    return tuple(ret)


def run_test_environments_rid_fim(env_sets: Dict[str, tuple], number_of_agents: int = 1, montecarlo_runs: int = 100, steps_per_episode: int = 120,
                                  team_mode: str = "individual", obstruction_count: int = 0, enforce_grid_boundaries: bool = True,
                                  seed: int = 0, device: str = "cuda:0", return_actions: bool = False, falloff: str = "reference",
                                  fused: bool = True, lanes_per_pass: int = None, return_estimates: bool = False, fisher: bool = False,
                                  **bpf_kwargs):
    """The reference's information-driven baseline ('rid-fim' in algos/test_environment/eval/test_policy.py:184-231; FIC and
    ParticleFilter, eval/core.py:528-620, 655-764) on saved test environments: every agent runs a bootstrap particle filter over
    (intensity, x, y) on its own readings and moves where the Renyi divergence of the predicted readings -- after the latch has
    fallen, the trace of the particles' Fisher information -- is largest.  A lock-step is rs_action_uniforms (unused: the controller
    draws no action), the filter's track on the current reading, the controller round, rs_step and the bookkeeping, on
    _run_lane_per_run_team like the gradient search: one lane per (saved environment, Monte-Carlo run), teams of 1..8 with nothing
    shared between agents, no statistics buffer.  bpf_kwargs go to BootstrapParticleFilter (nParticles, noise_params, thresh, intensity,
    coord, alpha, fim_thresh, interval; the reference's values by default).

    fused=True: rs_bpf_track and rs_ridfim_eval_step, one launch each for every agent of every lane.  fused=False: the same lock-step
    composed from rs_bpf_draws, rs_peek and float64 torch ops with the torch bookkeeping: the A/B baseline (its resampler walks the
    chain one batched torch step per particle).

    The filter's measurement model is the inverse-square law I 1e4 / R^2 + bkg (core.py:594-596), while the env's reference falloff is
    I / r (rad_search_env.py:501): under falloff="reference" -- the default, as for every runner -- the filter is mis-specified, as it is
    in the reference, and does not localise; falloff="inverse_square" is the env the filter models.

    One difference from the reference, on purpose: it rebuilds only the filter between runs (test_policy.py:230-231, 493) and lets the
    controller's latch RDIV_FLAG leak from one run into the next; here every run starts with a fresh filter AND the latch set.

    At 6000 particles a pair's state takes about 0.4 MB, so the saved environments are run in passes of at most lanes_per_pass lanes
    (whole environments, so a given lanes_per_pass below montecarlo_runs is refused; default: what a third of the free device memory holds, one environment at least) and the results are concatenated; every lane keeps
    the Philox key of its place in the whole set, so the split does not change a result.

    Returns (List[MonteCarloResults], summary); with return_actions also the [lock-steps, N, A] int8 action log (rows of 8 where a lane
    had finished; passes that stopped early are padded with 8); with return_estimates also a dict of per-lane float64 arrays:
    "rmse", the root of the mean squared distance of agent 0's estimates from the source over the lane's steps (the reference's
    LocEstErr, test_policy.py:444, without its initial prior-mean entry), and "final", the distance of the last estimate.
    fisher (the reference's --fisher, test_policy.py:361-371, 403-405, 432-436): every track is followed by one rs_bpf_fim launch -- the
    initial bound from the prior's particles at lock-step 0, the matrix at the agent's position afterwards -- and that dict (returned
    with fisher alone too) holds "bounds" [N, A, L, 3, 3] float64: the posterior Cramer-Rao bound's recursion (bpf.pcrb) on the
    recorded matrices, nan from a lane's end on.  The position is the detector's (x, y), not the reference's broadcast y (bpf.fim)."""
    A = int(number_of_agents)
    if not 1 <= A <= _lib.RS_MAX_AGENTS:
        raise ValueError(f"number_of_agents must be in 1..{_lib.RS_MAX_AGENTS}")
    return _filter_passes(lambda run, f, rec, base: _rid_fim_rounds(run, f, bpf_kwargs, rec), {i: None for i in range(A)},
                          "run_test_environments_rid_fim", env_sets, montecarlo_runs, steps_per_episode, team_mode, obstruction_count,
                          enforce_grid_boundaries, seed, device, return_actions, falloff, fused, False, lanes_per_pass, return_estimates,
                          fisher, False, bpf_kwargs)


def run_test_environments_bpf_a2c(agents: Dict[int, Any], env_sets: Dict[str, tuple], montecarlo_runs: int = 100, steps_per_episode: int = 120,
                                  team_mode: str = "individual", obstruction_count: int = 0, enforce_grid_boundaries: bool = True,
                                  seed: int = 0, device: str = "cuda:0", return_actions: bool = False, falloff: str = "reference",
                                  fused=None, lanes_per_pass: int = None, fisher: bool = False, return_scores: bool = False,
                                  return_estimates: bool = False, **bpf_kwargs):
    """The reference's 'bpf-a2c' controller (algos/test_environment/eval/test_policy.py:109-156, 573-574) on saved test environments:
    the trained recurrent actor of RAD-A2C fed the bootstrap particle filter's location estimate in place of its PFGRU's -- the one
    comparison of the RAD-A2C paper that needs both.  agents: {id: RNNAgentPPO}, ids 0..A-1 with A in 1..8, all of the same widths;
    every agent has its own network, GRU state, filter and statistics buffer, nothing is shared.  A lock-step is rs_action_uniforms,
    the filter's track on the current reading, the policy round (the reading standardised and clipped to +-8, the estimate over the
    search area's side, GRU, policy head, draw; then the step's score J_tot, the trace of the particles' Fisher matrix at the position
    the controller's own table of moves predicts), rs_step and the bookkeeping, on _run_lane_per_run_team with the running
    statistics: one lane per (saved environment, Monte-Carlo run), every run with a fresh filter and a fresh GRU state (`hidden = None`,
    test_policy.py:490) drawn as recurrent_team_start draws it; the agents' PFGRUs are not used.  bpf_kwargs go to
    BootstrapParticleFilter (the reference's values by default); the passes and lanes_per_pass are run_test_environments_rid_fim's.

    fused=True: rs_bpf_track, rs_bpf_a2c_eval_step and rs_bpf_fim, one launch each for every agent of every lane; default widths only
    (GRU 24, heads 32 / 32: the reference's ac_kwargs, :569-570), ValueError at others.  fused=False: the same lock-step composed from
    track_composed, the standardisation, clip and scaling in torch, rs_rnn_team_eval_step (rs_rnn_sized_team_step at the other
    widths), fim_composed and the torch idle rule with the torch bookkeeping: the A/B form.  fused=None: fused at the default widths.

    As for 'rid-fim', the filter's measurement model is the inverse-square law I 1e4 / R^2 + bkg (core.py:594-596), while the env's
    reference falloff is I / r: under falloff="reference" -- the default -- the filter is mis-specified, as it is in the reference, and
    the actor is fed an estimate that does not localise; falloff="inverse_square" is the env the filter models.

    Returns (List[MonteCarloResults], summary); with return_actions also the [lock-steps, N, A] int8 action log; with fisher,
    return_scores or return_estimates also a dict of float64 arrays: "bounds" [N, A, L, 3, 3] (fisher: the posterior Cramer-Rao bound,
    as run_test_environments_rid_fim returns it), "scores" [L, N, A] (J_tot of every step; nan where a lane had finished), "rmse" and
    "final" [N] (agent 0's localisation error, as for 'rid-fim')."""
    A = len(agents)
    if sorted(agents) != list(range(A)) or not 1 <= A <= _lib.RS_MAX_AGENTS:
        raise ValueError(f"agents must carry the ids 0..A-1 with A in 1..{_lib.RS_MAX_AGENTS}")
    if torch.device(device).type != "cuda":
        raise ValueError("run_test_environments_bpf_a2c needs a cuda device")
    acs = [getattr(agents[a], "agent", None) for a in range(A)]
    if not all(hasattr(ac, "gru_cell") and hasattr(agents[a], "policy_weights") for a, ac in enumerate(acs)):
        raise ValueError("run_test_environments_bpf_a2c evaluates recurrent (RAD-A2C) agents")
    if len({(ac.hid, tuple(ac.pol), tuple(ac.val)) for ac in acs}) != 1:
        raise ValueError("the agents of a team must have the same GRU and head widths: the state tensor holds one width")
    default = all(ac.fused_policy for ac in acs)
    if not default and not all(ac.sized_policy for ac in acs):
        raise ValueError("the policy kernels serve a GRU of 1..64 units with single-layer heads of 2..64 units")
    if fused is None:
        fused = default
    if fused and not default:
        raise ValueError("the fused BPF-A2C lock-step is built for the default widths (GRU 24, heads 32 / 32); fused=False composes the others")
    return _filter_passes(lambda run, f, rec, base: _bpf_a2c_rounds(run, f, agents, bpf_kwargs, rec, base), agents,
                          "run_test_environments_bpf_a2c", env_sets, montecarlo_runs, steps_per_episode, team_mode, obstruction_count,
                          enforce_grid_boundaries, seed, device, return_actions, falloff, fused, True, lanes_per_pass, return_estimates,
                          fisher, return_scores, bpf_kwargs)


def _collect_results(keys, E, R, ep_len, ep_ret, success, inten, bkg) -> List[MonteCarloResults]:
    ep_len_c, ep_ret_c, suc = ep_len.cpu().numpy(), ep_ret.cpu().numpy(), success.cpu().numpy()
    i_c, b_c = inten.cpu().numpy(), bkg.cpu().numpy()
    out: List[MonteCarloResults] = []
    for e in range(E):
        res = MonteCarloResults(id=int(keys[e].split("_")[1]))
        for r in range(R):
            n = e * R + r
            bucket = res.successful if suc[n] else res.unsuccessful
            if r < 1:                                             # evaluate.py:425-431
                bucket.intensity.append(int(i_c[n])); bucket.background_intensity.append(int(b_c[n]))
            res.total_episode_length.append(int(ep_len_c[n]))
            res.success_counter += int(suc[n])
            bucket.episode_length.append(int(ep_len_c[n])); bucket.episode_return.append(float(ep_ret_c[n]))
        res.completed_runs = R
        out.append(res)
    return out


def variance(data) -> float:             # evaluate.py:83-85
    return float(np.var(data)) if len(data) > 0 else float("nan")


def weighted_quantiles(values, weights, qs):
    """Quantiles of a weighted sample (what the reference asks statsmodels' DescrStatsW for, evaluate.py:742-760): the smallest value
    whose cumulative weight reaches q of the total."""
    v, w = np.asarray(values, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    keep = np.isfinite(v) & (w > 0)
    v, w = v[keep], w[keep]
    if v.size == 0:
        return [float("nan")] * len(qs)
    order = np.argsort(v, kind="stable")
    v, cw = v[order], np.cumsum(w[order])
    return [float(v[min(np.searchsorted(cw, q * cw[-1], side="left"), v.size - 1)]) for q in qs]


def summarize(results: List[MonteCarloResults]) -> Dict[str, Any]:
    """evaluate_PPO.parse_results / calc_stats (evaluate.py:645-880).  The reference's parse_results is unfinished -- every
    median it stores reads `scenario.successful.background_intensity` and it ends in an undefined `keys` -- so this follows the
    evident intent spelled out in calc_stats' comments: per scenario (saved environment) the success count and the median /
    variance of the returns, lengths, intensities and backgrounds of its successful and unsuccessful runs, the distribution of
    successful episode lengths (unique values ordered by count), and over all scenarios the run-weighted median and
    2.5 / 25 / 75 / 97.5 percentiles of the success count and of the successful episode length."""
    per = []
    for sc in results:
        uni, cnt = np.unique(sc.successful.episode_length, return_counts=True) if sc.successful.episode_length else (np.array([]), np.array([]))
        order = np.argsort(cnt, kind="stable")
        per.append({"id": sc.id, "runs": sc.completed_runs, "success_count": sc.success_counter,
                    "successful": {k: (float(median(getattr(sc.successful, k))), variance(getattr(sc.successful, k)))
                                   for k in ("episode_return", "episode_length", "intensity", "background_intensity")},
                    "unsuccessful": {k: (float(median(getattr(sc.unsuccessful, k))), variance(getattr(sc.unsuccessful, k)))
                                     for k in ("episode_return", "episode_length", "intensity", "background_intensity")},
                    "success_length_distribution": {"unique": [int(x) for x in uni[order]], "counts": [int(x) for x in cnt[order]]}})
    runs = np.array([p["runs"] for p in per], dtype=np.float64)
    succ = np.array([p["success_count"] for p in per], dtype=np.float64)
    med_len = np.array([p["successful"]["episode_length"][0] for p in per])
    qs = [0.025, 0.25, 0.5, 0.75, 0.975]
    done_len = [l for r in results for l in r.successful.episode_length]
    done_ret = [l for r in results for l in r.successful.episode_return]
    nd_ret = [l for r in results for l in r.unsuccessful.episode_return]
    tot_len = [l for r in results for l in r.total_episode_length]
    return {"episodes": len(results), "montecarlo_runs": int(runs[0]) if len(runs) else 0, "completed_runs": int(runs.sum()),
            "success_rate": float(succ.sum() / max(runs.sum(), 1.0)), "success_count_median": float(np.median(succ)) if len(succ) else float("nan"),
            "success_count_weighted_quantiles": dict(zip(map(str, qs), weighted_quantiles(succ, runs, qs))),
            "successful_episode_length_weighted_quantiles": dict(zip(map(str, qs), weighted_quantiles(med_len, succ, qs))),
            "successful_episode_length_median": float(median(done_len)), "successful_episode_return_median": float(median(done_ret)),
            "unsuccessful_episode_return_median": float(median(nd_ret)), "total_episode_length_median": float(median(tot_len)),
            "scenarios": per}


@dataclass
class evaluate_PPO:
    """evaluate_PPO (evaluate.py:581-643): `eval_kwargs` as the reference builds them in main.py -- test_env_path (directory of the
    saved sets), obstruction_count (0..7, not -1), snr ('none' | 'low' | 'med' | 'high'), episodes, montecarlo_runs, model_path
    (directory holding `<id>_agent*/actor.pt, critic.pt[, predictor.pt]` or `<id>_agent*/pyt_save/model.pt`),
    actor_critic_architecture ('cnn' | 'rnn' | 'ff' / 'mlp' | 'gs', the gradient-search baseline, which reads no model_path and takes
    `q`, default 1.0 | 'rid-fim', the particle-filter baseline, which reads no model_path either and takes BootstrapParticleFilter's
    parameters | 'bpf-a2c', the recurrent actor on the particle filter's estimate: agents loaded as for 'rnn', the filter's parameters as
    for 'rid-fim', and `fisher` (the posterior Cramer-Rao bounds, kept in `extras["bounds"]`)), number_of_agents, steps_per_episode,
    enforce_boundaries, team_mode, seed.
    The set is read with the safe reader (radiation_ppo_amd.testsets); all episodes x runs advance in lock-step on the device."""
    eval_kwargs: Dict[str, Any]

    def __post_init__(self) -> None:
        kw = self.eval_kwargs
        if kw["obstruction_count"] == -1:
            raise ValueError("Random sample of obstruction counts indicated. Please indicate a specific count between 1 and 7")
        self.test_env_dir = kw["test_env_path"]
        self.test_env_path = os.path.join(self.test_env_dir, f"test_env_dict_obs{kw['obstruction_count']}_{kw.get('snr', 'high')}_v4")

    def evaluate(self):
        from .testsets import load_test_environments
        kw = self.eval_kwargs
        sets = load_test_environments(self.test_env_path)
        keys = sorted(sets, key=lambda k: int(k.split("_")[1]))[:int(kw.get("episodes", 100))]
        sets = {k: sets[k] for k in keys}
        A, arch = int(kw.get("number_of_agents", 1)), kw.get("actor_critic_architecture", "cnn")
        dev = kw.get("device", "cuda:0")
        common = dict(montecarlo_runs=int(kw.get("montecarlo_runs", 100)), steps_per_episode=int(kw.get("steps_per_episode", 120)),
                      obstruction_count=int(kw["obstruction_count"]), enforce_grid_boundaries=bool(kw.get("enforce_boundaries", True)),
                      seed=int(kw.get("seed", 0) or 0), device=dev)

        def agent_dir(i):
            cands = sorted(d for d in os.listdir(kw["model_path"]) if d.startswith(f"{i}_agent"))
            if not cands:
                raise FileNotFoundError(f"no {i}_agent* directory under {kw['model_path']}")
            return os.path.join(kw["model_path"], cands[0])

        def ff_agent(i):                                                # <id>_agent*/pyt_save/model.pt, or model.pt beside it
            ag = VecAgentPPO(id=i, device=dev)
            f = os.path.join(agent_dir(i), "pyt_save", "model.pt")
            ag.load(f if os.path.exists(f) else os.path.join(agent_dir(i), "model.pt"))
            return ag

        def rnn_agent(i):                                               # pyt_save/model.pt (epoch_logger.py:216-284)
            from .rada2c import RNNAgentPPO
            ag = RNNAgentPPO(id=i, device=dev)
            ag.load(agent_dir(i))
            return ag
        if arch == "cnn":
            from .maps import CNNCritic
            from .pfgru import PFGRUCell
            from .ppo_cnn import CNNAgentPPO
            from .maps import heat_map_geometry
            # the maps' side as the environment and train_PPO derive it: 27 with enforced walls, 27 + steps_per_episode without; the env's
            # bbox and observation area are RadSearchVec's defaults here, as in the runners
            d = inspect.signature(RadSearchVec.__init__).parameters
            bb, oa = d["bbox"].default, d["observation_area"].default
            env_cfg = SimpleNamespace(cfg=SimpleNamespace(bbox=(min(q[0] for q in bb), min(q[1] for q in bb), max(q[0] for q in bb),
                                                                max(q[1] for q in bb)), observation_area=oa))
            map_dim = tuple(heat_map_geometry(env_cfg, common["steps_per_episode"], common["enforce_grid_boundaries"])[2])
            agents = {}
            for i in range(A):
                ag = CNNAgentPPO(id=i, map_dim=map_dim, device=dev)
                ag.model = PFGRUCell().to(dev)
                ag.load(agent_dir(i))                                   # CNNBase.load (RADTEAM_core.py:1945-1953)
                agents[i] = ag
            # the HIP lock-steps where they apply (ids 0..A-1, a cuda device; 27 x 27 maps, or square maps of another side 8..256);
            # elsewhere the composed runner
            hip = torch.device(dev).type == "cuda" and 1 <= A <= _lib.RS_MAX_AGENTS
            if hip and map_dim == (27, 27):
                runner = run_test_environments_cnn_team
            elif hip and map_dim[0] == map_dim[1] and 8 <= map_dim[0] <= 256:
                runner = run_test_environments_cnn_team_sized
            else:
                runner = run_test_environments_cnn
            self.results, self.summary = runner(agents, sets, team_mode=kw.get("team_mode", "individual"), **common)
        elif arch == "rnn":
            carry = bool(kw.get("carry_hidden_across_runs", True))
            if A >= 2:
                # a recurrent team: one RNNModelActorCritic per agent on its own rows (evaluate.py:305-318)
                if kw.get("team_mode", "individual") != "individual":
                    raise ValueError("team_mode must be 'individual' for a recurrent team: no global critic for RAD-A2C")    # evaluate.py:279-280
                self.results, self.summary = run_test_environments_rnn_team({i: rnn_agent(i) for i in range(A)}, sets, fused=None,
                                                                            carry_hidden_across_runs=carry, **common)
            else:
                self.results, self.summary = run_test_environments_rnn(rnn_agent(0), sets, fused=None, carry_hidden_across_runs=carry, **common)
        elif arch == "gs":
            # the gradient-search baseline (eval/test_policy.py:73-108): no network, so no model_path is read
            self.results, self.summary = run_test_environments_gradient_search(sets, number_of_agents=A, q=float(kw.get("q", 1.0)),
                                                                               team_mode=kw.get("team_mode", "individual"), **common)
        elif arch == "rid-fim":
            # the information-driven baseline (eval/test_policy.py:184-231): no network, so no model_path is read
            bpf = {k: kw[k] for k in ("nParticles", "noise_params", "thresh", "intensity", "coord", "alpha", "fim_thresh", "interval") if k in kw}
            self.results, self.summary = run_test_environments_rid_fim(sets, number_of_agents=A, team_mode=kw.get("team_mode", "individual"),
                                                                       falloff=kw.get("falloff", "reference"), **common, **bpf)
        elif arch == "bpf-a2c":
            # the trained recurrent actor on the particle filter's estimate (eval/test_policy.py:109-156): agents as for 'rnn', the
            # filter's parameters as for 'rid-fim'; with `fisher` the posterior Cramer-Rao bounds are kept in self.extras["bounds"]
            bpf = {k: kw[k] for k in ("nParticles", "noise_params", "thresh", "intensity", "coord", "alpha", "fim_thresh", "interval") if k in kw}
            out = run_test_environments_bpf_a2c({i: rnn_agent(i) for i in range(A)}, sets, team_mode=kw.get("team_mode", "individual"),
                                                falloff=kw.get("falloff", "reference"), fisher=bool(kw.get("fisher", False)), **common, **bpf)
            self.results, self.summary = out[:2]
            self.extras = out[2] if len(out) > 2 else {}
        elif A >= 2:
            # a feed-forward team: every agent's own network on its own rows (evaluate.py:305-331)
            team_mode = kw.get("team_mode", "individual")
            if team_mode != "individual":
                raise ValueError("team_mode must be 'individual' for a feed-forward team: no global critic for RAD-A2C")   # evaluate.py:279-280
            agents = {i: ff_agent(i) for i in range(A)}
            self.results, self.summary = run_test_environments_team(agents, sets, team_mode=team_mode, **common)
        else:
            self.results, self.summary = run_test_environments(ff_agent(0), sets, **common)
        return self.results, self.summary
