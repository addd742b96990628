"""Plain-Python reference of the env look-ahead (rs_peek; RadSearch.FIM_step, rad_search_env.py:1768-1799, over all eight moves with a
measurement at each candidate) and of the gradient-search controller on top of it (rs_gs_eval_step; GradSearch.step,
algos/test_environment/eval/core.py:636-653), over a RadSearchOracle and built from the oracle's own pieces: its take_action rule
(_take_action), shortest_path_len, dist_i, _is_intersect, _lam, and poisson_from_uniforms on the look-ahead's streams.  The oracle is
never changed: the rule is applied to a stand-in agent and the oracle's error word is put back."""
import copy

import numpy as np
import torch

from oracle.radsearch_oracle import OracleAgent, dist_i, philox4x32_10, poisson_from_uniforms, shortest_path_len, u53

STREAM_PEEK = 128                    # + 8 * agent + move (RS_STREAM_PEEK in csrc/rs_device.hpp)


def candidate(env, a, k, start=None):
    """(xy, moved, lam, meas) of move k (0..7) of agent a from `start` (default: its position)."""
    ag = env.agents[a]
    tmp = OracleAgent(a)
    tmp.det = tmp.detector = tuple(int(v) for v in (ag.det if start is None else start))
    tmp.out_of_bounds_count = ag.out_of_bounds_count
    moved = env._take_action(tmp, k, [])                           # no proposed coordinates: no collision rule (:1789)
    x, y = tmp.det
    tmp.sp_dist = shortest_path_len(env.src[0], env.src[1], x, y, env.rects, env.dsrc)
    tmp.euc_dist = dist_i(x, y, env.src[0], env.src[1])
    tmp.intersect = env._is_intersect(tmp)
    err = env.err
    lam = env._lam(tmp)
    env.err = err                                                  # r == 0 is taken as 1 and no error bit is set
    rng = env.rng

    def next_uv(i):
        o = philox4x32_10(i & 0xFFFFFFFF, env.t & 0xFFFFFFFF, rng.episode, STREAM_PEEK + 8 * a + k, rng.k0, rng.k1)
        return u53(o[0], o[1]), u53(o[2], o[3])
    return (x, y), bool(moved), lam, poisson_from_uniforms(lam, next_uv)


def peek(env, from_xy=None):
    """rs_peek for one oracle env: xy int32 [A,8,2], moved uint8 [A,8], lam float64 [A,8], meas int64 [A,8]."""
    A = env.number_agents
    xy, moved = np.zeros((A, 8, 2), np.int32), np.zeros((A, 8), np.uint8)
    lam, meas = np.zeros((A, 8), np.float64), np.zeros((A, 8), np.int64)
    for a in range(A):
        for k in range(8):
            xy[a, k], moved[a, k], lam[a, k], meas[a, k] = candidate(env, a, k, None if from_xy is None else from_xy[a])
    return xy, moved, lam, meas


def step_candidate(env, k):
    """The pinned oracle's own answer: a deep copy stepped with its int form step(k), which applies no collision rule.  Returns per
    agent (position, moved, last_lam)."""
    twin = copy.deepcopy(env)
    before = [twin.agents[a].det for a in range(twin.number_agents)]
    twin.step(int(k))
    return [(twin.agents[a].det, twin.agents[a].det != before[a], twin.last_lam[a]) for a in range(twin.number_agents)]


def gradient(meas_now, meas, moved, q):
    """grad float32 [..., 8] of GradSearch.step (core.py:641-644): (meas_k - meas_now) * 0.01 * (1 / q) in float64 -- Python floats in
    the reference --, rounded once by the store into the float32 tensor; 0 for a move that did not take place."""
    q_rec = 1 / q                                                  # core.py:624
    g = (np.asarray(meas, np.float64) - np.asarray(meas_now, np.float64)[..., None]) * 0.01 * q_rec
    return np.where(np.asarray(moved, bool), g.astype(np.float32), np.float32(0.0)).astype(np.float32)


def draw(grad32, u):
    """The action of Categorical(softmax(grad)) as the inverse-CDF draw from u, in float64 (tests/_f64_ref.py draw_f64's arithmetic):
    (action int64 [...], probabilities float64 [..., 8], CDF float64 [..., 8])."""
    lp = torch.log_softmax(torch.as_tensor(np.asarray(grad32)).double(), dim=-1)
    cdf = torch.cumsum(lp.exp(), dim=-1)
    act = (cdf[..., :-1] <= torch.as_tensor(np.asarray(u)).double().unsqueeze(-1)).sum(dim=-1)
    return act.numpy(), lp.exp().numpy(), cdf.numpy()


EDGE = 16 * 2.0 ** -24               # a float32 CDF of 8 expf terms may sit this far from the float64 one


def near_edge(cdf64, u):
    """the draws whose uniform lies within EDGE of a float64 CDF step: the float32 kernel may take the neighbouring action there"""
    return np.abs(np.asarray(cdf64)[..., :-1] - np.asarray(u, np.float64)[..., None]).min(axis=-1) < EDGE


def controller_action(env, obs0, u, q):
    """The reference controller's action for every agent of env in its present state: (actions int64 [A], near_edge [A], grad [A, 8]);
    obs0 [A]: the agents' current readings, u [A]: the env's action uniforms of this step."""
    _, moved, _, meas = peek(env)
    g = gradient(np.asarray(obs0, np.float64), meas, moved, q)
    act, _, cdf = draw(g, u)
    return act, near_edge(cdf, u), g


def action_uniforms(env):
    """rs_action_uniforms for one oracle env: float32 [A]"""
    rng = env.rng
    return np.array([np.float32(philox4x32_10(0, env.t & 0xFFFFFFFF, rng.episode, 32 + a, rng.k0, rng.k1)[0] >> 8) * np.float32(1.0 / 16777216.0)
                     for a in range(env.number_agents)], dtype=np.float32)

