"""Bit-identity fixture of K6 (rs_rollout16_kernel, the fused rollout), recorded before wave 0's lock-step chain was shortened:
actor weights held in registers, the actor's output layer on v_mfma_f32_4x4x1_16b_f32 chains, and the env state carried in
registers across the lock-steps.  None of that may change a bit of what a launch leaves behind.

A case builds a FusedCollector and calls collect() twice, so that the carried state (Welford, running returns, the env arrays)
crosses a launch.  After each collect() it records, as raw bytes:
  buf_*    every rollout buffer field the kernel or the GAE pass writes (obs, act, rew, val, logp, last_val, cut, source_tar, adv, ret)
  col_*    cur_obs, the Welford carry (w_count, w_mean, w_sq, w_std), steps_in_ep, ep_ret and the episode statistics
  env_*    the env state arrays (x, y, sp, prev, oob_count, aflags, done, iter_count, tstep, episode, src_x, src_y, intensity, bkg,
           epoch_end, err, num_obs)
  err      error_flags()
A case is stored as ONE uint8 vector, blob(): the fields in the order of FIELDS, each through pack() (its bytes, regrouped into
byte planes).  One member per case instead of one per field keeps the fixture under 1 MB (1 376 zip members cost 0.4 MB alone).

Cases: 16 and 48 envs (one and three workgroups) x walls on / off x obstruction_count 0 / -1 (both kernel templates), each with
two (seed, weight scale) pairs.  steps_per_epoch = 23 with steps_per_episode = 5: timeouts, cuts, bootstraps and the t == T - 1
epoch end all occur in every case.  Weights are uniform(+-1/sqrt(fan_in)) times the scale; at scale 4 the logits span several
units (main() asserts that the recorded log-probabilities reach below -4), so the output layer's sums carry real rounding.

The weights come from params() of tests/_k7_bits.py, which every bit-identity suite shares.

    python tests/golden/make_k6_rollout_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "k6_rollout_bits.npz")

sys.path.insert(0, os.path.dirname(HERE))
import _k7_bits as K  # noqa: E402

T, L = 23, 5
SEEDS = ((101, 1.0), (202, 4.0))                      # (seed of env and weights, weight scale)
# (name, N, walls, obstruction_count, seed, scale)
CASES = [(f"n{N}_{'walls' if walls else 'open'}_{'obs' if obst else 'free'}_s{seed}", N, walls, obst, seed, scale)
         for N in (16, 48) for walls in (True, False) for obst in (0, -1) for seed, scale in SEEDS]
BUF = ("obs", "act", "rew", "val", "logp", "last_val", "cut", "source_tar", "adv", "ret")
COL = ("cur_obs", "w_count", "w_mean", "w_sq", "w_std", "steps_in_ep", "ep_ret", "done_count", "oob_count", "ep_count", "ep_ret_sum",
       "ep_len_sum", "ep_ret_sq", "ep_ret_max", "ep_ret_min")
ENV = ("x", "y", "sp", "prev", "oob_count", "aflags", "done", "iter_count", "tstep", "episode", "src_x", "src_y", "intensity", "bkg",
       "epoch_end", "err", "num_obs")


def pack(v: np.ndarray) -> np.ndarray:
    """the bytes of v, byte plane by byte plane (uint8 [itemsize, v.size]): the same information as v.tobytes(), but the sign /
    exponent bytes of neighbouring floats lie together, which halves the compressed fixture"""
    v = np.ascontiguousarray(v)
    return v.reshape(-1).view(np.uint8).reshape(-1, v.dtype.itemsize).T.copy()


FIELDS = [f for launch in range(2) for f in [f"{launch}_buf_{k}" for k in BUF] + [f"{launch}_col_{k}" for k in COL] +
          [f"{launch}_env_{k}" for k in ENV] + [f"{launch}_err"]]


def blob(got) -> np.ndarray:
    """one case's record: the packed fields of run()'s result, concatenated in the order of FIELDS"""
    assert sorted(got) == sorted(FIELDS)
    return np.concatenate([pack(got[k]).ravel() for k in FIELDS])


def run(N: int, walls: bool, obst: int, seed: int, scale: float):
    """{key: numpy array} of one case on cuda:0: keys '<launch>_<group>_<field>' and '<launch>_err', launch = 0, 1"""
    import torch
    sys.path.insert(0, ROOT)
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.ppo import FusedCollector, VecAgentPPO
    env = RadSearchVec(N, number_agents=1, obstruction_count=obst, enforce_grid_boundaries=walls, seed=seed)
    agents = {0: VecAgentPPO(id=0, steps_per_epoch=T, steps_per_episode=L, alpha=0.1)}
    ac = agents[0].agent
    ps = [ac.actor[0].weight, ac.actor[0].bias, ac.actor[2].weight, ac.actor[2].bias, ac.actor[4].weight, ac.actor[4].bias,
          ac.critic[0].weight, ac.critic[0].bias, ac.critic[2].weight, ac.critic[2].bias, ac.critic[4].weight, ac.critic[4].bias]
    with torch.no_grad():
        for p, v in zip(ps, K.params(seed)):
            p.copy_(torch.from_numpy((v.astype(np.float64) * scale).astype(np.float32)))
    col = FusedCollector(env, agents, T, L)
    out = {}
    for launch in range(2):
        col.collect()
        torch.cuda.synchronize()
        for k in BUF:
            out[f"{launch}_buf_{k}"] = getattr(col.buf, k).cpu().numpy().copy()
        for k in COL:
            out[f"{launch}_col_{k}"] = getattr(col, k).cpu().numpy().copy()
        for k in ENV:
            out[f"{launch}_env_{k}"] = env.state(k).cpu().numpy().copy()
        out[f"{launch}_err"] = np.array([env.error_flags()], dtype=np.uint32)
    return out


def main():
    out, bad = {}, []
    for name, N, walls, obst, seed, scale in CASES:
        got = run(N, walls, obst, seed, scale)
        cut, lastv, logp = got["0_buf_cut"], got["0_buf_last_val"], got["0_buf_logp"]
        print(name, "cuts", int(cut.sum()), "of", cut.size, "boots", int((lastv != 0).sum()), "episodes", int(got["1_col_ep_count"].sum()),
              "logp min", float(logp.min()), "err", int(got["1_err"][0]), flush=True)
        if not (cut[T - 1].all() and cut[:T - 1].any() and (lastv != 0).any() and np.isfinite(logp).all()):
            bad.append(name)
        if scale > 1.0 and not logp.min() < -4.0:
            bad.append(name)
        out[name] = blob(got)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert not bad and os.path.getsize(path) < (1 << 20), bad


if __name__ == "__main__":
    main()
