"""Bit-identity fixture of K6 (rs_rollout16_kernel, the fused rollout), recorded while its measurement draw was the serial
rs_poisson loop and its action uniform a Philox block of its own inside the softmax.  The grouped sampler (rs_poisson_group,
csrc/rs_device.hpp: candidates 0..2 of the draw evaluated at once in three lanes of the env, the serial loop only from candidate 3
on) and the one Philox call per lock-step may not change a bit of what a launch leaves behind.

Cases (T = 60 steps per epoch, L = 20 per episode, walls on, two collect() calls each, weights from params() of tests/_k7_bits.py):
  n64_free_*    N = 64 (four workgroups), obstruction_count 0: the headline template, weight scales 1 and 4
  n64_obs_*     the same with obstruction_count -1: the obstacle template
  n16_invsq     N = 16, falloff="inverse_square", DEBUG=True: source (500, 500), detector (1000, 1000), intensity 1e6, no
                background, so the rate is 1e6 / r^2: below 10 beyond r = 316 (rs_poisson_small inside K6) and PTRS nearer
Per case and launch the fixture holds the SHA-256 digest of every field of make_k6_rollout_bits.py's list ("<case>/dig": uint8
[fields, 32], rows in the order of FIELDS) and the raw arrays act, rew and obs[..., 0] ("<case>/<launch>_<name>"), so that a
failure names the element.

main() replays the recorded actions of the obstacle-free cases through RadSearchOracle on the CPU (the rewards must come out as
recorded), counts the candidates every measurement draw of a step consumed, and asserts that at least 5 draws of the n64_free
cases needed more than 3 (the in-kernel fallback is then on the tested path) and that n16_invsq holds rates on both sides of 10.

    python tests/golden/make_k6_poisson_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "k6_poisson_bits.npz")

sys.path.insert(0, os.path.dirname(HERE))
import _k7_bits as K  # noqa: E402

MK = K.maker("make_k6_rollout_bits")                   # BUF, COL, ENV, FIELDS: what a launch leaves behind
T, L = 60, 20
RAW = ("act", "rew", "obs0")
# (name, N, obstruction_count, falloff, DEBUG, seed, weight scale)
CASES = [(f"n64_{'obs' if obst else 'free'}_s{seed}", 64, obst, "reference", False, seed, scale)
         for obst in (0, -1) for seed, scale in ((303, 1.0), (404, 4.0))] + [("n16_invsq", 16, 0, "inverse_square", True, 505, 1.0)]


def run(N: int, obst: int, falloff: str, debug: bool, seed: int, scale: float):
    """{key: numpy array} of one case on cuda:0, keys as in make_k6_rollout_bits.run"""
    import torch
    sys.path.insert(0, ROOT)
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.ppo import FusedCollector, VecAgentPPO
    env = RadSearchVec(N, number_agents=1, obstruction_count=obst, enforce_grid_boundaries=True, seed=seed, falloff=falloff, DEBUG=debug)
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
        for k in MK.BUF:
            out[f"{launch}_buf_{k}"] = getattr(col.buf, k).cpu().numpy().copy()
        for k in MK.COL:
            out[f"{launch}_col_{k}"] = getattr(col, k).cpu().numpy().copy()
        for k in MK.ENV:
            out[f"{launch}_env_{k}"] = env.state(k).cpu().numpy().copy()
        out[f"{launch}_err"] = np.array([env.error_flags()], dtype=np.uint32)
    return out


def digests(got) -> np.ndarray:
    """uint8 [len(FIELDS), 32]: SHA-256 of every field's bytes, rows in the order of FIELDS"""
    assert sorted(got) == sorted(MK.FIELDS)
    return np.stack([K.digest(got[k]) for k in MK.FIELDS])


def raw(got, launch: int, name: str) -> np.ndarray:
    """the arrays stored in full: act, rew, and the first column of obs (the standardised reading)"""
    if name == "obs0":
        return np.ascontiguousarray(got[f"{launch}_buf_obs"][..., 0])
    return got[f"{launch}_buf_{name}"]


def replay(got, N: int, falloff: str, debug: bool, seed: int):
    """[(rate, candidates consumed)] of every measurement draw inside a step of the two launches, from RadSearchOracle driven by the
    recorded actions and cuts on the CPU; the rewards it returns must be the recorded ones"""
    sys.path.insert(0, ROOT)
    from oracle.radsearch_oracle import PhiloxDraws, RadSearchOracle, philox4x32_10, poisson_from_uniforms, u53
    log = []

    class Counting(PhiloxDraws):
        in_step = False

        def poisson(self, lam, agent):
            used = [0]

            def next_uv(i):
                used[0] = i + 1
                o = philox4x32_10(i & 0xFFFFFFFF, self.t, self.episode, 1 + agent, self.k0, self.k1)
                return u53(o[0], o[1]), u53(o[2], o[3])
            v = poisson_from_uniforms(lam, next_uv)
            if self.in_step:
                log.append((float(lam), used[0]))
            return v

    for n in range(N):
        draws = Counting(seed, n)
        ref = RadSearchOracle(draws, number_agents=1, obstruction_count=0, enforce_grid_boundaries=True, falloff=falloff, DEBUG=debug)
        for launch in range(2):
            act, rew, cut = (got[f"{launch}_buf_{k}"] for k in ("act", "rew", "cut"))
            for t in range(T):
                draws.in_step = True
                _, rr, _, _ = ref.step({0: int(act[t, n, 0])})
                draws.in_step = False
                assert np.float32(rr["individual_reward"][0]) == rew[t, n, 0], ("replay", launch, t, n)
                if cut[t, n, 0]:
                    ref.reset()
    return log


def main():
    out, bad, over3 = {}, [], 0
    for name, N, obst, falloff, debug, seed, scale in CASES:
        got = run(N, obst, falloff, debug, seed, scale)
        cut, logp = got["0_buf_cut"], got["0_buf_logp"]
        print(name, "cuts", int(cut.sum()), "of", cut.size, "episodes", int(got["1_col_ep_count"].sum()), "logp min", float(logp.min()),
              "err", int(got["1_err"][0]), flush=True)
        if not (cut[T - 1].all() and cut[:T - 1].any() and np.isfinite(logp).all() and int(got["1_err"][0]) == 0):
            bad.append(name)
        if obst == 0:
            log = replay(got, N, falloff, debug, seed)
            lam = np.array([r for r, _ in log])
            used = np.array([c for _, c in log])
            ptrs = lam >= 10.0
            print("   ", len(log), "draws in steps; rate", float(lam.min()), "..", float(lam.max()), "; below 10:", int((~ptrs).sum()),
                  "; PTRS draws with > 1 / > 3 / > 4 candidates:", int((used[ptrs] > 1).sum()), int((used[ptrs] > 3).sum()),
                  int((used[ptrs] > 4).sum()), flush=True)
            assert len(log) == 2 * T * N
            if debug and not ((~ptrs).sum() >= 100 and ptrs.sum() >= 10):
                bad.append(name + ": rates on one side of 10")
            if not debug:
                over3 += int((used[ptrs] > 3).sum())
        out[f"{name}/dig"] = digests(got)
        for launch in range(2):
            for k in RAW:
                out[f"{name}/{launch}_{k}"] = raw(got, launch, k)
    print("draws of the n64_free cases that needed more than 3 candidates:", over3)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert over3 >= 5, over3
    assert not bad and os.path.getsize(path) < (1 << 20), bad


if __name__ == "__main__":
    main()
