"""Bit-identity fixture of K6 (rs_rollout16_kernel, the fused rollout), recorded while wave 0 computed all four output tiles of the
actor's two hidden layers itself (RsMlp16::hidden: 76 MFMAs and 32 tanh in one wave).  With one tile per wave (four waves per
workgroup, the tiles exchanged through LDS between workgroup barriers) the order of every sum is the same, so nothing a launch
leaves behind may change a bit.

Cases, the smallest at which the tile waves can go wrong (walls on, two collect() calls each so that carried state crosses a launch,
weights from params() of tests/_k7_bits.py times the scale):
  n16_t1_l1        N = 16, T = 1, L = 1: one workgroup, message -1 and one lock-step: the barrier counts at the shortest launch, and a
                   cut on the only step
  n16_t2_l120,     T = 2 and 3 with L = 120: the mailbox slot's parity for even and odd T
  n16_t3_l120
  n32_t7_l3_s*     N = 32 (two workgroups), T = 7, L = 3: cuts inside the launch (t = 2, 5) and on its last step, weight scales 1 and 4
                   (4: saturated tanh)
  n32_t7_l3_stag   the same, but the collector starts with steps_in_ep = env index mod 3, so that in every lock-step some envs of a
                   wave are cut and others are not: the helper waves must take the post-reset row for the former and the pre-reset
                   row for the latter (with steps_in_ep = 0 everywhere all envs of a wave time out together)
  n16_t7_l3_obs    N = 16, T = 7, L = 3 with obstruction_count -1: the obstacle template
  n4112_t3_l2_wide N = 4112 = 257 workgroups, one more than the MI355X has CUs: the library then launches the two-wave workgroup
                   (rs_rollout16_wide_kernel), two of which share a CU.  Digests only
Per case the fixture holds the SHA-256 digest of every field of make_k6_rollout_bits.py's list ("<case>/dig": uint8 [fields, 32],
rows in the order of FIELDS) and, for the cases of up to RAW_MAX_N envs, the raw arrays act, rew and obs of both launches
("<case>/<launch>_<name>"), so that a failure names the element.

main() checks on the CPU (float64, from the recorded observations) that a tile mix-up cannot hide: with any two of the four
16-unit tiles of the first or the second hidden layer swapped, the logits of every recorded sample of the N = 32 cases move by more
than 1e-3, a thousand times float32's rounding of these sums.

    python tests/golden/make_k6_tile_waves_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "k6_tile_waves_bits.npz")

sys.path.insert(0, os.path.dirname(HERE))
import _k7_bits as K  # noqa: E402

MK = K.maker("make_k6_rollout_bits")                   # BUF, COL, ENV, FIELDS: what a launch leaves behind
RAW = ("act", "rew", "obs")
RAW_MAX_N = 64
# (name, N, T, L, obstruction_count, seed, weight scale, staggered steps_in_ep)
CASES = [("n16_t1_l1", 16, 1, 1, 0, 611, 1.0, False),
         ("n16_t2_l120", 16, 2, 120, 0, 612, 1.0, False),
         ("n16_t3_l120", 16, 3, 120, 0, 613, 1.0, False),
         ("n32_t7_l3_s1", 32, 7, 3, 0, 614, 1.0, False),
         ("n32_t7_l3_s4", 32, 7, 3, 0, 615, 4.0, False),
         ("n32_t7_l3_stag", 32, 7, 3, 0, 616, 1.0, True),
         ("n16_t7_l3_obs", 16, 7, 3, -1, 617, 1.0, False),
         ("n4112_t3_l2_wide", 4112, 3, 2, 0, 618, 1.0, False)]


def run(N: int, T: int, L: int, obst: int, seed: int, scale: float, stagger: bool):
    """{key: numpy array} of one case on cuda:0, keys as in make_k6_rollout_bits.run"""
    import torch
    sys.path.insert(0, ROOT)
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.ppo import FusedCollector, VecAgentPPO
    env = RadSearchVec(N, number_agents=1, obstruction_count=obst, enforce_grid_boundaries=True, seed=seed)
    agents = {0: VecAgentPPO(id=0, steps_per_epoch=T, steps_per_episode=L, alpha=0.1)}
    ac = agents[0].agent
    ps = [ac.actor[0].weight, ac.actor[0].bias, ac.actor[2].weight, ac.actor[2].bias, ac.actor[4].weight, ac.actor[4].bias,
          ac.critic[0].weight, ac.critic[0].bias, ac.critic[2].weight, ac.critic[2].bias, ac.critic[4].weight, ac.critic[4].bias]
    with torch.no_grad():
        for p, v in zip(ps, weights(seed, scale)):
            p.copy_(torch.from_numpy(v))
    col = FusedCollector(env, agents, T, L)
    if stagger:
        col.start()
        col.steps_in_ep.copy_(torch.arange(N, dtype=torch.int32, device=col.steps_in_ep.device) % L)
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


def weights(seed: int, scale: float):
    """the twelve float32 arrays a case's networks hold"""
    return [(v.astype(np.float64) * scale).astype(np.float32) for v in K.params(seed)]


def digests(got) -> np.ndarray:
    """uint8 [len(FIELDS), 32]: SHA-256 of every field's bytes, rows in the order of FIELDS"""
    assert sorted(got) == sorted(MK.FIELDS)
    return np.stack([K.digest(got[k]) for k in MK.FIELDS])


def raw(got, launch: int, name: str) -> np.ndarray:
    return got[f"{launch}_buf_{name}"]


def logits(obs: np.ndarray, w, swap1=None, swap2=None) -> np.ndarray:
    """the actor's logits [samples, 8] in float64; swap1 / swap2 = (i, j): tiles i and j (units 16 i .. 16 i + 15) of hidden layer 1 /
    2 change places before the next layer reads them, which is what a tile handed to the wrong wave or slot would do"""
    w1, b1, w2, b2, w3, b3 = (a.astype(np.float64) for a in w[:6])

    def swapped(h, sw):
        if sw is None:
            return h
        i, j = sw
        h = h.copy()
        h[:, 16 * i:16 * i + 16], h[:, 16 * j:16 * j + 16] = h[:, 16 * j:16 * j + 16].copy(), h[:, 16 * i:16 * i + 16].copy()
        return h
    h1 = swapped(np.tanh(obs.astype(np.float64) @ w1.T + b1), swap1)
    h2 = swapped(np.tanh(h1 @ w2.T + b2), swap2)
    return h2 @ w3.T + b3


def tile_swaps_show(obs: np.ndarray, w) -> float:
    """the smallest change, over the samples and the twelve swaps, of a sample's logits (largest over its eight)"""
    base = logits(obs, w)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    return min(float(np.abs(logits(obs, w, **{kw: p}) - base).max(axis=1).min()) for kw in ("swap1", "swap2") for p in pairs)


def main():
    out, bad = {}, []
    for name, N, T, L, obst, seed, scale, stagger in CASES:
        got = run(N, T, L, obst, seed, scale, stagger)
        cut, logp = got["0_buf_cut"], got["0_buf_logp"]
        mixed = sum(int(0 < cut[t, 16 * b:16 * b + 16].sum() < 16) for t in range(T) for b in range(N // 16))
        print(name, "cuts", int(cut.sum()), "of", cut.size, "(wave, step) pairs with cut and uncut envs:", mixed, "episodes",
              int(got["1_col_ep_count"].sum()), "logp min", float(logp.min()), "err", int(got["1_err"][0]), flush=True)
        if not (cut[T - 1].all() and np.isfinite(logp).all() and int(got["1_err"][0]) == 0):
            bad.append(name)
        if L < T and not cut[:T - 1].any():
            bad.append(name + ": no cut inside the launch")
        if stagger and mixed < T - 1:
            bad.append(name + ": the envs of a wave are cut together")
        if N == 32:
            obs = np.concatenate([got[f"{launch}_buf_obs"].reshape(-1, got["0_buf_obs"].shape[-1]) for launch in range(2)])
            least = tile_swaps_show(obs, weights(seed, scale))
            print("    a swap of two hidden tiles moves every sample's logits by at least", least, flush=True)
            if not least > 1e-3:
                bad.append(name + ": a tile swap could hide")
        out[f"{name}/dig"] = digests(got)
        for launch in range(2 if N <= RAW_MAX_N else 0):
            for k in RAW:
                out[f"{name}/{launch}_{k}"] = raw(got, launch, k)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert not bad and os.path.getsize(path) < 200 * 1024, bad


if __name__ == "__main__":
    main()
