"""Bit-identity fixture of K7 (rs_ppo_grad: the fused PPO loss + gradient pass of the FF_core actor and critic).

K7 feeds a chaotic RL loop: a last-bit change in one gradient eventually flips an action draw, so every layout or instruction
change inside the kernels must leave the gradients, the five statistics and the stop-flag path BITWISE equal.  This script
records what the library computes on inputs drawn from seeded numpy generators (the seeds are stored, not the inputs, so the
same inputs are rebuilt on every machine) and tests/test_k7_bitwise_gpu.py replays them with exact equality.

    python tests/golden/make_k7_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "k7_bits.npz")

# (name, M, seed, stop flag set): M = 64 (one partial group), 1 000 and 20 483 (ragged tails, fewer groups than waves),
# 1 966 080 = BASELINE config 2's batch (4096 envs x 480 steps)
CASES = [("m64", 64, 11, False), ("m1000", 1000, 12, False), ("m20483", 20483, 13, False), ("m1966080", 1966080, 14, False),
         ("stop", 1000, 15, True)]
CLIP, ALPHA, VF = 0.2, 0.01, 0.01


def params(seed: int):
    """FF_core parameters (actor then critic, nn.Linear order) as float32 numpy arrays, uniform(+-1/sqrt(fan_in)) like torch's init."""
    rng = np.random.default_rng(seed)
    out = []
    for nout in (8, 1):
        for fi, fo in ((11, 64), (64, 64), (64, nout)):
            b = 1.0 / np.sqrt(fi)
            out.append(rng.uniform(-b, b, (fo, fi)).astype(np.float32))
            out.append(rng.uniform(-b, b, (fo,)).astype(np.float32))
    return out


def batch(M: int, seed: int):
    """X, act, adv, ret, logp_old, w.  logp_old scatters around log(1/8) so that the ratios fall on both sides of the clip
    interval; the weights are non-uniform."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((M, 11)).astype(np.float32)
    act = rng.integers(0, 8, M).astype(np.int64)
    adv = rng.standard_normal(M).astype(np.float32)
    ret = rng.standard_normal(M).astype(np.float32)
    lpo = (np.log(0.125) + 0.4 * rng.standard_normal(M)).astype(np.float32)
    w = (rng.uniform(0.25, 1.75, M) / M).astype(np.float32)
    return X, act, adv, ret, lpo, w


def run(name: str, M: int, seed: int, stop: bool):
    """(gradient bucket float32 [RS_PPO_GRAD_FLOATS], statistics float64 [5]) of one case, computed by the library on cuda:0."""
    import torch
    sys.path.insert(0, ROOT)
    from radiation_ppo_amd.ppo import FFActorCritic, FusedPPOGrad
    ac = FFActorCritic().cuda()
    with torch.no_grad():
        ps = [ac.actor[0].weight, ac.actor[0].bias, ac.actor[2].weight, ac.actor[2].bias, ac.actor[4].weight, ac.actor[4].bias,
              ac.critic[0].weight, ac.critic[0].bias, ac.critic[2].weight, ac.critic[2].bias, ac.critic[4].weight, ac.critic[4].bias]
        for p, v in zip(ps, params(seed)):
            p.copy_(torch.from_numpy(v))
    X, act, adv, ret, lpo, w = (torch.from_numpy(a).cuda() for a in batch(M, seed))
    f = FusedPPOGrad(ac)
    f.bucket.fill_(7.0)                      # the stop path must overwrite these
    f.stats.fill_(7.0)
    if stop:
        f.state_i32[1] = 1                   # rs_update_state.stopped
    st, _ = f(X, act, adv, ret, lpo, w, CLIP, ALPHA, VF, use_stop_flag=stop)
    torch.cuda.synchronize()
    return f.bucket.cpu().numpy().copy(), st.cpu().numpy().copy()


def main():
    out = {}
    for name, M, seed, stop in CASES:
        g, s = run(name, M, seed, stop)
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(s)), name
        out["g_" + name], out["s_" + name] = g, s
        print(name, M, "grad |max|", float(np.abs(g).max()), "stats", s.tolist())
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
