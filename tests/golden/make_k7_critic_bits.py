"""Bit-identity fixture of K7's critic pass (rs_ppo_grad2_body<1>: the value network's loss + gradient pass), recorded through
rs_ppo_update_step so that both launch forms are covered: the pair launch (critic workgroups in the upper half of one grid) and
one launch per network (RS_PPO_SPLIT_GRAD=1).

The cases sit at the edges of the group -> (workgroup, wave, trip) mapping (2048 waves per network, 32 samples per group):
M = 1 is one clamped group (every other wave runs a zero-weight trip), M = 33 a ragged second group, M = 32 * 2048 + 5 gives some
waves a second trip with a ragged tail.  The stop case sets rs_update_state.stopped before the step: zeros are published.
Inputs come from the seeded generators of make_k7_bits.py (which stays as it is); only the critic's part of the gradient bucket
and the value-loss statistic are stored.

    python tests/golden/make_k7_critic_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "k7_critic_bits.npz")

_spec = importlib.util.spec_from_file_location("make_k7_bits", os.path.join(HERE, "make_k7_bits.py"))
K7 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(K7)

# (name, M, seed, stop flag set)
CASES = [("m1", 1, 21, False), ("m33", 33, 22, False), ("m65541", 32 * 2048 + 5, 23, False), ("stop", 33, 24, True)]
FORMS = ("pair", "split")
ACTOR_PARAMS = 5448           # the critic's 4993 gradients lie behind the actor's in the bucket
N_PARAMS = 10441
STAT_VALUE_LOSS = 3


def run(M: int, seed: int, stop: bool, form: str):
    """(critic gradients float32 [4993], statistics float64 [5], whole bucket) after ONE rs_ppo_update_step (lr = 0) on cuda:0."""
    import torch
    sys.path.insert(0, ROOT)
    from radiation_ppo_amd.ppo import FFActorCritic, FusedPPOGrad
    ac = FFActorCritic().cuda()
    with torch.no_grad():
        ps = [ac.actor[0].weight, ac.actor[0].bias, ac.actor[2].weight, ac.actor[2].bias, ac.actor[4].weight, ac.actor[4].bias,
              ac.critic[0].weight, ac.critic[0].bias, ac.critic[2].weight, ac.critic[2].bias, ac.critic[4].weight, ac.critic[4].bias]
        for p, v in zip(ps, K7.params(seed)):
            p.copy_(torch.from_numpy(v))
    b = [torch.from_numpy(a).cuda() for a in K7.batch(M, seed)]
    f = FusedPPOGrad(ac)
    f.begin_update()
    f.bucket.fill_(7.0)                      # the stop path must overwrite these
    f.stats.fill_(7.0)
    if stop:
        f.state_i32[1] = 1                   # rs_update_state.stopped
    old = os.environ.pop("RS_PPO_SPLIT_GRAD", None)
    try:
        if form == "split":
            os.environ["RS_PPO_SPLIT_GRAD"] = "1"
        f.step(*b, K7.CLIP, K7.ALPHA, K7.VF, lr=0.0, kl_threshold=1e30)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("RS_PPO_SPLIT_GRAD", None)
        if old is not None:
            os.environ["RS_PPO_SPLIT_GRAD"] = old
    bucket = f.bucket.cpu().numpy().copy()
    return bucket[ACTOR_PARAMS:N_PARAMS].copy(), f.stats.cpu().numpy().copy(), bucket


def main():
    out = {}
    for name, M, seed, stop in CASES:
        g, s, _ = run(M, seed, stop, "pair")
        g2, s2, _ = run(M, seed, stop, "split")
        assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and np.array_equal(s.view(np.uint64), s2.view(np.uint64)), name
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(s)), name
        assert stop or g.any(), name
        out["g_" + name], out["s_" + name] = g, s[STAT_VALUE_LOSS:STAT_VALUE_LOSS + 1]
        print(name, M, "critic grad |max|", float(np.abs(g).max()), "value loss", float(s[STAT_VALUE_LOSS]))
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
