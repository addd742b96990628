"""Bit-identity fixture of K7's critic pass (rs_ppo_grad2_body<1>: the value network's loss + gradient pass), recorded through
rs_ppo_update_step so that both launch forms are covered: the pair launch (critic workgroups in the upper half of one grid) and
one launch per network (RS_PPO_SPLIT_GRAD=1).

The cases sit at the edges of the group -> (workgroup, wave, trip) mapping (2048 waves per network, 32 samples per group):
M = 1 is one clamped group (every other wave runs a zero-weight trip), M = 33 a ragged second group, M = 32 * 2048 + 5 gives some
waves a second trip with a ragged tail.  The stop case sets rs_update_state.stopped before the step: zeros are published.
Inputs come from the seeded generators that make_k7_bits.py uses; only the critic's part of the gradient bucket and the value-loss
statistic are stored.
params(), batch() and run() live in tests/_k7_bits.py, which every bit-identity suite shares.

    python tests/golden/make_k7_critic_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "k7_critic_bits.npz")

sys.path.insert(0, os.path.dirname(HERE))
import _k7_bits as K  # noqa: E402

# (name, M, seed, stop flag set)
CASES = [("m1", 1, 21, False), ("m33", 33, 22, False), ("m65541", 32 * 2048 + 5, 23, False), ("stop", 33, 24, True)]
FORMS = ("pair", "split")


def run(M: int, seed: int, stop: bool, form: str):
    """(critic gradients float32 [4993], statistics float64 [5], whole bucket) after ONE rs_ppo_update_step (lr = 0) on cuda:0.
    begin_update() clears stopped, so it comes first: then the sentinel fill, then the stop flag."""
    r = K.run(K.params(seed), K.device_batch(K.batch(M, seed)), form, lr=0.0, stop=stop, begin="first")
    return r["g"][K.ACTOR_PARAMS:K.N_PARAMS].copy(), r["s"], r["g"]


def main():
    out = {}
    for name, M, seed, stop in CASES:
        g, s, _ = run(M, seed, stop, "pair")
        g2, s2, _ = run(M, seed, stop, "split")
        assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and np.array_equal(s.view(np.uint64), s2.view(np.uint64)), name
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(s)), name
        assert stop or g.any(), name
        out["g_" + name], out["s_" + name] = g, s[K.STAT_VALUE_LOSS:K.STAT_VALUE_LOSS + 1]
        print(name, M, "critic grad |max|", float(np.abs(g).max()), "value loss", float(s[K.STAT_VALUE_LOSS]))
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
