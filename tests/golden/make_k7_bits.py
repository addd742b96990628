"""Bit-identity fixture of K7 (rs_ppo_grad: the fused PPO loss + gradient pass of the FF_core actor and critic).

K7 feeds a chaotic RL loop: a last-bit change in one gradient eventually flips an action draw, so every layout or instruction
change inside the kernels must leave the gradients, the five statistics and the stop-flag path BITWISE equal.  This script
records what the library computes on inputs drawn from seeded numpy generators (the seeds are stored, not the inputs, so the
same inputs are rebuilt on every machine) and tests/test_k7_bitwise_gpu.py replays them with exact equality.
params(), batch() and run() live in tests/_k7_bits.py, which every bit-identity suite shares.

    python tests/golden/make_k7_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "k7_bits.npz")

sys.path.insert(0, os.path.dirname(HERE))
import _k7_bits as K  # noqa: E402

# (name, M, seed, stop flag set): M = 64 (one partial group), 1 000 and 20 483 (ragged tails, fewer groups than waves),
# 1 966 080 = BASELINE config 2's batch (4096 envs x 480 steps)
CASES = [("m64", 64, 11, False), ("m1000", 1000, 12, False), ("m20483", 20483, 13, False), ("m1966080", 1966080, 14, False),
         ("stop", 1000, 15, True)]


def run(name: str, M: int, seed: int, stop: bool):
    """(gradient bucket float32 [RS_PPO_GRAD_FLOATS], statistics float64 [5]) of one case, computed by the library on cuda:0."""
    r = K.run(K.params(seed), K.device_batch(K.batch(M, seed)), "grad", begin=None, stop=stop, use_stop_flag=stop)
    return r["g"], r["s"]


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
