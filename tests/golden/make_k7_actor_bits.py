"""Bit-identity fixture of K7's actor pass (rs_ppo_grad2_body<8>: the policy network's loss + gradient pass), recorded before the
actor's output layer moved from VALU fmaf chains to v_mfma_f32_4x4x1_16b_f32 chains.  Every case runs three ways: rs_ppo_grad,
and rs_ppo_update_step (lr = 1e-3, first Adam step) as the pair launch and as one launch per network (RS_PPO_SPLIT_GRAD=1).
Stored per case: the actor's 5448 gradients, the five statistics and, for the update step, all 10441 parameters after Adam, as raw
bits.  The inputs of the small cases (M <= 33) are stored too; the large case is rebuilt from its seed (its rows alone are 2.9 MB).

Cases:
  m1 .. m65569   M = 1, 31, 32, 33 and 65536 + 33 (2048 waves of 32-sample groups: one wave takes a second trip, the last group is
                 ragged), inputs from the seeded generators of tests/_k7_bits.py.
  w3_distinct    W3[o][u] = +-(64 o + u + 1) / 4096: every (output, unit) has a magnitude of its own, so a wrong lane, output set
                 or unit mapping of the 4x4x1 operands cannot cancel.
  w3_denorm      W3 scaled to <= 1e-38 and b3 = 0: every product W3 * h2 is subnormal, the partial sums run through the subnormal
                 range and the logits are what the chains leave.
  x_tiny         inputs of about +-1e-30 with b1 = b2 = 0.  tanh is 1 - 2 / (1 + 2^y) here, so h2 cannot be about 1e-30: it
                 collapses to zeros, and the chains add signed-zero products.
  x_nan, x_inf   one row holds a NaN, two rows hold +inf / -inf.

params(), batch() and run() live in tests/_k7_bits.py, which every bit-identity suite shares.

    python tests/golden/make_k7_actor_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "k7_actor_bits.npz")

sys.path.insert(0, os.path.dirname(HERE))
import _k7_bits as K  # noqa: E402

# (name, M, seed, variant)
CASES = [("m1", 1, 31, "plain"), ("m31", 31, 32, "plain"), ("m32", 32, 33, "plain"), ("m33", 33, 34, "plain"),
         ("m65569", 65536 + 33, 35, "plain"), ("w3_distinct", 33, 36, "w3_distinct"), ("w3_denorm", 33, 37, "w3_denorm"),
         ("x_tiny", 33, 38, "x_tiny"), ("x_nan", 33, 39, "x_nan"), ("x_inf", 33, 40, "x_inf")]
PATHS = ("grad", "pair", "split")
KINDS = ("g", "s", "p")                  # what is stored: actor gradients, statistics, all parameters after Adam
LR = 1e-3
STORE_INPUTS_UP_TO = 33


def inputs(M: int, seed: int, variant: str):
    """(12 parameter arrays, 6 batch arrays) of one case."""
    p = K.params(seed)
    b = list(K.batch(M, seed))
    if variant == "w3_distinct":
        o, u = np.meshgrid(np.arange(8), np.arange(64), indexing="ij")
        p[4] = (np.where((o + u) % 3 == 0, -1.0, 1.0) * (64 * o + u + 1) / 4096.0).astype(np.float32)
    elif variant == "w3_denorm":
        p[4] = (p[4].astype(np.float64) * 8e-38).astype(np.float32)          # |W3| <= 0.125 * 8e-38 = 1e-38
        p[5] = np.zeros_like(p[5])
        assert np.abs(p[4]).max() < 1.1e-38 and np.count_nonzero(p[4]) == p[4].size
    elif variant == "x_tiny":
        b[0] = (b[0].astype(np.float64) * 1e-30).astype(np.float32)
        p[1] = np.zeros_like(p[1])
        p[3] = np.zeros_like(p[3])
    elif variant == "x_nan":
        b[0][5, 3] = np.nan
    elif variant == "x_inf":
        b[0][7, 2] = np.inf
        b[0][20, 9] = -np.inf
    else:
        assert variant == "plain"
    return p, b


def run(M: int, seed: int, variant: str, path: str):
    """(actor gradients float32 [5448], statistics float64 [5], parameters after Adam float32 [10441] or None) on cuda:0."""
    pv, bv = inputs(M, seed, variant)
    r = K.run(pv, K.device_batch(bv), path, lr=LR)
    return r["g"][:K.ACTOR_PARAMS], r["s"], r.get("p")


def main():
    out = {}
    for name, M, seed, variant in CASES:
        if M <= STORE_INPUTS_UP_TO:
            pv, bv = inputs(M, seed, variant)
            for k, v in zip(K.PARAM_NAMES[:6], pv[:6]):
                out[f"in_{name}_{k}"] = v
            for k, v in zip(K.BATCH_NAMES, bv):
                out[f"in_{name}_{k}"] = v
        for path in PATHS:
            g, s, p = run(M, seed, variant, path)
            got = {"g": g.view(np.uint32), "s": s.view(np.uint64)}
            if p is not None:
                assert p.shape == (K.N_PARAMS,)
                got["p"] = p.view(np.uint32)
            K.record(out, name, path, got)
            print(name, M, path, "finite grads", int(np.isfinite(g).sum()), "/", g.size, "grad |max|", float(np.nanmax(np.abs(g))) if
                  np.isfinite(g).any() else float("nan"), "stats", s.tolist(), flush=True)
        if variant in ("plain", "w3_distinct", "w3_denorm", "x_tiny"):
            assert np.all(np.isfinite(out[f"g_{name}_grad"].view(np.float32))), name
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
