"""Bit-identity fixture of K7's actor pass (rs_ppo_grad2_body<8>), recorded before the actor's dW3 / db3 / statistics phase moved from
16x16x4 MFMA tiles to chains of v_mfma_f32_4x4x1_16b_f32 and before the tanh / tanh' chains of both networks were packed in pairs.
Every case runs three ways: rs_ppo_grad, and rs_ppo_update_step (lr = 1e-3, first Adam step) as the pair launch and as one launch
per network (RS_PPO_SPLIT_GRAD=1).  Stored per case, as raw bits: the actor's 5448 gradients, the five statistics and, for the update
step, the actor's 5448 parameters after Adam in full and the critic's 4993 as a SHA-256 digest (17 cases of all 10441 words would not
fit a committed file; the critic's own gradients are pinned word by word in k7_critic_bits.npz).  All cases share one parameter set
(stored once; w3_denorm stores its own W3 / b3); the batch arrays of the small cases (M <= 64) are stored, the large case is rebuilt
from its seed.

Cases:
  m1 .. m65553   M = 1, 3, 4, 5 (the edges of a four-sample b128 operand chunk), 15, 16, 17 (where the row-sum chain changes
                 halves), 31, 32, 33 and 65536 + 17 (2048 waves: one takes a second trip, whose A rows overlay the zones the
                 look-ahead DMA refills; the last group is ragged).  Seeded generators of make_k7_bits.py.
  decades        |adv| = 10^U(-8, 4): dz has a magnitude of its own per (output, sample), so a wrong sample order or a wrong
                 (output, unit) block cannot cancel.
  all_actions    every group of 32 holds all eight actions, four times each.
  zero_w_clip    every third row has weight 0 (one of them -0.0); every third row has its ratio far outside the clip interval
                 on the side where the surrogate is flat, so dz = +-0 there.
  x_nan, x_inf   one row holds a NaN, two rows hold +inf / -inf.
  w3_denorm      W3 scaled to <= 1e-38 and b3 = 0.

At record time every finite case with M > 1 also runs (rs_ppo_grad) with the rows of every 32-sample group reversed.  The number of
dW3, db3 and statistics words that then differ from the forward order is stored (rev_<case> = [dW3, db3, statistics]) and, from M =
15 up, asserted to be nonzero in all three: the inputs can see a summation-order error.  (Swapping two neighbouring samples would
not show that: a + b commutes.  Below M = 15 a sum has so few terms that its reversal may round the same.)

params(), batch() and run() live in tests/_k7_bits.py, which every bit-identity suite shares.

    python tests/golden/make_k7_actor_dw3_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "k7_actor_dw3_bits.npz")

sys.path.insert(0, os.path.dirname(HERE))
import _k7_bits as K  # noqa: E402

# (name, M, batch seed, variant)
CASES = [("m1", 1, 51, "plain"), ("m3", 3, 52, "plain"), ("m4", 4, 53, "plain"), ("m5", 5, 54, "plain"),
         ("m15", 15, 55, "plain"), ("m16", 16, 56, "plain"), ("m17", 17, 57, "plain"),
         ("m31", 31, 58, "plain"), ("m32", 32, 59, "plain"), ("m33", 33, 60, "plain"),
         ("m65553", 65536 + 17, 61, "plain"),
         ("decades", 64, 62, "decades"), ("all_actions", 64, 63, "all_actions"), ("zero_w_clip", 64, 64, "zero_w_clip"),
         ("x_nan", 64, 65, "x_nan"), ("x_inf", 64, 66, "x_inf"), ("w3_denorm", 64, 67, "w3_denorm")]
PATHS = ("grad", "pair", "split")
KINDS = ("g", "s", "p", "c")             # what is stored: actor gradients, statistics, actor parameters after Adam, the critic's digest
FINITE = ("plain", "decades", "all_actions", "zero_w_clip", "w3_denorm")
PARAM_SEED = 50
W3_OFF, B3_OFF = 4928, 5440          # actor slab: w1 704, b1 64, w2 4096, b2 64, w3 512, b3 8
LR = 1e-3
STORE_INPUTS_UP_TO = 64
REV_ASSERT_FROM = 15


def inputs(M: int, seed: int, variant: str):
    """(12 parameter arrays, 6 batch arrays) of one case."""
    p = K.params(PARAM_SEED)
    b = list(K.batch(M, seed))
    rng = np.random.default_rng(1000 + seed)
    i = np.arange(M)
    if variant == "decades":
        b[2] = (np.where(rng.random(M) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-8.0, 4.0, M)).astype(np.float32)
    elif variant == "all_actions":
        b[1] = ((3 * i + i // 8) % 8).astype(np.int64)
        for g0 in range(0, M - 31, 32):
            assert np.array_equal(np.bincount(b[1][g0:g0 + 32], minlength=8), np.full(8, 4))
    elif variant == "zero_w_clip":
        b[5][i % 3 == 0] = 0.0
        b[5][3] = -0.0
        # logp is log(1/8) +- a little for these parameters: ratio = exp(logp - lpo) is about e^3 or e^-3, far outside 1 +- 0.2, on
        # the side where min(ratio adv, clip(ratio) adv) is the clipped term (adv > 0 above, adv < 0 below) -> dr = 0, dz = +-0
        clip = i % 3 == 1
        b[4][clip] = (np.log(0.125) + np.where(b[2][clip] > 0, -3.0, 3.0)).astype(np.float32)
    elif variant == "x_nan":
        b[0][5, 3] = np.nan
    elif variant == "x_inf":
        b[0][7, 2] = np.inf
        b[0][40, 9] = -np.inf
    elif variant == "w3_denorm":
        p[4] = (p[4].astype(np.float64) * 8e-38).astype(np.float32)          # |W3| <= 0.125 * 8e-38 = 1e-38
        p[5] = np.zeros_like(p[5])
        assert np.abs(p[4]).max() < 1.1e-38 and np.count_nonzero(p[4]) == p[4].size
    else:
        assert variant == "plain"
    return p, b


def reversed_groups(bv):
    """the batch with the rows of every 32-sample group in reverse order (a ragged last group within its own rows)"""
    M = bv[0].shape[0]
    idx = np.concatenate([np.arange(min(g0 + 32, M) - 1, g0 - 1, -1) for g0 in range(0, M, 32)])
    assert np.array_equal(np.sort(idx), np.arange(M))
    return [np.ascontiguousarray(a[idx]) for a in bv]


def run_arrays(pv, bv, path: str):
    """(actor gradients float32 [5448], statistics float64 [5], parameters after Adam float32 [10441] or None) on cuda:0."""
    r = K.run(pv, K.device_batch(bv), path, lr=LR)
    return r["g"][:K.ACTOR_PARAMS], r["s"], r.get("p")


def run(M: int, seed: int, variant: str, path: str, reverse: bool = False):
    pv, bv = inputs(M, seed, variant)
    return run_arrays(pv, reversed_groups(bv) if reverse else bv, path)


def words(g, s, p):
    """what is stored and compared: {kind: array of raw words}"""
    out = {"g": g.view(np.uint32), "s": s.view(np.uint64)}
    if p is not None:
        assert p.shape == (K.N_PARAMS,)
        out["p"] = p[:K.ACTOR_PARAMS].view(np.uint32)
        out["c"] = K.digest(p[K.ACTOR_PARAMS:])
    return out


def order_words(g, s):
    """(dW3, db3, statistics) words: what the moved phase sums over the samples of a group"""
    w = g.view(np.uint32)
    return w[W3_OFF:B3_OFF], w[B3_OFF:K.ACTOR_PARAMS], s.view(np.uint64)


def main():
    out = {}
    for k, v in zip(K.PARAM_NAMES, K.params(PARAM_SEED)):
        out[f"in_params_{k}"] = v
    for name, M, seed, variant in CASES:
        pv, bv = inputs(M, seed, variant)
        if M <= STORE_INPUTS_UP_TO:
            for k, v in zip(K.BATCH_NAMES, bv):
                out[f"in_{name}_{k}"] = v
            for k, v, v0 in zip(K.PARAM_NAMES, pv, K.params(PARAM_SEED)):
                if v.tobytes() != v0.tobytes():
                    out[f"in_{name}_{k}"] = v
        for path in PATHS:
            g, s, p = run_arrays(pv, bv, path)
            K.record(out, name, path, words(g, s, p))
            print(name, M, path, "finite grads", int(np.isfinite(g).sum()), "/", g.size, "grad |max|", float(np.nanmax(np.abs(g))) if
                  np.isfinite(g).any() else float("nan"), "stats", s.tolist(), flush=True)
        if variant in FINITE:
            assert np.all(np.isfinite(out[f"g_{name}_grad"].view(np.float32))), name
            if M > 1:
                g, s, _ = run_arrays(pv, reversed_groups(bv), "grad")
                fwd = order_words(out[f"g_{name}_grad"].view(np.float32), out[f"s_{name}_grad"].view(np.float64))
                n = [int((a != b).sum()) for a, b in zip(order_words(g, s), fwd)]
                out[f"rev_{name}"] = np.array(n, dtype=np.int64)
                print("   ", name, "rows of every group reversed: dW3 / db3 / statistics words that differ", n, flush=True)
                if M >= REV_ASSERT_FROM:
                    assert all(v > 0 for v in n), (name, n)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
