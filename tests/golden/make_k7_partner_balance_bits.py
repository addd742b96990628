"""Bit-identity fixture of K7 (rs_ppo_grad2_body, both networks), recorded before the waves of a SIMD began to trade issue priority by
progress (rs_ppo_grad2.hpp, RS_K7_PRIO).  Priority moves issue slots between the two waves of a SIMD and nothing else: which groups a
wave sums, and in which order, stays, so every word must stay.  The cases are chosen by their trip counts (2048 waves, 32 samples
per group, 65 536 samples per trip of the whole grid):

  m1        M = 1        one wave has a real group, 2047 run one clamped trip
  m65553    M = 65 553   two trips, the second with one real (ragged) group
  m196609   M = 196 609  four trips, three full and one nearly empty: priorities flip several times, partners end on different work
  m196608   M = 196 608  three trips, an odd count

Inputs: the seeded generators of tests/_k7_bits.py, then all eight actions in every group of 32, |adv| = 10^U(-4, 2) with either sign,
every seventh row at weight 0 (row 10 at -0.0).  Nothing but seeds is stored.  Every case runs three ways: rs_ppo_grad, and
rs_ppo_update_step (lr = 1e-3, first Adam step) as the pair launch and as one launch per network (RS_PPO_SPLIT_GRAD=1).  Stored as raw
bits: the whole gradient bucket (10 441 gradients and the (hi, lo) statistics tail), the five statistics, the 10 441 parameters after
the step, and the Adam moments m and v after the step as SHA-256 digests (in full they would double the file).  A path's result is
stored on its own only where it differs from the first path's.

  seq       six rs_ppo_update_step calls on M = 196 609 that run into the KL stop.  Most advantages are negative here, so the taken
            actions lose probability and the KL statistic moves a lot from step to step; the recorder first runs the six steps
            without a threshold at a few learning rates, takes the one whose KL exceeds all its earlier values latest, puts the
            threshold between (stored: lr, threshold, the call that stops) and records the run with it.  Stored: the five statistics and the update state after every call, and after the sixth the
            gradient bucket, the parameters, m and v in full.  The calls after the stop are no-ops.

params(), batch() and run() live in tests/_k7_bits.py, which every bit-identity suite shares.

    python tests/golden/make_k7_partner_balance_bits.py [OUT.npz]   # on the MI355X, with the library whose results are the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "k7_partner_balance_bits.npz")

sys.path.insert(0, os.path.dirname(HERE))
import _k7_bits as K  # noqa: E402

# (name, M, batch seed)
CASES = [("m1", 1, 71), ("m65553", 65536 + 17, 72), ("m196609", 3 * 65536 + 1, 73), ("m196608", 3 * 65536, 74)]
PATHS = ("grad", "pair", "split")
KINDS = ("g", "s", "p", "m", "v")        # what is stored: the bucket, statistics, parameters after Adam, digests of Adam's m and v
PARAM_SEED = 70
LR = 1e-3
SEQ_M, SEQ_SEED, SEQ_STEPS = 3 * 65536 + 1, 75, 6
SEQ_LRS = (3e-2, 2e-2, 5e-2, 1.5e-2, 1e-2)


def inputs(M: int, seed: int, negative: float = 0.5):
    """(12 parameter arrays, 6 batch arrays); negative: the share of rows with a negative advantage."""
    p = K.params(PARAM_SEED)
    b = list(K.batch(M, seed))
    rng = np.random.default_rng(2000 + seed)
    i = np.arange(M)
    b[1] = ((3 * i + i // 8) % 8).astype(np.int64)
    for g0 in range(0, min(M, 4096) - 31, 32):
        assert np.array_equal(np.bincount(b[1][g0:g0 + 32], minlength=8), np.full(8, 4))
    b[2] = (np.where(rng.random(M) < negative, -1.0, 1.0) * 10.0 ** rng.uniform(-4.0, 2.0, M)).astype(np.float32)
    b[5][i % 7 == 3] = 0.0
    if M > 10:
        b[5][10] = -0.0
    return p, b


def run_arrays(pv, b, path: str):
    """{kind: float array}: g bucket [10457], s statistics float64 [5] and, for the update step, p parameters, m, v [10441] each.
    b: the batch on the device (K.device_batch), built once per case and reused across the paths."""
    return K.run(pv, b, path, lr=LR)


def words(r):
    """what is stored and compared: {kind: raw words}; the Adam moments as digests"""
    assert r["g"].shape == (K.BUCKET,) and r["s"].shape == (5,)
    out = {"g": r["g"].view(np.uint32), "s": r["s"].view(np.uint64)}
    if "p" in r:
        assert r["p"].shape == r["m"].shape == r["v"].shape == (K.N_PARAMS,)
        out.update(p=r["p"].view(np.uint32), m=K.digest(r["m"]), v=K.digest(r["v"]))
    return out


def run_sequence(pv, b, lr: float, thr: float, path: str = "pair"):
    """six update steps; ({kind: array} after the sixth, statistics [6][5] float64, update state int32 [6][3] = adam_step, stopped, iters)"""
    import torch
    ac, ps, f = K.load(pv)
    stats, states = [], []
    with K.split_grad(path):
        f.begin_update()
        f.bind(*b, K.CLIP, K.ALPHA, K.VF)
        for _ in range(SEQ_STEPS):
            f.step_bound(lr, thr)
            stats.append(f.stats.cpu().numpy().copy())
            states.append(f.state_i32[:3].cpu().numpy().copy())
        torch.cuda.synchronize()
    assert K.SPLIT_ENV not in os.environ
    return K.read_back(ps, f), np.stack(stats), np.stack(states)


def seq_words(fin, stats, states):
    return {"g": fin["g"].view(np.uint32), "p": fin["p"].view(np.uint32), "m": fin["m"].view(np.uint32), "v": fin["v"].view(np.uint32),
            "stats": stats.view(np.uint64), "state": states.astype(np.int32)}


def main():
    out = {}
    for name, M, seed in CASES:
        pv, bv = inputs(M, seed)
        b = K.device_batch(bv)
        for path in PATHS:
            r = run_arrays(pv, b, path)
            K.record(out, name, path, words(r))
            assert np.all(np.isfinite(r["g"])) and np.all(np.isfinite(r["s"])), name
            print(name, M, path, "grad |max|", float(np.abs(r["g"][:K.N_PARAMS]).max()), "stats", r["s"].tolist(), flush=True)
    # the sequence: the learning rate and a threshold with which the loop stops as late as it can between its second and fifth call
    pv, bv = inputs(SEQ_M, SEQ_SEED, negative=0.85)
    b = K.device_batch(bv)
    best = None
    for lr_try in SEQ_LRS:
        _, stats, states = run_sequence(pv, b, lr_try, 1e30)
        kl_try = stats[:, 0]
        print("seq lr", lr_try, "kl without a threshold", kl_try.tolist(), flush=True)
        assert states[-1].tolist() == [SEQ_STEPS, 0, SEQ_STEPS]
        j_try = max((j for j in range(1, 5) if kl_try[j] > kl_try[:j].max()), default=None)
        if j_try is not None and (best is None or j_try > best[0]):
            best = (j_try, lr_try, kl_try)
    assert best is not None, "no call of the sequence exceeds the KL of all calls before it"
    j, lr, kl = best
    thr = float(np.float32((kl[:j].max() + kl[j]) / 2))
    assert kl[:j].max() < thr <= kl[j]
    fin, stats, states = run_sequence(pv, b, lr, thr)
    print("seq lr", lr, "threshold", thr, "stops at call", j, "states", states.tolist(), flush=True)
    assert states[j].tolist() == [j, 1, j + 1] and all(s.tolist() == states[j].tolist() for s in states[j:])
    for k, v in seq_words(fin, stats, states).items():
        out[f"seq_{k}"] = v
    out["seq_lr"], out["seq_thr"], out["seq_stop"] = np.float64(lr), np.float64(thr), np.int64(j)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 700000


if __name__ == "__main__":
    main()
