"""K7's two waves per SIMD trade issue priority by progress (rs_ppo_grad2.hpp, RS_K7_PRIO): every wave publishes its trip index in an
LDS word, reads its partner's once per trip and runs at priority 1 while it is behind.  That moves issue slots between the partners
and must move nothing else.  tests/golden/k7_partner_balance_bits.npz holds, as recorded from the library before the change
(tests/golden/make_k7_partner_balance_bits.py, which also builds the inputs and describes the cases), the gradient bucket, the five
statistics, the parameters and the Adam moments after a step for M = 1, 65 553, 196 609 and 196 608 -- one, two, four and three trips
per wave -- through rs_ppo_grad, the pair launch and one launch per network, and a sequence of six update steps that runs into the
KL stop.  Equality is on the raw bits (the moments of the single steps: on their SHA-256 digests).  The priority decisions race by
design; the last test runs the same calls five times in one process and wants every output equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu
MK = K.maker("make_k7_partner_balance_bits")


@pytest.fixture(scope="module")
def golden():
    return K.golden("k7_partner_balance_bits.npz")


@pytest.fixture(scope="module")
def batches():
    """the inputs of every case, built once and left on the device: {name: (parameters, device batch)}"""
    out = {}
    for name, M, seed in MK.CASES:
        pv, bv = MK.inputs(M, seed)
        out[name] = (pv, K.device_batch(bv))
    pv, bv = MK.inputs(MK.SEQ_M, MK.SEQ_SEED, negative=0.85)
    out["seq"] = (pv, K.device_batch(bv))
    return out


def test_inputs_have_what_the_cases_need(batches):
    for name, M, seed in MK.CASES:
        _, b = batches[name]
        act, adv, w = b[1].cpu().numpy(), b[2].cpu().numpy(), b[5].cpu().numpy()
        assert act.shape == (M,)
        if M >= 32:
            assert sorted(set(act.tolist())) == list(range(8))
            assert np.log10(np.abs(adv).max() / np.abs(adv).min()) > 5 and (adv > 0).any() and (adv < 0).any()
            assert (w == 0).sum() >= M // 7 and (w > 0).sum() > M // 2
        else:
            assert w[0] > 0


@pytest.mark.parametrize("path", MK.PATHS)
@pytest.mark.parametrize("name,M,seed", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_k7_partner_balance_bitwise(golden, batches, name, M, seed, path):
    pv, b = batches[name]
    r = MK.run_arrays(pv, b, path)
    got, want = MK.words(r), K.expected(golden, name, path, MK.KINDS)
    print(name, path, "statistics", r["s"].tolist())
    assert sorted(got) == sorted(want)
    assert np.all(np.isfinite(r["g"])) and np.all(np.isfinite(r["s"])) and np.any(r["g"][:K.N_PARAMS] != 0)
    for kind, what in (("g", "gradient bucket"), ("s", "statistics"), ("p", "parameters after Adam"), ("m", "digest of Adam's m"),
                       ("v", "digest of Adam's v")):
        if kind in want:
            K.same_bits(got[kind], want[kind], (name, path, what))


@pytest.mark.parametrize("path", ("pair", "split"))
def test_six_steps_into_the_kl_stop(golden, batches, path):
    pv, b = batches["seq"]
    lr, thr, j = float(golden["seq_lr"]), float(golden["seq_thr"]), int(golden["seq_stop"])
    fin, stats, states = MK.run_sequence(pv, b, lr, thr, path)
    print("kl per call", stats[:, 0].tolist(), "states", states.tolist(), "recorded stop at call", j)
    assert 1 <= j <= 4 and states[j].tolist() == [j, 1, j + 1]
    for k in range(j, MK.SEQ_STEPS):                      # the calls after the stop are no-ops
        assert states[k].tolist() == states[j].tolist()
    got = MK.seq_words(fin, stats, states)
    for kind in ("state", "stats", "g", "p", "m", "v"):
        K.same_bits(got[kind], golden[f"seq_{kind}"], ("seq", path, kind))


def test_five_runs_agree(batches):
    """M = 196 609 (four trips): rs_ppo_grad and the pair-launch update step, five times each from the same state"""
    import torch
    pv, b = batches["m196609"]
    for path in ("grad", "pair"):
        runs = [MK.run_arrays(pv, b, path) for _ in range(5)]
        for r in runs[1:]:
            assert sorted(r) == sorted(runs[0])
            for kind in r:
                assert torch.equal(torch.from_numpy(r[kind].view(np.uint8)), torch.from_numpy(runs[0][kind].view(np.uint8))), (path, kind)
