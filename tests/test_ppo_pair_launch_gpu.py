"""The pair launch of an Adam step (rs_ppo_update_step: the actor's and the critic's gradient pass as ONE grid of twice the workgroups,
rs_ppo_grad2_pair_kernel) against the form it replaces, one launch per network (RS_PPO_SPLIT_GRAD=1): same batch, same starting
networks and state.  Gradients, statistics, Adam moments, update state and parameters must be equal bit for bit after every step.

M = 33 is one full and one partial sample group (every other wave works on clamped rows with weight 0), M = 4096 + 17 leaves most
waves without a group, M = 70 001 has more groups (2188) than a network has waves (2048): some waves take a second trip, the others a
clamped one."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 1e30
PLANS = {
    "three_steps": [BIG, BIG, BIG],
    "kl_stop": [BIG, 1e-30, BIG],          # the second step trips the stop (no |KL| estimate is that small), the third is a no-op
}


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("M", [33, 4096 + 17, 70_001])
def test_pair_launch_bitwise_equals_one_launch_per_network(monkeypatch, M, plan):
    from radiation_ppo_amd.ppo import FFActorCritic, FusedPPOGrad
    torch.manual_seed(5)
    ac_a = FFActorCritic().cuda()
    ac_b = copy.deepcopy(ac_a)
    fa, fb = FusedPPOGrad(ac_a), FusedPPOGrad(ac_b)
    b = K.torch_batch(M, 4321)
    lr = 3e-3
    fa.begin_update(); fb.begin_update()
    for k, thr in enumerate(PLANS[plan]):
        monkeypatch.setenv("RS_PPO_SPLIT_GRAD", "1")
        fa.step(*b, 0.2, 0.1, lr=lr, kl_threshold=thr)
        monkeypatch.delenv("RS_PPO_SPLIT_GRAD")
        fb.step(*b, 0.2, 0.1, lr=lr, kl_threshold=thr)
        xa, xb = K.state_bytes(fa), K.state_bytes(fb)
        for name in xa:
            assert torch.equal(xa[name], xb[name]), (k, name)
    iters, stopped, adam_step, last = fb.read_state()
    if plan == "three_steps":
        assert (iters, stopped, adam_step) == (3, 0, 3)
        assert fb.grads.any().item() and all(x == x for x in last)
    else:
        assert (iters, stopped, adam_step) == (2, 1, 1)
        assert not fb.bucket.any().item() and not fb.stats.any().item()       # after the stop: zeros are published
    # the steps moved the parameters at all (the comparison above is not between two untouched copies)
    torch.manual_seed(5)
    fresh = FFActorCritic().cuda()
    assert not torch.equal(fresh.critic[2].weight, ac_b.critic[2].weight)
    assert not torch.equal(fresh.actor[2].weight, ac_b.actor[2].weight)
