"""The fused single-GPU tail of an Adam step (rs_ppo_update_step: slab reduction + Adam + state update in one launch behind the two
gradient kernels) against the three-kernel tail it replaces (rs_ppo_grad's reduce kernel, then rs_adam_step's apply and commit
kernels): same batch, same starting networks and state, several steps -- taken steps, the step at which the KL threshold trips, a step
after the stop, and the first step of the next update.  Everything either path leaves must be equal bit for bit."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M", [4096 * 3 + 17, 200_000])
def test_fused_tail_bitwise_equals_three_kernel_tail(M):
    from radiation_ppo_amd.ppo import FFActorCritic, FusedPPOGrad
    torch.manual_seed(7)
    ac_a = FFActorCritic().cuda()
    ac_b = copy.deepcopy(ac_a)
    fa, fb = FusedPPOGrad(ac_a), FusedPPOGrad(ac_b)
    b = K.torch_batch(M, 1234)
    lr, big = 3e-3, 1e30
    # (threshold, begin a new update first): three taken steps, the trip (no KL is below -1), two steps after the stop, then the next update
    plan = [(big, True), (big, False), (big, False), (-1.0, False), (big, False), (big, False), (big, True), (big, False)]
    seen_stop = seen_zero = False
    for k, (thr, begin) in enumerate(plan):
        if begin:
            fa.begin_update(); fb.begin_update()
        fa(*b, 0.2, 0.1, use_stop_flag=True)
        fa.adam_step(lr, thr)
        fb.step(*b, 0.2, 0.1, lr=lr, kl_threshold=thr)
        xa, xb = K.state_bytes(fa), K.state_bytes(fb)
        for name in xa:
            assert torch.equal(xa[name], xb[name]), (k, name)
        iters, stopped, adam_step, last = fb.read_state()
        if k == 2:
            assert (iters, stopped, adam_step) == (3, 0, 3)
        if k == 3:
            assert (iters, stopped, adam_step) == (4, 1, 3) and fb.stats[0].item() == last[0]
            seen_stop = True
        if k in (4, 5):
            # after the stop: zeros are published, the state is frozen
            assert (iters, stopped, adam_step) == (4, 1, 3)
            assert not fb.bucket.any().item() and not fb.stats.any().item()
            seen_zero = True
        if k == 7:
            assert (iters, stopped, adam_step) == (2, 0, 5)
    assert seen_stop and seen_zero
    # the steps moved the parameters at all (the comparison above is not between two untouched copies)
    torch.manual_seed(7)
    fresh = FFActorCritic().cuda()
    assert not torch.equal(fresh.actor[2].weight, ac_b.actor[2].weight)


def test_update_loop_takes_the_fused_tail_on_one_rank(monkeypatch):
    """VecAgentPPO's update: the fused and the split loop leave the same networks and the same result."""
    from radiation_ppo_amd.ppo import VecAgentPPO
    b = K.torch_batch(50_000, 1234)
    res, params = [], []
    for split in (False, True):
        if split:
            monkeypatch.setenv("RS_PPO_SPLIT_TAIL", "1")
        torch.manual_seed(11)
        ag = VecAgentPPO(id=0, alpha=0.1, train_pi_iters=6, actor_learning_rate=3e-3, target_kl=0.002, device="cuda:0")
        res.append(ag.update_agent(*b))
        params.append(torch.cat([p.data.reshape(-1) for p in ag.agent.parameters()]).cpu())
    assert res[0] == res[1]
    assert torch.equal(params[0].view(torch.int32), params[1].view(torch.int32))
