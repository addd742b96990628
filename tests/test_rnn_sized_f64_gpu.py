"""The sized RAD-A2C kernels (csrc/rs_rnn_sized.hip) against the project's modules in float64 on the CPU, at every GRU tier edge
(1, 2, 7, 8, 9, 15 / 16 / 17, 31 / 32 / 33, 47 / 48 / 49, 63, 64) and head widths at their edges (2, 4, 63, 64 units, 8k + 1 units:
one real unit in the last 8-unit block): the policy step, the GRU sequence with its back-propagation, the heads-loss and one whole
a2c_losses pass.  Tolerances: tests/_f64_ref.py's error model; each test names the terms its constants cover."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GRID = R.head_grid()


def _agent(hid, pol, val, seed=1):
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    torch.manual_seed(seed * 1000 + hid * 64 + pol + val)
    ag = RNNAgentPPO(id=0, seed=1, actor_critic_args=R.rnn_args(hid, pol, val))
    with torch.no_grad():
        for p in ag.agent.pi.parameters():
            p.mul_(1.7)                                        # livelier gates than the default initialisation
    assert ag.agent.sized_policy
    return ag


@pytest.mark.parametrize("hid", R.HIDS)
def test_sized_step_matches_float64(hid):
    """rs_rnn_sized_step against RNNModelActorCritic.policy_step in float64, N = 1, 63, 64, 65, 1000 (a partial wave, one full wave,
    one lane into a second).  h': the gate pre-activations are sums of 13 + hid + 1 <= 78 products (<= ~9 u of the sum of |terms| in
    expectation), each gate a sigm / tanh_ of them (rcp + exp2 + argument scaling: <= ~4 u + u |x|), h' = (1 - z) n + z h with |h'| < 1:
    ~1e-6 absolute; held to rtol 1e-5, atol 2e-6.  logits / value: a second tanh_ layer (<= 64 units) and a dot product of <= 64
    products: rtol 1e-5, atol 5e-6.  (These are the bounds of the float32-torch check of the same outputs, test_rnn_sized_gpu.)
    The action and logp: R.check_draw.  Then the masked value-only form: the masked envs' values, nothing else written; an all-zero mask
    writes nothing at all."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for pol, val in GRID[hid]:
        ag = _agent(hid, pol, val)
        ac64 = R.f64(ag.agent)
        w = ag.policy_weights()
        for N in (1, 63, 64, 65, 1000):
            key = (hid, pol, val, N)
            g = torch.Generator().manual_seed(N * 7 + pol)
            x = torch.randn(N, 11, generator=g)
            loc = torch.rand(N, 2, generator=g)
            h = (torch.rand(N, hid, generator=g) * 2 - 1) * torch.tensor([0.0, 0.3, 1.0])[torch.randint(0, 3, (N, 1), generator=g)]
            u = torch.rand(N, generator=g)
            with torch.no_grad():
                lg64, v64, h64 = ac64.policy_step(x.double(), loc.double(), h.double())
            act64, lp64, cdf64 = R.draw_f64(lg64, u)
            xc, lc, uc = x.cuda(), loc.cuda(), u.cuda()
            hk = h.cuda()
            logits = torch.full((N, 8), 7.0, device="cuda"); v = torch.full((N,), 7.0, device="cuda"); lp = torch.full((N,), 7.0, device="cuda")
            act = torch.full((N,), -1, dtype=torch.int64, device="cuda")
            ag.policy_step_hip(xc, lc, hk, u=uc, h_out=hk, logits=logits, value=v, act=act, logp=lp)
            R.close(hk, h64, f"h' {key}", rtol=1e-5, noise=0.0, tiny=2e-6)
            R.close(logits, lg64, f"logits {key}", rtol=1e-5, noise=0.0, tiny=5e-6)
            R.close(v, v64, f"value {key}", rtol=1e-5, noise=0.0, tiny=5e-6)
            R.check_draw(act, lp, act64, lp64, cdf64, u, str(key))
            # the masked value-only form (the bootstrap round): mask drawn, then all zero
            for m in ((torch.rand(N, generator=g) < 0.4).to(torch.uint8), torch.zeros(N, dtype=torch.uint8)):
                mc = m.cuda()
                hb = h.cuda(); vb = torch.full((N,), 7.0, device="cuda")
                _lib.check(lib.rs_rnn_sized_step(w.data_ptr(), hid, pol, val, xc.data_ptr(), 11, lc.data_ptr(), 2, hb.data_ptr(), None, 1, None,
                                                 None, vb.data_ptr(), None, None, None, 1, mc.data_ptr(), N, st), "masked step")
                torch.cuda.synchronize()
                mb = m.bool()
                R.close(vb.cpu()[mb], v64[mb], f"masked value {key}", rtol=1e-5, noise=0.0, tiny=5e-6)
                assert bool((vb.cpu()[~mb] == 7.0).all()) and torch.equal(hb.cpu(), h), key


@pytest.mark.parametrize("hid", R.HIDS)
def test_sized_gru_sequence_matches_float64(hid):
    """GRUSequenceSized (rs_gru_sized_forward / _backward) against torch.nn.GRU in float64 with autograd, L = 1, 120 (the reference's
    episode length), E = 1, 64, 65, 333, h0 of scale 0, 0.3 and 1 mixed per episode, the loss a random-weighted sum of the outputs.
    States: a step's error (see test_sized_step_matches_float64: ~1e-6) is carried on through z h with |z| < 1 and through W_hh into
    the gates; over 120 steps it stays within rtol 1e-5, atol 2e-6 of the state scale (the float32 check of the same states:
    rtol 1e-4, atol 1e-5).  Gradients, per gate block (the r, z and n rows of each tensor separately, each against its own largest
    element): a sum over L E <= 40 000 per-sample terms (~sqrt(n) u ~ 1.2e-5 of the sum of |terms|, which is ~the block's scale when
    the dL/dgate signs are mixed) on top of per-term errors of the back-propagated dL/dh (~1e-6 relative, growing with the steps they
    travel): rtol 1e-4, atol 5e-5 of the block's scale, 20x tighter than the 1e-3 of the float32 check.  A saturated gate is the one
    exception to a block's own scale: 1 - n^2, z (1 - z) and r (1 - r) are formed from float32 gates with an absolute error of ~2 u, so
    where tanh_ / sigm round to +-1 / 1 (|pre-activation| > ~9 / ~17) the float32 derivative is 0 and the float64 one ~1e-7; a block
    whose every sample saturates (hid 1, one episode) has float64 gradients of ~1e-9 that float32 cannot resolve.  Hence a floor of
    2e-6 of the largest gradient element over the four tensors: ~30 u, far below any mix-up between gate blocks."""
    from radiation_ppo_amd.rada2c import GRUSequenceSized
    torch.manual_seed(hid)
    gru = torch.nn.GRU(13, hid, 1)
    with torch.no_grad():
        for p in gru.parameters():
            p.mul_(1.7)
    gru64 = R.f64(gru)
    gru = gru.cuda()
    for L in (1, 120):
        for E in (1, 64, 65, 333):
            key = (hid, L, E)
            g = torch.Generator().manual_seed(L * 1000 + E)
            x = torch.randn(L, E, 13, generator=g)
            h0 = (torch.rand(E, hid, generator=g) * 2 - 1) * torch.tensor([0.0, 0.3, 1.0])[torch.randint(0, 3, (E, 1), generator=g)]
            wgt = torch.randn(L, E, hid, generator=g) * (torch.rand(L, E, 1, generator=g) < 0.7)
            gru64.zero_grad()
            ref, _ = gru64(x.double(), h0.double().unsqueeze(0))
            (ref * wgt.double()).sum().backward()
            gru.zero_grad()
            got = GRUSequenceSized.apply(x.cuda(), h0.cuda(), gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
            R.close(got, ref, f"gru states {key}", rtol=1e-5, noise=2e-6)
            (got * wgt.cuda()).sum().backward()
            names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
            floor = 2e-6 * max(float(getattr(gru64, n).grad.abs().max()) for n in names)
            for name in names:
                a, b = getattr(gru, name).grad.cpu(), getattr(gru64, name).grad
                for gi, gate in enumerate("rzn"):
                    rows = slice(gi * hid, (gi + 1) * hid)
                    R.close(a[rows], b[rows], f"gru grad {name}[{gate}] {key}", rtol=1e-4, noise=5e-5, tiny=floor)


def _heads_inputs(ac64, hid, S, seed, clip):
    g = torch.Generator().manual_seed(seed)
    hs = torch.rand(S, hid, generator=g) * 2 - 1
    act = torch.randint(0, 8, (S,), generator=g)
    adv, ret = torch.randn(S, generator=g), torch.randn(S, generator=g)
    wt = torch.rand(S, generator=g) / S * (torch.rand(S, generator=g) >= 0.1)          # ~10 % of the samples with weight 0
    with torch.no_grad():
        lg, _ = ac64.heads(hs.double())
        lp64 = torch.log_softmax(lg, dim=-1).gather(-1, act.unsqueeze(-1)).squeeze(-1)
    lpo = (lp64 - torch.log(R.target_ratios(S, g, clip))).float()
    return hs, act, adv, ret, lpo, wt


@pytest.mark.parametrize("hid", R.HIDS)
def test_sized_heads_loss_matches_float64(hid):
    """HeadsLossSized (rs_a2c_sized_heads_loss + the two-step GEMM reductions) against the library branch of a2c_losses written out
    in float64 (R.heads_loss_f64, vf = 0.01), S = 1, 63, 64, 65, 1024, 3 * 1024 + 17 (the 1024s run the row-slab reduction of
    _two_step), ratios below, inside and above the clip range with a margin of 0.02 from its ends, ~10 % of the weights 0.
    Statistics and the loss: per-sample terms within ~1e-6 relative (heads as in the step test, then expf / logf: a few u), summed in
    float32 over a wave (6 rounding levels: <= 6 u = 3.6e-7 of the sum of |terms|) and in float64 across waves: 5e-6 of the sum of the
    absolute terms (R.heads_loss_f64's mags), and never more than the float32 check of the same statistics allows (rtol 2e-5,
    atol 1e-7): each statistic is held to the smaller of the two.  A statistic without cancellation (entropy, weight sum) is its own
    sum of magnitudes, so the first bound is rtol 5e-6 there; the clip fraction takes the same branches: no ratio is within 0.02 of a
    clip end.
    dL/dhs: per sample, a back-propagation through two layers of <= 64 units: rtol 1e-5, atol 1e-5 of the tensor's scale.  Parameter
    gradients: a sum over S samples of per-sample products on top of that: rtol 1e-4, atol 2e-5 of each tensor's scale (the float32
    check at the default widths: rtol 1e-4, atol 1e-5 kernel against kernel; against torch in the whole update: 1e-4)."""
    from radiation_ppo_amd.rada2c import HeadsLossSized, pack_sized_policy_weights
    clip, vf = 0.2, 0.01
    for pol, val in GRID[hid]:
        ag = _agent(hid, pol, val, seed=2)
        ac64 = R.f64(ag.agent)
        params = R.heads_params(ag.agent)
        params64 = R.heads_params(ac64)
        w = pack_sized_policy_weights(ag.agent)
        for S in (1, 63, 64, 65, 1024, 3 * 1024 + 17):
            key = (hid, pol, val, S)
            hs, act, adv, ret, lpo, wt = _heads_inputs(ac64, hid, S, seed=S + 31 * pol + val, clip=clip)
            hx = hs.cuda().requires_grad_(True)
            c = lambda t: t.cuda().contiguous()
            loss, stt = HeadsLossSized.apply(hx, *params, w, c(act), c(adv), c(ret), c(lpo), c(wt), clip, vf)
            gr = torch.autograd.grad(loss, [hx] + params)
            h64 = hs.double().requires_grad_(True)
            loss64, st64, mags = R.heads_loss_f64(ac64, h64, act, adv.double(), ret.double(), lpo.double(), wt.double(), clip, vf)
            gr64 = torch.autograd.grad(loss64, [h64] + params64)
            # each statistic within the smaller of the float32 check's bound (rtol 2e-5, atol 1e-7) and 5e-6 of its magnitudes
            bound = lambda ref, mag: min(2e-5 * abs(float(ref)) + 1e-7, 5e-6 * float(mag)) + 1e-12
            R.close(loss.reshape(1), loss64.detach().reshape(1), f"heads loss {key}", rtol=0.0, noise=0.0, tiny=bound(loss64, mags[6]))
            for q, nm in enumerate(("kl", "entropy", "clipfrac", "value loss", "surrogate", "weight sum")):
                R.close(stt[q].reshape(1), st64[q].reshape(1), f"heads stat {nm} {key}", rtol=0.0, noise=0.0, tiny=bound(st64[q], mags[q]))
            R.close(gr[0], gr64[0], f"heads dL/dhs {key}", rtol=1e-5, noise=1e-5)
            for nm, a, b in zip(("W1", "b1", "W2", "b2", "V1", "vb1", "V2", "vb2"), gr[1:], gr64[1:]):
                R.close(a, b, f"heads grad {nm} {key}", rtol=1e-4, noise=2e-5)


@pytest.mark.parametrize("hid,pol,val", [(9, 64, 2), (31, 8, 17), (40, 9, 57), (49, 63, 33)])
def test_sized_a2c_losses_match_float64(hid, pol, val):
    """One RNNAgentPPO.a2c_losses pass on the sized path (GRUSequenceSized + HeadsLossSized, the collector's packed weights) against
    the same pass of the agent's float64 twin on the CPU (nn.GRU and the library heads branch), one width per tier, the PFGRU
    locations given (the same for both): all seven statistics and every pi gradient.  logp_old is set from the float64 log-probabilities
    so that the ratios fall below, inside and above the clip range with a margin.  Tolerances: the GRU test's states feed the heads
    test's per-sample terms; statistics rtol 2e-5, atol 1e-7 (the float32 check of the same pass), gradients rtol 1e-4, atol 5e-5 of
    each tensor's scale (the float32 check: 1e-4 of the scale, with rtol 1e-3)."""
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    ag = _agent(hid, pol, val, seed=3)
    ag.agent.train()
    B = R.make_batch(19 + hid, T=60, N=150, device="cuda")
    L, E = B.X.shape[0], B.X.shape[1]
    g = torch.Generator().manual_seed(hid)
    loc = torch.rand(L, E, 2, generator=g)
    h0 = (torch.rand(E, hid, generator=g) * 2 - 1) / np.sqrt(hid)
    ag64 = RNNAgentPPO(id=0, seed=1, actor_critic_args=R.rnn_args(hid, pol, val), device="cpu")
    ag64.agent.load_state_dict({k: v.cpu() for k, v in ag.agent.state_dict().items()})
    ag64.agent.double().train()
    B64 = R.batch_to(B, "cpu", torch.float64)
    lp64 = R.chain_logp_f64(ag64.agent, B64.X, loc.double(), h0.double(), B.act)
    B.logp.copy_((lp64 - torch.log(R.target_ratios(L * E, g).view(L, E))).float())
    B64.logp = B.logp.double().cpu()
    ag.pi_optimizer.zero_grad(set_to_none=True)
    loss, st = ag.a2c_losses(B, slice(0, E), R.GruH0(h0.cuda()), loc=loc.cuda())
    loss.backward()
    loss64, st64 = ag64.a2c_losses(B64, slice(0, E), R.GruH0(h0.double()), loc=loc.double())
    loss64.backward()
    # both clip sides are hit: the float64 ratios are the targets (up to the float32 rounding of logp_old), each side >1 % of the weight
    ratio64 = torch.exp(lp64 - B64.logp)
    w64 = B64.w.cpu()
    for side in (ratio64 < 1 - ag.clip_ratio, ratio64 > 1 + ag.clip_ratio):
        assert float((w64 * side).sum()) > 0.01 * float(w64.sum())
    key = (hid, pol, val)
    for q in range(7):
        R.close(st[q].reshape(1), st64[q].reshape(1), f"chain stat {q} {key}", rtol=2e-5, noise=0.0, tiny=1e-7)
    p64 = dict(ag64.agent.pi.named_parameters())
    for k, p in ag.agent.pi.named_parameters():
        R.close(p.grad, p64[k].grad, f"chain grad {k} {key}", rtol=1e-4, noise=5e-5)
