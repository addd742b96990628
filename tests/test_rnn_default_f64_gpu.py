"""The default-width RAD-A2C kernels -- K14 (csrc/rs_rnn_policy.hip: rs_rnn_policy_step, rs_rnn_policy_step_rows), K12 (csrc/rs_gru.hip:
rs_gru_forward / _backward behind GRUSequence) and K15 (rs_a2c_heads_loss behind HeadsLoss): GRU 24, heads 32 / 32, what the product
runs at the reference's layer sizes -- against the project's modules in float64 on the CPU.  test_rnn_sized_f64_gpu.py test for test,
with ITS constants unchanged: they come from tests/_f64_ref.py's error model for sums of at most 13 + 64 + 1 terms and heads of at
most 64 units, and 24 / 32 / 32 lies inside that."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402
from test_rnn_sized_f64_gpu import _heads_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

HID = 24


def _agent(seed=1):
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    torch.manual_seed(seed * 1000 + 7)
    ag = RNNAgentPPO(id=0, seed=1)
    with torch.no_grad():
        for p in ag.agent.pi.parameters():
            p.mul_(1.7)                                        # livelier gates than the default initialisation
    assert ag.agent.fused_policy
    return ag


def _step_inputs(N, g):
    x = torch.randn(N, 11, generator=g)
    loc = torch.rand(N, 2, generator=g)
    h = (torch.rand(N, HID, generator=g) * 2 - 1) * torch.tensor([0.0, 0.3, 1.0])[torch.randint(0, 3, (N, 1), generator=g)]
    return x, loc, h, torch.rand(N, generator=g)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_default_step_matches_float64(N):
    """K14 (rs_rnn_policy_step through policy_step_hip) against RNNModelActorCritic.policy_step in float64, N = 1, 63, 64, 65, 1000 (a
    partial wave, one full wave, one lane into a second), h of scale 0 / 0.3 / 1 mixed per env.  The sized step test's constants,
    unchanged: h' rtol 1e-5, atol 2e-6 (gate sums of 13 + 24 + 1 products, sigm / tanh_ of them, |h'| < 1); logits / value rtol 1e-5,
    atol 5e-6 (a second tanh_ layer of 32 units and a dot product of 32); action and logp by R.check_draw.  Then the value-only
    bootstrap form: the values, nothing else written, h untouched bit for bit."""
    ag = _agent()
    ac64 = R.f64(ag.agent)
    g = torch.Generator().manual_seed(N * 7 + 32)
    x, loc, h, u = _step_inputs(N, g)
    with torch.no_grad():
        lg64, v64, h64 = ac64.policy_step(x.double(), loc.double(), h.double())
    act64, lp64, cdf64 = R.draw_f64(lg64, u)
    xc, lc, uc, hk = x.cuda(), loc.cuda(), u.cuda(), h.cuda()
    logits = torch.full((N, 8), 7.0, device="cuda"); v = torch.full((N,), 7.0, device="cuda"); lp = torch.full((N,), 7.0, device="cuda")
    act = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    ag.policy_step_hip(xc, lc, hk, u=uc, h_out=hk, logits=logits, value=v, act=act, logp=lp)
    R.close(hk, h64, f"K14 h' N={N}", rtol=1e-5, noise=0.0, tiny=2e-6)
    R.close(logits, lg64, f"K14 logits N={N}", rtol=1e-5, noise=0.0, tiny=5e-6)
    R.close(v, v64, f"K14 value N={N}", rtol=1e-5, noise=0.0, tiny=5e-6)
    R.check_draw(act, lp, act64, lp64, cdf64, u, f"K14 N={N}")
    hb, vb = h.cuda(), torch.full((N,), 7.0, device="cuda")
    ag.policy_step_hip(xc, lc, hb, value=vb)
    torch.cuda.synchronize()
    R.close(vb, v64, f"K14 bootstrap value N={N}", rtol=1e-5, noise=0.0, tiny=5e-6)
    assert torch.equal(hb.cpu(), h), N


@pytest.mark.parametrize("A", [1, 3])
def test_default_step_rows_match_float64(A):
    """rs_rnn_policy_step_rows through policy_step_rows, as the collector calls it: agent a's rows of [N, A, .] tensors (row strides
    A x 11, A x 2, A), h updated in place, the action once more as int8 at stride A; N = 1, 65, 200.  Same bounds as the step.  With
    a mask, the masked-out envs keep the bits of h, value, action, logp and the int8 action, in the drawing form and in the
    value-only (bootstrap) form, where h keeps its bits everywhere; the other agents' int8 columns are never touched."""
    ag = _agent()
    ac64 = R.f64(ag.agent)
    for N in (1, 65, 200):
        for a in range(A):
            key = (A, N, a)
            g = torch.Generator().manual_seed(N * 13 + A * 5 + a)
            X = torch.randn(N, A, 11, generator=g)
            LOC = torch.rand(N, A, 2, generator=g)
            _, _, h, _ = _step_inputs(N, g)
            U = torch.rand(N, A, generator=g)
            with torch.no_grad():
                lg64, v64, h64 = ac64.policy_step(X[:, a].double(), LOC[:, a].double(), h.double())
            act64, lp64, cdf64 = R.draw_f64(lg64, U[:, a])
            Xc, Lc, Uc = X.cuda(), LOC.cuda(), U.cuda()
            masks = [None, (torch.rand(N, generator=g) < 0.5).to(torch.uint8)]
            if N > 1:
                masks[1][0], masks[1][N - 1] = 1, 0
            for m in masks:
                on = torch.ones(N, dtype=torch.bool) if m is None else m.bool()
                mc = None if m is None else m.cuda()
                hk = h.cuda()
                v = torch.full((N,), 7.0, device="cuda"); lp = torch.full((N,), 7.0, device="cuda")
                act = torch.full((N,), -1, dtype=torch.int64, device="cuda")
                act8 = torch.full((N, A), -3, dtype=torch.int8, device="cuda")
                ag.policy_step_rows(Xc, Lc, hk, Uc, a, v, act=act, logp=lp, act8=act8, mask8=mc)
                torch.cuda.synchronize()
                if bool(on.any()):
                    R.close(hk.cpu()[on], h64[on], f"K14 rows h' {key}", rtol=1e-5, noise=0.0, tiny=2e-6)
                    R.close(v.cpu()[on], v64[on], f"K14 rows value {key}", rtol=1e-5, noise=0.0, tiny=5e-6)
                    R.check_draw(act.cpu()[on], lp.cpu()[on], act64[on], lp64[on], cdf64[on], U[:, a][on], f"K14 rows {key}")
                    assert torch.equal(act8.cpu()[:, a][on].long(), act.cpu()[on])
                off = ~on
                assert torch.equal(hk.cpu()[off], h[off]) and bool((v.cpu()[off] == 7.0).all()) and bool((lp.cpu()[off] == 7.0).all()), key
                assert bool((act.cpu()[off] == -1).all()) and bool((act8.cpu()[:, a][off] == -3).all()), key
                others = [b for b in range(A) if b != a]
                assert bool((act8.cpu()[:, others] == -3).all()), key
                # the bootstrap form: value only
                hb, vb = h.cuda(), torch.full((N,), 7.0, device="cuda")
                ag.policy_step_rows(Xc, Lc, hb, None, a, vb, mask8=mc)
                torch.cuda.synchronize()
                if bool(on.any()):
                    R.close(vb.cpu()[on], v64[on], f"K14 rows bootstrap value {key}", rtol=1e-5, noise=0.0, tiny=5e-6)
                assert bool((vb.cpu()[off] == 7.0).all()) and torch.equal(hb.cpu(), h), key


@pytest.mark.parametrize("L", [1, 120])
def test_default_gru_sequence_matches_float64(L):
    """K12 (GRUSequence: rs_gru_forward / rs_gru_backward) against torch.nn.GRU(13, 24) in float64 with autograd, L = 1, 120 (the
    reference's episode length), E = 1, 64, 65, 333, h0 of scale 0, 0.3 and 1 mixed per episode, the loss a random-weighted sum of the
    outputs with the weights zero on ~30 % of the steps.  The sized sequence test's constants, unchanged: states rtol 1e-5, noise 2e-6
    of the state scale (a step's ~1e-6 error carried through z h and W_hh over up to 120 steps); gradients per gate block (the r, z
    and n rows of each of the four tensors, each against its own largest element) rtol 1e-4, noise 5e-5 (sums over L E <= 40 000
    per-sample terms on top of the back-propagated dL/dh), floor 2e-6 of the largest gradient element over the four tensors (saturated
    gates: 1 - n^2, z (1 - z), r (1 - r) from float32 gates)."""
    from radiation_ppo_amd.rada2c import GRUSequence
    torch.manual_seed(HID)
    gru = torch.nn.GRU(13, HID, 1)
    with torch.no_grad():
        for p in gru.parameters():
            p.mul_(1.7)
    gru64 = R.f64(gru)
    gru = gru.cuda()
    for E in (1, 64, 65, 333):
        key = (L, E)
        g = torch.Generator().manual_seed(L * 1000 + E)
        x = torch.randn(L, E, 13, generator=g)
        h0 = (torch.rand(E, HID, generator=g) * 2 - 1) * torch.tensor([0.0, 0.3, 1.0])[torch.randint(0, 3, (E, 1), generator=g)]
        wgt = torch.randn(L, E, HID, generator=g) * (torch.rand(L, E, 1, generator=g) < 0.7)
        gru64.zero_grad()
        ref, _ = gru64(x.double(), h0.double().unsqueeze(0))
        (ref * wgt.double()).sum().backward()
        gru.zero_grad()
        got = GRUSequence.apply(x.cuda(), h0.cuda(), gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
        R.close(got, ref, f"K12 states {key}", rtol=1e-5, noise=2e-6)
        (got * wgt.cuda()).sum().backward()
        names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
        floor = 2e-6 * max(float(getattr(gru64, n).grad.abs().max()) for n in names)
        for name in names:
            a, b = getattr(gru, name).grad.cpu(), getattr(gru64, name).grad
            for gi, gate in enumerate("rzn"):
                rows = slice(gi * HID, (gi + 1) * HID)
                R.close(a[rows], b[rows], f"K12 grad {name}[{gate}] {key}", rtol=1e-4, noise=5e-5, tiny=floor)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 1024, 3 * 1024 + 17])
def test_default_heads_loss_matches_float64(S):
    """K15 (HeadsLoss: rs_a2c_heads_loss + the two-step GEMM reductions) against the library branch of a2c_losses written out in
    float64 (R.heads_loss_f64, vf = 0.01), S = 1, 63, 64, 65, 1024, 3 * 1024 + 17, ratios from R.target_ratios (below, inside and above
    the clip range, 0.02 from its ends), ~10 % of the weights 0.  test_sized_heads_loss_matches_float64's constants, unchanged: the
    loss and each of the six statistics within the smaller of (rtol 2e-5, atol 1e-7) and 5e-6 of the sum of its absolute per-sample
    terms (mags); dL/dhs rtol 1e-5, atol 1e-5 of the tensor's scale; the eight parameter gradients rtol 1e-4, atol 2e-5 of each
    tensor's scale."""
    from radiation_ppo_amd.rada2c import HeadsLoss, pack_policy_weights
    clip, vf = 0.2, 0.01
    ag = _agent(seed=2)
    ac64 = R.f64(ag.agent)
    params, params64 = R.heads_params(ag.agent), R.heads_params(ac64)
    w = pack_policy_weights(ag.agent)
    hs, act, adv, ret, lpo, wt = _heads_inputs(ac64, HID, S, seed=S + 31 * 32 + 32, clip=clip)
    hx = hs.cuda().requires_grad_(True)
    c = lambda t: t.cuda().contiguous()
    loss, stt = HeadsLoss.apply(hx, *params, w, c(act), c(adv), c(ret), c(lpo), c(wt), clip, vf)
    gr = torch.autograd.grad(loss, [hx] + params)
    h64 = hs.double().requires_grad_(True)
    loss64, st64, mags = R.heads_loss_f64(ac64, h64, act, adv.double(), ret.double(), lpo.double(), wt.double(), clip, vf)
    gr64 = torch.autograd.grad(loss64, [h64] + params64)
    bound = lambda ref, mag: min(2e-5 * abs(float(ref)) + 1e-7, 5e-6 * float(mag)) + 1e-12
    R.close(loss.reshape(1), loss64.detach().reshape(1), f"K15 loss S={S}", rtol=0.0, noise=0.0, tiny=bound(loss64, mags[6]))
    for q, nm in enumerate(("kl", "entropy", "clipfrac", "value loss", "surrogate", "weight sum")):
        R.close(stt[q].reshape(1), st64[q].reshape(1), f"K15 stat {nm} S={S}", rtol=0.0, noise=0.0, tiny=bound(st64[q], mags[q]))
    R.close(gr[0], gr64[0], f"K15 dL/dhs S={S}", rtol=1e-5, noise=1e-5)
    for nm, a, b in zip(("W1", "b1", "W2", "b2", "V1", "vb1", "V2", "vb2"), gr[1:], gr64[1:]):
        R.close(a, b, f"K15 grad {nm} S={S}", rtol=1e-4, noise=2e-5)


def test_default_a2c_losses_match_float64():
    """One RNNAgentPPO.a2c_losses pass on K12 + K15 (the PFGRU locations given, R.GruH0) against the same pass of the agent's float64
    twin on the CPU: all seven statistics and every pi gradient, logp_old set from the float64 log-probabilities so that the ratios
    fall below, inside and above the clip range with a margin; both clip sides carry more than 1 % of the weight.
    test_sized_a2c_losses_match_float64's constants, unchanged: statistics rtol 2e-5, atol 1e-7, gradients rtol 1e-4, noise 5e-5 of
    each tensor's scale."""
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    ag = _agent(seed=3)
    ag.agent.train()
    B = R.make_batch(19 + HID, T=60, N=150, device="cuda")
    L, E = B.X.shape[0], B.X.shape[1]
    g = torch.Generator().manual_seed(HID)
    loc = torch.rand(L, E, 2, generator=g)
    h0 = (torch.rand(E, HID, generator=g) * 2 - 1) / np.sqrt(HID)
    ag64 = RNNAgentPPO(id=0, seed=1, device="cpu")
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
    ratio64 = torch.exp(lp64 - B64.logp)
    w64 = B64.w.cpu()
    for side in (ratio64 < 1 - ag.clip_ratio, ratio64 > 1 + ag.clip_ratio):
        assert float((w64 * side).sum()) > 0.01 * float(w64.sum())
    for q in range(7):
        R.close(st[q].reshape(1), st64[q].reshape(1), f"K12 + K15 chain stat {q}", rtol=2e-5, noise=0.0, tiny=1e-7)
    p64 = dict(ag64.agent.pi.named_parameters())
    for k, p in ag.agent.pi.named_parameters():
        R.close(p.grad, p64[k].grad, f"K12 + K15 chain grad {k}", rtol=1e-4, noise=5e-5)
