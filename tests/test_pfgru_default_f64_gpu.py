"""The default-width PFGRU kernels -- K11 (csrc/rs_pfgru.hip: rs_pfgru_step_recorded) and K13 (csrc/rs_pfgru_train.hip: rs_pfgru_train,
rs_pfgru_train_keyed), 40 particles x 24 units, what the product runs at the reference's layer sizes -- against float64 on the CPU.
Both kernels take the noise and the resampling indices as inputs (RecordedKernelDraws), so every discrete choice is the same on both
sides and the whole arithmetic is compared with no near-tie exception.  Tolerances: tests/_f64_ref.py's error model; each test names
the terms its constants cover.  The references are held to the float32 library path on the CPU in tests/test_f64_references.py."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402
from test_pfgru_sized_f64_gpu import _cells, _indices  # noqa: E402

pytestmark = pytest.mark.gpu

P, H = 40, 24


@pytest.mark.parametrize("carry", [True, False])
def test_default_recorded_step_matches_float64(carry):
    """K11's recorded-draw instantiation (rs_pfgru_step_recorded, weights from pack_weights) against PFGRUCell.forward in float64:
    test_pfgru_sized_f64_gpu.test_sized_recorded_step_matches_float64 at H = 24 with K11's entry points in place of the sized ones --
    the same cells, inputs, indices (identity / one repeated particle at the first and last env), N = 1, 6, 7, 200, A = 1, 3, 8, four
    steps, the mask on alternate steps, carry on and off.  The constants are the sized test's, unchanged (K = 27 term gate sums lie
    inside its K = H + 3 <= 67): h and p rtol 2e-5, atol 1e-5 of the scale over up to 4 carried steps; pred rtol 1e-4, atol 1e-5 of the
    scale plus 2e-6 on the outputs whose float64 pre-activations are at least 1e-4 from a ReLU kink (R.hid_obs_fragile); the same
    kept >= 0.6 counted condition.  Masked-out envs keep the bits of pred, h and p; carry off writes no state at all."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.pfgru import PredictorBank, pack_weights
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kept = counted = 0
    for N in (1, 6, 7, 200):
        for A in (1, 3, 8):
            key = (carry, N, A)
            cells = _cells(A, H)
            c64 = [R.f64(c) for c in cells]
            w = pack_weights([c.cuda() for c in cells])
            g = torch.Generator().manual_seed(H * 1000 + N * 10 + A)
            h0 = torch.rand(A, N, P, H, generator=g)
            p0 = torch.log_softmax(torch.randn(A, N, P, generator=g), dim=-1)
            hq = PredictorBank.to_quads(h0).cuda().contiguous()
            pk = p0.cuda().contiguous()
            pred = torch.full((N, A, 2), -5.0, device="cuda")
            ref_h, ref_p = h0.double(), p0.double()
            for t in range(4):
                kt = key + (t,)
                obs = torch.rand(N, A, 11, generator=g)
                obs[..., 0] = torch.randint(0, 4000, (N, A), generator=g).float() / 100.0 - 10.0
                eps = torch.randn(A, N, P, H, generator=g)
                idx = _indices(A, N, t, g)
                mask = None if t % 2 == 0 else (torch.rand(N, generator=g) < 0.6).to(torch.uint8)
                if mask is not None and N > 1:
                    mask[0], mask[N - 1] = 1, 0
                hq_before, p_before, pred_before = hq.clone(), pk.clone(), pred.clone()
                oc, ec, ic = obs.cuda(), eps.cuda().contiguous(), idx.to(torch.int32).cuda().contiguous()
                mc = None if mask is None else mask.cuda()
                _lib.check(lib.rs_pfgru_step_recorded(w.data_ptr(), oc.data_ptr(), hq.data_ptr(), pk.data_ptr(), ec.data_ptr(), ic.data_ptr(),
                                                      None if mc is None else mc.data_ptr(), 1 if carry else 0, 0.7, pred.data_ptr(), N, A, st),
                           "rs_pfgru_step_recorded")
                torch.cuda.synchronize()
                on = torch.ones(N, dtype=torch.bool) if mask is None else mask.bool()
                got_h, got_p, got_pred = PredictorBank.from_quads(hq.cpu()), pk.cpu(), pred.cpu()
                new_h, new_p = ref_h.clone(), ref_p.clone()
                for a in range(A):
                    pr64, h1, p1, mean = R.pfgru_step_f64(c64[a], obs[:, a, :3].double(), ref_h[a], ref_p[a], eps[a].double(), idx[a])
                    keep = ~R.hid_obs_fragile(c64[a], mean, 1e-4) & on.view(N, 1)
                    kept += int((keep & (pr64 != 0)).sum()); counted += 2 * int(on.sum())
                    R.close(got_pred[:, a][keep], pr64[keep], f"K11 pred {kt} a={a}", rtol=1e-4, noise=1e-5, tiny=2e-6)
                    if carry:
                        R.close(got_h[a][on], h1[on], f"K11 h {kt} a={a}", rtol=2e-5, noise=1e-5)
                        R.close(got_p[a][on], p1[on], f"K11 p {kt} a={a}", rtol=2e-5, noise=1e-5)
                        new_h[a][on], new_p[a][on] = h1[on], p1[on]
                off = ~on
                assert torch.equal(pred.cpu()[off], pred_before.cpu()[off]), kt
                if carry:
                    assert torch.equal(hq.cpu()[:, off], hq_before.cpu()[:, off]) and torch.equal(pk.cpu()[:, off], p_before.cpu()[:, off]), kt
                    ref_h, ref_p = new_h, new_p
                else:
                    assert torch.equal(hq, hq_before) and torch.equal(pk, p_before), kt
            assert not math.isnan(float(pred.sum()))
    assert kept >= 0.6 * counted, (kept, counted)


def _agent(case):
    from radiation_ppo_amd.rada2c import BpArgs, RNNAgentPPO
    l2, l1, elbo = case[4]
    bpa = BpArgs(l2_weight=l2, l1_weight=l1, elbo_weight=elbo, area_scale=2500.0)
    torch.manual_seed(5)
    ag = RNNAgentPPO(id=0, seed=1, bp_args=bpa)
    assert ag.agent.fused_pfgru
    R.k13_cell(ag.agent.model, case[5])
    return ag, bpa


def _report(line):
    """One line per case for the record of measured error ratios (the test run's output)."""
    print("K13 f64:", line)


@pytest.mark.parametrize("case", R.K13_CASES, ids=R.k13_case_id)
def test_k13_training_pass_matches_float64(case):
    """K13 through RNNAgentPPO.model_pass_hip with recorded draws (RecordedKernelDraws: indices are the kernel's input, u = NULL)
    against R.model_loss_f64 + float64 autograd, fed exactly what model_pass_hip hands the kernel (the float32 target and step
    weights, widened).  Cases: one one-step episode; 70 one-step episodes; one 120-step episode; ragged episodes of 1 .. 40 steps,
    sorted by length and not; 65 episodes of the reference's 120 steps (more than one workgroup's waves); loss weights (l2, l1, elbo) =
    (1, 0, 1) the default, (1, 0.5, 1), (1, 0.5, 0) ELBO off, (0, 1, 1) L1 terms alone.  Cell parameters off the initialisation.

    The bound comes from the error model of test_rnn_sized_f64_gpu.test_sized_gru_sequence_matches_float64, which has the same
    sources -- hardware rcp / exp2 gates (~4 u + u |x| each), back-propagation through up to 120 steps, weight gradients summed over
    L x E per-sample terms -- with 40 particles per (step, episode) more terms per sum (sqrt(40) ~ 6 in expectation) and bw_log /
    bw_exp / bw_div (1 ulp each) in the loss; it was fixed before K13 was ever run against float64:
      loss       5e-6 of the sum of its absolute per-(step, episode) terms (R.model_loss_f64's mags): per-term ~1e-6 (the step's
                 state errors, then log / exp), summed over a wave's lanes and <= 120 steps in float32, over episodes in float64;
      gradients  per block (fc_z, fc_r, the mu and var rows of fc_n, fc_obs, hid_obs.0, hid_obs.2; weight and bias separately),
                 each against its own largest element: rtol 1e-4, noise 3e-4 of the block's scale at 120 x 65 and 1e-4 at the
                 smaller cases (the GRU test's 5e-5 x sqrt(40), rounded: MFMA sums over 40 particles x <= 120 steps per episode in
                 float32, then E slab rows), floor 2e-6 of the cell's largest gradient element (saturated gates, as there);
      fc_obs.bias shifts every particle's logit alike and cancels in the log-softmax: exactly 0 in exact arithmetic (~1e-19 in
                 float64), held to the floor alone.
    ReLU / |.| kinks: hid_obs runs 41 times per (step, episode) and a float32 pre-activation within rounding of 0 takes the other
    branch.  R.kink_count finds ~1e-3 of the evaluations within 1e-5 of a kink (5 of 2 870 .. 71 of 39 360 on the CPU cases); an
    allowance of that count times a block's largest per-sample term would be 1e4 - 1e5 times the block's tolerance and void the test,
    so NO allowance is made and no sample is masked: a flip moves one term of a sum of thousands by the term's own size, and the float32
    library path, which has the same kinks, stays below 0.4 % of this bound on every case (test_f64_references.py).
    Also: fewer than 20 % of the float64 location outputs on valid steps are clamped by the final ReLU; a second launch returns
    the same bits."""
    from radiation_ppo_amd.rada2c import RecordedKernelDraws, unpack_train_grads
    T, N, ragged, srt, _, seed = case
    name = R.k13_case_id(case)
    ag, bpa = _agent(case)
    cell = ag.agent.model
    B = R.k13_batch(T, N, seed, ragged, srt, device="cuda")
    L, E = B.X.shape[0], B.X.shape[1]
    pf, eps, idx = R.k13_draws(L, E, 100 + seed)
    res, g64, _ = R.k13_reference(cell, B, bpa, pf, eps, idx)
    assert res.clamped < 0.2, res.clamped
    sl = slice(0, E)
    d = RecordedKernelDraws(pf.cuda(), None, eps.cuda(), idx.cuda())
    loss_k, slab, idx_k = ag.model_pass_hip(B, sl, d)
    loss_k, slab = float(loss_k), slab.clone()
    assert torch.equal(idx_k.cpu().long()[B.valid.cpu()], idx[B.valid.cpu()])            # the indices are inputs: untouched
    loss_2, slab_2, _ = ag.model_pass_hip(B, sl, d)
    assert float(loss_2) == loss_k and torch.equal(slab, slab_2), name                   # bitwise repeatable
    lerr = abs(loss_k - float(res.loss.detach())) / (5e-6 * float(res.mags))
    rep = []
    try:
        worst = R.check_k13_grads(unpack_train_grads(cell, slab), g64, L, E, name, report=rep)
    finally:
        _report(f"{name} L {L} E {E} loss {lerr:.4f} kinks {res.kinks}/{res.samples} clamped {res.clamped:.3f} | "
                + " ".join(f"{k} {v:.4f}" for k, v in rep))
    assert math.isfinite(loss_k) and lerr <= 1.0, (name, loss_k, float(res.loss.detach()), lerr)
    assert worst <= 1.0


def _k13_raw(ag, B, pf, eps, idx):
    """rs_pfgru_train on batch B with recorded draws, as RNNAgentPPO.model_pass_hip launches it, on fresh buffers: the per-episode
    losses [E] and gradient slabs [E, PF_TRAIN_GRAD_FLOATS] before model_pass_hip sums them."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.rada2c import PF_TRAIN_GRAD_FLOATS, pack_train_weights
    a = ag.bp_args
    X = B.X.contiguous()
    L, E = X.shape[0], X.shape[1]
    tar, bp = R.k13_inputs(B, a)
    tar, bp = tar.contiguous(), bp.contiguous()
    lens, w_ep = B.lens.contiguous(), B.w_ep.float().contiguous()
    dev = X.device
    hs = torch.empty(L, E, 40, 24, dtype=torch.float32, device=dev)
    ps = torch.empty(L, E, 40, dtype=torch.float32, device=dev)
    gates = torch.empty(L * E * 40 * 96, dtype=torch.float32, device=dev)
    loss = torch.full((E,), 7.0, dtype=torch.float32, device=dev)
    slab = torch.full((E, PF_TRAIN_GRAD_FLOATS), 7.0, dtype=torch.float32, device=dev)
    w = pack_train_weights(ag.agent.model)
    pfc, epc, ic = pf.cuda().contiguous(), eps.cuda().contiguous(), idx.to(torch.int32).cuda().contiguous()
    assert pfc.shape == (E, 40, 24) and epc.shape == (L, E, 40, 24) and ic.shape == (L, E, 40) and tar.shape == (L, E, 2) and bp.shape == (L, E)
    assert int(lens.max()) <= L and int(lens.min()) >= 1 and int(ic.min()) >= 0 and int(ic.max()) < 40
    _lib.check(_lib.load().rs_pfgru_train(w.data_ptr(), X.data_ptr(), tar.data_ptr(), bp.data_ptr(), lens.data_ptr(), w_ep.data_ptr(), pfc.data_ptr(),
                                          epc.data_ptr(), None, hs.data_ptr(), ps.data_ptr(), gates.data_ptr(), ic.data_ptr(), loss.data_ptr(),
                                          slab.data_ptr(), L, E, float(ag.agent.model.resamp_alpha), float(a.l2_weight), float(a.l1_weight),
                                          float(a.elbo_weight), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "rs_pfgru_train")
    torch.cuda.synchronize()
    return loss, slab


def _take(B, keep):
    from radiation_ppo_amd.rada2c import EpisodeBatch
    return EpisodeBatch(X=B.X[:, keep], act=B.act[:, keep], adv=B.adv[:, keep], ret=B.ret[:, keep], logp=B.logp[:, keep], src=B.src[:, keep],
                        valid=B.valid[:, keep], lens=B.lens[keep], w_ep=B.w_ep[keep], key=B.key[keep])


def test_k13_zero_weight_episodes_have_zero_rows_and_leave_the_others_alone():
    """Episodes with w_ep = 0 (every third one, the first and the last among them): their slab rows and losses are exactly 0, and
    the other episodes' rows and losses are bit for bit those of a launch without the zero-weight episodes.  The packing allows the
    comparison: K13 runs one wave per episode and writes one slab row per episode, so an episode's arithmetic does not depend on its
    neighbours; only the caller's sum over the rows does, which is why the rows are taken from the kernel directly here."""
    case = R.K13_CASES[7]
    ag, bpa = _agent(case)
    B = R.k13_batch(case[0], case[1], case[5], True, False, device="cuda")
    L, E = B.X.shape[0], B.X.shape[1]
    pf, eps, idx = R.k13_draws(L, E, 100 + case[5])
    zero = torch.zeros(E, dtype=torch.bool)
    zero[0::3] = True; zero[E - 1] = True
    B.w_ep = torch.where(zero.cuda(), torch.zeros_like(B.w_ep), B.w_ep)
    loss, slab = _k13_raw(ag, B, pf, eps, idx)
    assert bool((slab[zero.cuda()] == 0).all()) and bool((loss[zero.cuda()] == 0).all())
    keep = (~zero).nonzero().squeeze(1)
    assert int(B.lens[keep.cuda()].max()) == L                                     # the same padded length in both launches
    loss_b, slab_b = _k13_raw(ag, _take(B, keep.cuda()), pf[keep], eps[:, keep], idx[:, keep])
    assert torch.equal(slab[keep.cuda()], slab_b) and torch.equal(loss[keep.cuda()], loss_b)
    assert float(slab_b.abs().max()) > 0 and bool(torch.isfinite(slab_b).all())


def test_k13_with_hashed_draws_matches_float64():
    """K13 through KernelDraws (hashed uniforms: the kernel picks the resampling indices) on the ragged case: the float64 reference
    fed the kernel's own indices, same bounds as test_k13_training_pass_matches_float64; and the indices themselves against the
    float64 inverse CDF of the same uniforms (PFGRUCell.forward's resample_u branch on the float64 twin, continued from the kernel's
    choice so that one moved index cannot cascade): all but 2 of the valid (step, episode) rows take the same 40 particles."""
    from radiation_ppo_amd.rada2c import KernelDraws, unpack_train_grads
    case = R.K13_CASES[7]
    name = "hashed " + R.k13_case_id(case)
    ag, bpa = _agent(case)
    cell = ag.agent.model
    B = R.k13_batch(case[0], case[1], case[5], True, True, device="cuda")
    L, E = B.X.shape[0], B.X.shape[1]
    kd = KernelDraws(B.key * 64 + 1, L)
    loss_k, slab, idx = ag.model_pass_hip(B, slice(0, E), kd)
    loss_k, slab, idx = float(loss_k), slab.clone(), idx.clone().cpu().long()
    valid = B.valid.cpu()
    assert int(idx[valid].min()) >= 0 and int(idx[valid].max()) < 40
    idx = torch.where(valid.unsqueeze(-1), idx, torch.zeros_like(idx))
    pf, eps, u = kd._pf.cpu(), kd._eps.cpu(), kd._u.cpu()
    res, g64, c64 = R.k13_reference(cell, B, bpa, pf, eps, idx)
    lerr = abs(loss_k - float(res.loss.detach())) / (5e-6 * float(res.mags))
    rep = []
    try:
        R.check_k13_grads(unpack_train_grads(cell, slab), g64, L, E, name, report=rep)
    finally:
        _report(f"{name} L {L} E {E} loss {lerr:.4f} | " + " ".join(f"{k} {v:.4f}" for k, v in rep))
    assert lerr <= 1.0, (loss_k, float(res.loss.detach()))
    same = tot = 0
    with torch.no_grad():
        h, p = pf.double(), torch.full((E, 40), math.log(1 / 40), dtype=torch.float64)
        X3 = B.X[..., :3].cpu().double()
        for t in range(L):
            _, (hu, _) = c64(X3[t], (h, p), eps[t].double(), resample_u=u[t])
            _, (h, p) = c64(X3[t], (h, p), eps[t].double(), resample_idx=idx[t])
            ok = ((hu - h).abs().amax(dim=(1, 2)) < 1e-12) & valid[t]
            same += int(ok.sum()); tot += int(valid[t].sum())
    assert same >= tot - 2, (same, tot)
