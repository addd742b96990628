"""The feed-forward PPO kernels against float64 past their first trip: K7 (rs_ppo_grad / rs_ppo_update_step), rs_policy_forward and
the fused tail's Adam step.  References, cases and the rule are in tests/_f64_ref.py (its CPU self-checks: test_f64_references.py).

K7.  rs_ppo_grad2_kernel hands groups of 32 samples to 256 x 8 = 2048 waves, trips = ceil(ceil(M / 32) / 2048).  Sizes (R.FF_SIZES):
1, 31, 32, 33, 63, 65 (the last group mostly padding, exactly full, one sample into a second group), 65 536 (every wave one full
group), 65 537 (two trips: wave 0's second group holds one sample, the other 2047 waves run a clamped weight-0 trip), 65 536 + 32 768
+ 5 (half of the waves have a real second group, one of them partial) and 3 x 65 536 + 225 (four trips).  Half of the weight lies on the
tail (R.ff_weights), so a lost, repeated or mis-indexed tail is wrong by tens of percent (proved on the CPU at >= 100 x the allowance).

The rule, per gradient element and per statistic:  |got - ref| <= R.FF_RTOL |ref| + k U mag + R.FF_TINY,  U = 2^-24, mag the sum over
samples of the absolute per-sample term (R.ff_loss_f64).  The constants come from R.ff_error_model, term by term (units of U, s the
parameters' scale, SAFETY = 2 on everything because the terms are expectations):
  layer 1     dot of depth 11 + 1 (bias column): (sqrt(12) + 1) S1, S1 = 12 s 0.8; the + 1 is the rounding of the 2 log2(e) prescale
  tanh (x 2)  rs_tanh_scaled: v_exp_f32 1, argument scaling <= 0.5, add 0.5, v_rcp_f32 1, fma 0.5 -> 4 absolute, tanh' <= 1
  layer 2     h1's error through W2 (sqrt(64) s E_h1) + dot of depth 64 ((8 + 1) 65 s) + tanh
  output      h2's error through W3 + the 64-deep chains ((8 + 1) 65 s) + bias: E_out (x SAFETY: E_logit, part 4's absolute bound)
  softmax     eight __expf, their sum, one __logf, two subtractions: E_lp = 2 E_out + 9.8;  p_j: E_lp + 21 (argument scaling at lp ~ -20)
  ratio       __expf(logp - lpo): E_lp + 3, g_lp two products;  dz = g_lp (1[a = j] - p_j): E_dz = E_glp + E_p + 1
  backward    1 - h2^2 (2 E_h2 / gain, gain = E tanh' = 0.5 | 0.15), 3;  1 - h1^2 (2 E_h1 / gain), 3;  the activation factor of the
              dW3 / dW2 terms (2 E_h2).  The rounding of W3^T dz (depth 8) and W2^T dpre2 (depth 64) is relative to the sum of their
              absolute terms, not to their result: it is charged at R.FF_K_BP = SAFETY (sqrt(64) + 1) = 18 to bp_mag, the magnitude
              with the back-propagated error replaced by its bound without cancellation (so a gradient's "k U mag" reads
              U (k mag + 18 bp_mag)).  With that term inside k as 72 U mag -- right over many samples -- K7 stood at 1.05 and float32
              torch at 0.40 of the bound in a.w1 / a.b1 at M = 1, where the one unit whose 64 terms cancel best decides a row of dW1
  sums        a wave's MFMA accumulators over trips x 32 <= 128 samples sqrt(128) = 11.3, the 8-wave LDS sum sqrt(8) = 2.8, the 256
              slabs as 16 chunks of 16: 4 + 4
giving k = 6476 (k U = 3.9e-4) at s = 0.25 and k = 56520 (3.4e-3) at s = 0.75, where tanh units saturate and the softmax peaks.  Float32
torch on the CPU sits at <= 0.09 of this bound; K7's figures are in profiles/r11_ff_ppo_f64_error_ratios.txt.

rs_policy_forward: R.close with rtol 4 U, tiny = E_logit U (the forward half of the model; no sum over samples).

Adam (rs_ppo_tail_kernel), against torch.optim.Adam's formulas in float64 on the float32 gradient the bucket holds.  The hyper-parameters
are the float32 values the kernel holds (0.9f, 0.999f, 1e-8f, lr as a float32), widened: like every input here their rounding is charged
to neither side.  (0.999f is 1.3e-8 above 0.999, so the kernel's 1 - beta2 is 1.3e-5 of its value above torch's float64 1 - 0.999: the
kernel is Adam at beta2 = 0.99900001287.)  Roundings counted per expression, -ffp-contract=off so no product fuses with a sum; division
and square root counted 2 each, powf at HIP's stated 1 ulp:
  m' = m + (g - m)(1 - b1)       1 - b1 exact (Sterbenz); subtraction 1 and product 1 on c1 |g - m|, sum 1 on |m'|: U (2 c1 |g - m| + |m'|)
  v' = b2 v + (1 - b2) g g       1 - b2 exact; b2 v 1, the two products 2, the sum 1, all terms positive: 3 U v'
  bc = 1 - powf(b, t)            powf's 1 ulp is 2^-24 = U absolute for b^t in [0.5, 1), the subtraction is exact there: U / bc relative, which
                                 at t = 6 is 2.2 U for bc1 = 0.469 and 167.2 U for bc2 = 0.00598 -- the one large term, a cancellation
  p' = p - (lr / bc1)(m' / (sqrtf(v') / sqrtf(bc2) + eps))
                                 sqrtf(v') 2 + v's 3 / 2, sqrtf(bc2) 2 + 167.2 / 2, their quotient 2, + eps 1, m' / denom 2, lr / bc1 2.2 + 2,
                                 product 1: 99.3 -> 100 U |delta| + m's allowance x step / denom, and the subtraction: 1 U |p'|
                                 (|delta| ~ 1e-4 |p|: through p only an error of delta above ~1e-4 of it shows; m and v carry the precision)
"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
U = R.U


def _gpu(c):
    ac = copy.deepcopy(c.ac).cuda()
    return ac, tuple(t.cuda().contiguous() for t in c.batch)


@pytest.mark.parametrize("case", R.FF_CASES, ids=R.ff_case_id)
def test_k7_matches_float64(case):
    """rs_ppo_grad on every case under the rule; past one trip also rs_ppo_update_step (lr = 0, no KL stop) on a copy of the agent,
    whose bucket must equal rs_ppo_grad's bit for bit."""
    from radiation_ppo_amd.ppo import FusedPPOGrad
    M, pset = case
    c = R.ff_case(M, pset)
    ac, b = _gpu(c)
    f = FusedPPOGrad(ac)
    stats, g = f(*b, R.FF_CLIP, R.FF_ALPHA, R.FF_VF)
    rep = []
    try:
        R.check_ff(stats, g, c.ref, pset, "K7 " + R.ff_case_id(case), report=rep)
    finally:
        print(rep[0])
    if R.ff_trips(M) > 1:
        f2 = FusedPPOGrad(copy.deepcopy(ac))
        f2.begin_update()
        f2.step(*b, R.FF_CLIP, R.FF_ALPHA, R.FF_VF, lr=0.0, kl_threshold=1e30)
        torch.cuda.synchronize()
        assert torch.equal(f2.bucket.view(torch.int32), f.bucket.view(torch.int32))
        assert torch.equal(f2.stats.view(torch.int64), f.stats.view(torch.int64))


def test_k7_zero_weight_rows_contribute_nothing():
    """M = 1000 with w = 0 on 100 scattered rows whose X is x 1e3 and adv x 1e6 (finite): the reference is computed without them."""
    from radiation_ppo_amd.ppo import FusedPPOGrad
    c = R.ff_case(1000, "base", zero_rows=100)
    assert int((c.w == 0).sum()) == 100
    ac, b = _gpu(c)
    stats, g = FusedPPOGrad(ac)(*b, R.FF_CLIP, R.FF_ALPHA, R.FF_VF)
    rep = []
    try:
        R.check_ff(stats, g, c.ref, "base", "K7 M1000-base-100-zero-rows", report=rep)
    finally:
        print(rep[0])


@pytest.mark.parametrize("pset", sorted(R.FF_SCALES))
def test_policy_forward_matches_float64(pset):
    """rs_policy_forward (grid capped at 2048 waves of 64 samples) against the float64 twin: M = 1, 63, 64, 65, 131 072 (every wave one
    group), 131 073 (the grid-stride loop's first second iteration, one valid lane), 131 072 + 64 000 + 1; at 131 073 also the forms
    without logits and without value."""
    from radiation_ppo_amd.ppo import policy_forward
    ac = R.ff_agent(pset)
    ac64, acg = R.f64(ac), copy.deepcopy(ac).cuda()
    big = max(R.FWD_SIZES)
    X = torch.randn(big, 11, generator=torch.Generator().manual_seed(17))
    lg64, v64 = R.ff_forward_f64(ac64, X)
    t_out, _ = R.fwd_tolerance(pset)
    line, fails = [], []
    for M in R.FWD_SIZES:
        x = X[:M].cuda().contiguous()
        forms = [(True, True)] + ([(False, True), (True, False)] if M == 131073 else [])
        for wl, wv in forms:
            lg, v = policy_forward(acg, x, want_logits=wl, want_value=wv)
            assert (lg is None) == (not wl) and (v is None) == (not wv)
            for name, got, ref in (("logits", lg, lg64[:M]), ("value", v, v64[:M])):
                if got is None:
                    continue
                r = R.close_ratio(got, ref, **t_out)
                line.append(f"M{M}{'' if wl and wv else '-only'} {name} {r:.4f}")
                if not (r <= 1.0 and bool(torch.isfinite(got).all())):
                    fails.append(line[-1])
    print(f"rs_policy_forward {pset} | " + " ".join(line))
    assert not fails, fails


def test_fused_tail_adam_step_matches_float64_formulas():
    """One rs_ppo_update_step at M = 1000 from random moments (v > 0) at adam_step = 5: p, m, v against torch.optim.Adam's formulas in
    float64 on the bucket's float32 gradient (allowances: module docstring), adam_step 6, iters 1; a second call with kl_threshold
    below the batch's KL leaves parameters and moments as they are bit for bit, stopped = 1, adam_step unchanged."""
    from radiation_ppo_amd.ppo import FusedPPOGrad
    c = R.ff_case(1000, "base")
    ac, b = _gpu(c)
    f = FusedPPOGrad(ac)
    gen = torch.Generator().manual_seed(5)
    f.m.copy_(torch.randn(f.m.shape, generator=gen) * 1e-3)
    f.v.copy_(torch.rand(f.v.shape, generator=gen) * 1e-5 + 1e-9)
    f.begin_update()
    f.state_i32[0] = 5
    lr = 3e-4
    flat = lambda: torch.cat([p.detach().reshape(-1) for p, _ in f.views]).double().cpu()
    p0, m0, v0 = flat(), f.m.double().cpu(), f.v.double().cpu()
    f.step(*b, R.FF_CLIP, R.FF_ALPHA, R.FF_VF, lr=lr, kl_threshold=1e30)
    iters, stopped, adam_step, _ = f.read_state()
    assert (iters, stopped, adam_step) == (1, 0, 6)
    g = f.grads.double().cpu()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))     # the hyper-parameters as the kernel holds them
    lr32, b1, b2, eps = f32(lr), f32(0.9), f32(0.999), f32(1e-8)
    m1 = m0 + (g - m0) * (1 - b1)
    v1 = b2 * v0 + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** 6, 1 - b2 ** 6
    denom = v1.sqrt() / bc2 ** 0.5 + eps
    step = lr32 / bc1
    delta = step * m1 / denom
    p1 = p0 - delta
    tol_m = U * (2 * (1 - b1) * (g - m0).abs() + m1.abs())
    tol_v = 3 * U * v1
    k_delta = (2 + 1.5) + (2 + 0.5 / bc2) + 2 + 1 + 2 + (1 / bc1 + 2) + 1
    assert 99.0 < k_delta < 100.0
    tol_p = 100 * U * delta.abs() + tol_m * step / denom + U * p1.abs()
    worst = {}
    for name, got, ref, tol in (("m", f.m, m1, tol_m), ("v", f.v, v1, tol_v), ("p", flat(), p1, tol_p)):
        worst[name] = float(((got.double().cpu() - ref).abs() / tol).max())
    print("fused tail Adam step | " + " ".join(f"{k} {r:.4f}" for k, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst
    assert float((p1 - p0).abs().max()) > 1e-5                                           # the step moved the parameters
    kl = float(f.stats[0])
    before = [t.clone() for t in (flat().float().view(torch.int32), f.m.view(torch.int32), f.v.view(torch.int32))]
    f.step(*b, R.FF_CLIP, R.FF_ALPHA, R.FF_VF, lr=lr, kl_threshold=kl - abs(kl) - 1.0)
    iters, stopped, adam_step, _ = f.read_state()
    assert (iters, stopped, adam_step) == (2, 1, 6), (iters, stopped, adam_step, kl)
    after = [flat().float().view(torch.int32), f.m.view(torch.int32), f.v.view(torch.int32)]
    assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(before, after))
