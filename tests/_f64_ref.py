"""Float64 references and the tolerance rule shared by the float64 tests of the sized kernels (test_rnn_sized_f64_gpu.py,
test_pfgru_sized_f64_gpu.py) and their CPU self-checks (test_f64_references.py).

The references are the project's own modules copied and cast (copy.deepcopy(m).double().cpu()); what is written out here by hand is
the library branch of RNNAgentPPO.a2c_losses behind the GRU (heads_loss_f64), the collector's inverse-CDF draw (draw_f64), and the
kink masks of the ReLUs.  Each of them is held to the project's float32 path on the CPU before any GPU test relies on it.

Tolerance rule (close): |got - ref| <= rtol |ref| + noise max|ref| + tiny, elementwise, with ref in float64.  The float32 error model
behind every rtol / noise constant: u = 2^-24 per rounding; a dot product or sum of n terms carries up to ~n u of the sum of its
absolute terms in the worst case and ~sqrt(n) u in expectation; the hardware reciprocal, exp2 and log (v_rcp_f32, v_exp_f32,
v_log_f32, which sigm / tanh_ in rs_rnn_sized.hip and sz_sigmoid / sz_exp / sz_log in rs_pfgru_sized.hip are built from) add 1 ulp
each, and the scaling of their argument (x * log2(e)) adds 0.5 ulp of |x log2(e)| to the exponent, i.e. a relative error of
~u |x| of the result for |x| up to ~10.  Each test states which terms its constants cover."""
import copy

import torch

U = 2.0 ** -24                       # float32 unit roundoff


def close(got, ref, name, rtol, noise, tiny=1e-12):
    """got: any float tensor (cast to float64 on the CPU), ref: the float64 reference.  See the module docstring."""
    a = got.detach().double().cpu()
    b = ref.detach().double().cpu()
    assert a.shape == b.shape, (name, tuple(a.shape), tuple(b.shape))
    scale = float(b.abs().max()) if b.numel() else 0.0
    allowed = rtol * b.abs() + noise * scale + tiny
    err = (a - b).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / allowed).max()) if b.numel() else 0.0
    assert bool(torch.isfinite(a).all()) and ratio <= 1.0, (name, float(err.max()), scale, ratio)


def f64(m):
    """The project's module m as its float64 twin on the CPU."""
    return copy.deepcopy(m).double().cpu()


# ------------------------------------------------------------------------------------------------ RAD-A2C
HIDS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
HEADS = ((2, 2), (2, 64), (9, 57), (8, 17), (64, 2), (63, 33), (4, 41))     # head edges: 2, 4, 63, 64 units and 8k + 1 (9, 17, 33, 41, 57)


def tier(hid):
    return (hid + 15) // 16 * 16


def head_grid(per=3):
    """hid -> its `per` head pairs, drawn in rotation from HEADS with one counter per GRU tier: a tier of h widths meets the next
    h * per pairs of the rotation, so every tier (16: 7 widths, 32 / 48 / 64: 3 widths each) meets all seven pairs."""
    ctr, out = {}, {}
    for h in HIDS:
        c = ctr.get(tier(h), 0)
        out[h] = [HEADS[(c + i) % len(HEADS)] for i in range(per)]
        ctr[tier(h)] = c + per
    return out


def rnn_args(hid, pol, val, rec=24):
    return dict(hidden=((hid,),), hidden_sizes_pol=((pol,),), hidden_sizes_val=((val,),), hidden_sizes_rec=(rec,))


def heads_params(ac):
    """The eight head parameters in HeadsLossSized's argument order."""
    v = ac.pi.logits_net.v_net
    return [v.Woms[0].weight, v.Woms[0].bias, v.Woms[2].weight, v.Woms[2].bias, v.Valms[0].weight, v.Valms[0].bias, v.Valms[2].weight,
            v.Valms[2].bias]


def heads_loss_f64(ac, hs, act, adv, ret, logp_old, wt, clip, vf):
    """The library branch of RNNAgentPPO.a2c_losses (rada2c.py: the lines after `logits, val = ac.heads(...)`) on flat samples, in
    the dtype of ac / hs (float64 for the tests): returns (loss, stats [kl, entropy, clip fraction, value loss, surrogate, weight sum],
    mags), mags [7] the sums of the absolute per-sample terms of the six statistics and of the loss (the scale a float32 sum of those
    terms is rounded against; for kl, the surrogate and the value loss, whose terms are differences, the magnitudes of what is
    subtracted: |logp_old| + |logp|, |term| (1 + |logp|), (val - ret)^2 + 2 |val - ret| (1 + |val| + |ret|)).  The loss is
    -(surrogate - vf value loss): the branch's entropy term is a detached constant, so it changes no gradient, and the heads-loss
    kernel's loss leaves it out."""
    logits, val = ac.heads(hs)
    lp_all = torch.log_softmax(logits, dim=-1)
    logp = lp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1)
    ratio = torch.exp(logp - logp_old)
    clip_adv = torch.clamp(ratio, 1 - clip, 1 + clip) * adv
    surr = (wt * torch.min(ratio * adv, clip_adv)).sum()
    val_loss = (wt * (val - ret) ** 2).sum()
    with torch.no_grad():
        ent = (wt * -(lp_all.exp() * lp_all).sum(-1)).sum()
        clipped = (ratio > 1 + clip) | (ratio < 1 - clip)
        kl = (wt * (logp_old - logp)).sum()
        cf = (wt * clipped.to(wt.dtype)).sum()
        # kl, the ratio and val - ret are differences: their float32 errors scale with |logp|, |val| and |ret|, not with the difference
        a_surr = (wt * torch.min(ratio * adv, clip_adv) * (1 + logp.abs())).abs().sum()
        d = (val - ret).abs()
        a_vl = (wt * (d * d + 2 * d * (1 + val.abs() + ret.abs()))).sum()
        mags = torch.stack([(wt * (logp_old.abs() + logp.abs())).sum(), ent, cf, a_vl, a_surr, wt.sum(), a_surr + vf * a_vl])
    loss = -(surr - vf * val_loss)
    return loss, torch.stack([kl, ent, cf, val_loss.detach(), surr.detach(), wt.sum()]), mags


def target_ratios(n, g, clip=0.2, margin=0.02):
    """n PPO ratios spread over (1 - 2 clip, 1 + 3 clip): a third below the clip range, a third inside it, a third above it, each at
    least `margin` from 1 +- clip, where the gradient of the clipped surrogate jumps (a float32 ratio is within ~1e-6 of its float64
    value, far inside the margin, so kernel and reference take the same branch)."""
    part = torch.randint(0, 3, (n,), generator=g)
    x = torch.rand(n, generator=g, dtype=torch.float64)
    lo, hi = 1 - clip, 1 + clip
    below = (1 - 2 * clip) + x * (clip - margin)                  # [1 - 2 clip, lo - margin)
    inside = (lo + margin) + x * (2 * clip - 2 * margin)          # [lo + margin, hi - margin)
    above = (hi + margin) + x * (2 * clip - margin)               # [hi + margin, 1 + 3 clip)
    return torch.where(part == 0, below, torch.where(part == 1, inside, above))


def draw_f64(logits64, u):
    """The collector's inverse-CDF draw in float64: (action, log-probabilities [N, 8], CDF [N, 8])."""
    lp_all = torch.log_softmax(logits64, dim=-1)
    cdf = torch.cumsum(lp_all.exp(), dim=-1)
    act = (cdf[:, :-1] <= u.double().unsqueeze(-1)).sum(dim=-1)
    return act, lp_all, cdf


def check_draw(act, logp, act64, lp64, cdf64, u, name):
    """The kernel's action equals the float64 draw except on a lane whose uniform lies within 1e-5 of a CDF step (test_rnn_sized_gpu
    _check_draw's rule, the CDF now in float64: the kernel's float32 CDF is a sum of 8 expf terms, ~8 u off, plus the logits' error);
    logp must match on the lanes where the action matches: log-softmax of logits within ~1e-6 (see the logits tolerance) plus expf /
    logf rounding, held to rtol 1e-5, atol 5e-6 as the float32 check of the same quantity."""
    act, logp, u = act.cpu(), logp.cpu(), u.cpu()
    edge = (cdf64[:, :-1] - u.double().unsqueeze(-1)).abs().amin(dim=1) < 1e-5
    assert bool(((act == act64) | edge).all()) and int((act != act64).sum()) <= 2, (name, int((act != act64).sum()))
    same = act == act64
    close(logp[same], lp64.gather(-1, act64.unsqueeze(-1)).squeeze(-1)[same], f"logp {name}", rtol=1e-5, noise=0.0, tiny=5e-6)


def make_batch(seed, T=60, N=150, device="cuda"):
    """An episode batch as test_rnn_sized_gpu._batch, on `device` (logp_old is replaced by the tests)."""
    import numpy as np
    from radiation_ppo_amd.rada2c import pack_episodes
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(T, N, 11, generator=g)
    act = torch.randint(0, 8, (T, N), generator=g)
    adv, ret = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g)
    logp = float(np.log(1 / 8)) + 0.25 * torch.randn(T, N, generator=g)
    src = torch.rand(T, N, 2, generator=g) * 2000 + 200
    cut = (torch.rand(T, N, generator=g) < 0.08).to(torch.uint8)
    cut[-1] = 1
    d = lambda t: t.to(device)
    return pack_episodes(d(obs), d(act), d(adv), d(ret), d(logp), d(src), d(cut), n_total=N, seed=3, sort_by_length=True)


class GruH0:
    """Draws for RNNAgentPPO.a2c_losses when the PFGRU locations are given: only the GRU's initial states."""

    def __init__(self, h0):
        self.h0 = h0

    def gru_h0(self):
        return self.h0


def chain_logp_f64(ac64, X64, loc64, h064, act):
    """log pi(act) of every (step, episode) of a batch under the float64 twin: GRU over the episodes, then the heads."""
    g = ac64.pi.logits_net.v_net.seq_model
    with torch.no_grad():
        hs, _ = g(torch.cat((X64, loc64), dim=2), h064.unsqueeze(0))
        logits, _ = ac64.heads(hs.reshape(-1, hs.shape[-1]))
        lp = torch.log_softmax(logits, dim=-1).view(*act.shape, -1)
    return lp.gather(-1, act.cpu().unsqueeze(-1)).squeeze(-1)


def batch_to(B, device, dtype):
    """An EpisodeBatch with its float columns in dtype on device (integer / bool columns keep their type)."""
    from radiation_ppo_amd.rada2c import EpisodeBatch
    f = lambda t: t.to(device=device, dtype=dtype)
    i = lambda t: t.to(device)
    return EpisodeBatch(X=f(B.X), act=i(B.act), adv=f(B.adv), ret=f(B.ret), logp=f(B.logp), src=f(B.src), valid=i(B.valid), lens=i(B.lens),
                        w_ep=f(B.w_ep), key=i(B.key), lens_host=None if B.lens_host is None else list(B.lens_host))


# ------------------------------------------------------------------------------------------------ PFGRU
def hid_obs_fragile(cell64, mean_hid64, eps):
    """[B, 2] True where an output of hid_obs (Linear(H, 24)-ReLU-Linear(24, 2)-ReLU) on the float64 mean particle is within eps of
    a kink: its own pre-activation, or any of the 24 hidden pre-activations (each feeds both outputs)."""
    z0 = torch.nn.functional.linear(mean_hid64, cell64.hid_obs[0].weight, cell64.hid_obs[0].bias)
    z2 = torch.nn.functional.linear(torch.relu(z0), cell64.hid_obs[2].weight, cell64.hid_obs[2].bias)
    return (z2.abs() < eps) | (z0.abs() < eps).any(dim=-1, keepdim=True)


def pfgru_step_f64(cell64, obs3, h, p, eps, idx):
    """PFGRUCell.forward with given resampling indices in float64: (pred [B, 2], h1 [B, P, H], p1 [B, P], mean_hid [B, H])."""
    with torch.no_grad():
        pred, (h1, p1) = cell64(obs3, (h, p), eps, resample_idx=idx)
        mean = torch.sum(torch.exp(p1).unsqueeze(-1) * h1, dim=1)
    return pred, h1, p1, mean
