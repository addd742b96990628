"""Float64 references and the tolerance rule shared by the float64 tests of the sized kernels (test_rnn_sized_f64_gpu.py,
test_pfgru_sized_f64_gpu.py), of the feed-forward PPO kernels and of the RAD-TEAM actor loss and heads (test_cnn_heads_f64_gpu.py), and
their CPU self-checks (test_f64_references.py).

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


# ------------------------------------------------------------------------------------------------ PFGRU training pass (K13)
KINK_EPS = 1e-5                      # a float64 pre-activation this close to 0 may take the other branch in float32


def kink_count(z0, z2, d, valid, eps=KINK_EPS, l1_on=True):
    """Evaluations of hid_obs (one per (step, episode, particle-or-mean)) on valid steps that sit within eps of a kink: one of the 24
    hidden pre-activations z0 [L, E, Q, 24], one of the two output pre-activations z2 [L, E, Q, 2], or (with an L1 term in the loss)
    one of the two errors d = out - tar [L, E, Q, 2], the kink of |.|.  valid [L, E]."""
    near = (z0.abs() < eps).any(dim=-1) | (z2.abs() < eps).any(dim=-1)
    if l1_on:
        near = near | (d.abs() < eps).any(dim=-1)
    return int((near & valid.unsqueeze(-1)).sum())


class ModelLoss64:
    """What model_loss_f64 returns.  loss: the scalar to differentiate; mags: the sum of the absolute per-(step, episode) terms of the
    loss; loc [L, E, 2]: the location outputs; clamped: the fraction of them on valid steps that hid_obs's final ReLU clamps to 0;
    kinks of samples: kink_count of the pass and the hid_obs evaluations it ran over."""
    loss = mags = loc = clamped = kinks = samples = None


# the blocks a parameter gradient is compared in: rows of the layer's output (z | r gates; fc_n: mu rows, then var rows)
BLOCK_ROWS = {"fc_z": (("", slice(None)),), "fc_r": (("", slice(None)),), "fc_n": (("[mu]", slice(0, 24)), ("[var]", slice(24, 48))),
              "fc_obs": (("", slice(None)),), "hid_obs.0": (("", slice(None)),), "hid_obs.2": (("", slice(None)),)}


def grad_blocks(grads):
    """{parameter name: gradient} (PFGRUCell.named_parameters / unpack_train_grads) -> {block name: tensor}."""
    out = {}
    for name, g in grads.items():
        layer, kind = name.rsplit(".", 1)
        for blk, rows in BLOCK_ROWS[layer]:
            out[f"{layer}.{kind}{blk}"] = g[rows]
    return out


def model_loss_f64(cell64, X, tar32, bp32, valid, lens, w_ep, bp_args, pf_h0, eps, idx):
    """RNNAgentPPO.model_loss (rada2c.py: the PFGRU stepped through every episode from p0 = log(1 / 40), then the L2 / L1 regression
    terms on the mean prediction and the ELBO terms on every particle's prediction) written out in float64 with the resampling indices
    given, on the inputs model_pass_hip hands K13: tar32 [L, E, 2] = (src / area_scale).float(), bp32 [L, E] the float32 step
    weights, both widened here, so that the rounding of the inputs is charged to neither side.  X [L, E, >= 3], valid [L, E] bool,
    lens [E], w_ep [E], pf_h0 [E, P, H], eps [L, E, P, H], idx [L, E, P].  The step is PFGRUCell.forward with resample_idx, and hid_obs
    is applied to the 40 particles and their weighted mean together (cell.particle_predictions and the cell's own prediction:
    test_f64_references.py holds this to the cell)."""
    import math
    F = torch.nn.functional
    a = bp_args
    c = cell64
    L, E = X.shape[0], X.shape[1]
    P, H = c.num_particles, c.h_dim
    al = c.resamp_alpha
    X3 = X[..., :3].double()
    tar, bp = tar32.double(), bp32.double()
    h = pf_h0.double()
    p = torch.full((E, P), math.log(1.0 / P), dtype=torch.float64)
    res = ModelLoss64()

    lin = lambda name, layer, x: F.linear(x, layer.weight, layer.bias)
    outs, z0s, z2s = [], [], []
    for t in range(L):
        xin = X3[t].unsqueeze(1).expand(E, P, 3)
        cat = torch.cat((h, xin), dim=2)
        z = torch.sigmoid(lin("fc_z", c.fc_z, cat))
        r = torch.sigmoid(lin("fc_r", c.fc_r, cat))
        n1 = lin("fc_n", c.fc_n, torch.cat((r * h, xin), dim=2))
        n = torch.tanh(n1[..., :H] + eps[t].double() * F.softplus(n1[..., H:]))
        h1 = (1 - z) * n + z * h
        p1 = F.log_softmax(lin("fc_obs", c.fc_obs, torch.cat((h1, xin), dim=2)).squeeze(-1) + p, dim=1)
        ix = idx[t].long()
        h = torch.gather(h1, 1, ix.unsqueeze(-1).expand(E, P, H))
        pn = torch.exp(torch.gather(p1, 1, ix))
        pn = torch.log(pn / (al * pn + (1 - al) / P))
        p = pn - torch.logsumexp(pn, dim=1, keepdim=True)
        mean = torch.sum(torch.exp(p).unsqueeze(-1) * h, dim=1)
        hin = torch.cat((h, mean.unsqueeze(1)), dim=1)                    # [E, P + 1, H]: the particles, then their weighted mean
        z0 = lin("hid_obs.0", c.hid_obs[0], hin)
        z2 = lin("hid_obs.2", c.hid_obs[2], torch.relu(z0))
        outs.append(torch.relu(z2)); z0s.append(z0); z2s.append(z2)
    out = torch.stack(outs)                                               # [L, E, P + 1, 2]
    part, loc = out[:, :, :P], out[:, :, P]
    v = valid.double()
    n_el = (lens * 2).double()
    d_loc = loc - tar
    bp3 = bp.unsqueeze(-1)
    t_l2 = (d_loc ** 2 * bp3).sum(dim=2)                                   # [L, E] per-(step, episode) terms
    t_l1 = 10.0 * (d_loc.abs() * bp3).sum(dim=2) / n_el
    d_part = part - tar.unsqueeze(2)
    bp4 = bp3.unsqueeze(2)
    y2 = torch.exp(-(d_part ** 2) * bp4).mean(dim=2)
    y1 = torch.exp(-d_part.abs() * bp4).mean(dim=2)
    t_l2p = (-(y2.log()) * v.unsqueeze(-1)).sum(dim=2) / n_el
    t_l1p = 10.0 * (-(y1.log()) * v.unsqueeze(-1)).sum(dim=2) / n_el
    terms = w_ep.double() * (a.l2_weight * t_l2 + a.l1_weight * t_l1 + a.elbo_weight * (a.l2_weight * t_l2p + a.l1_weight * t_l1p))
    res.loss = terms.sum()
    with torch.no_grad():
        res.mags = terms.abs().sum()
        res.loc = loc.detach()
        res.clamped = float((loc[valid] == 0).double().mean())
        res.kinks = kink_count(torch.stack(z0s), torch.stack(z2s), torch.cat((d_part, d_loc.unsqueeze(2)), dim=2), valid, KINK_EPS,
                               l1_on=a.l1_weight != 0)
        res.samples = int(valid.sum()) * (P + 1)
    return res


def k13_inputs(B, bp_args):
    """(tar32, bp32) as RNNAgentPPO.model_pass_hip forms them for K13 from an EpisodeBatch (rada2c.py: ppo.py:1067, :1074-1075)."""
    L = B.X.shape[0]
    tt = torch.arange(L, device=B.X.device, dtype=torch.float64).unsqueeze(1)
    bp = torch.exp(bp_args.bp_decay * tt) * B.valid.double()
    bp = (bp / bp.sum(dim=0, keepdim=True)).float()
    return (B.src / bp_args.area_scale).float(), bp


def k13_batch(T, N, seed, ragged=False, sort_by_length=False, device="cpu"):
    """An episode batch for the PFGRU training pass: N envs x T steps; ragged: episodes cut at p = 0.08 with cut[0, k] = 1 forcing a
    one-step episode next to a full-length one (env k + 1 is left uncut); otherwise every env is one episode of T steps."""
    from radiation_ppo_amd.rada2c import pack_episodes
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(T, N, 11, generator=g)
    act = torch.randint(0, 8, (T, N), generator=g)
    z = torch.zeros(T, N)
    src = torch.rand(T, N, 2, generator=g) * 2000 + 200
    cut = torch.zeros(T, N, dtype=torch.uint8)
    if ragged:
        cut = (torch.rand(T, N, generator=g) < 0.08).to(torch.uint8)
        k = min(3, N - 1)
        cut[0, k] = 1
        if k + 1 < N:
            cut[:, k + 1] = 0
    cut[-1] = 1
    d = lambda t: t.to(device)
    return pack_episodes(d(obs), d(act), d(z), d(z), d(z), d(src), d(cut), n_total=N, seed=3, sort_by_length=sort_by_length)


def k13_draws(L, E, seed, P=40, H=24):
    """(pf_h0 [E, P, H], eps [L, E, P, H], idx [L, E, P]) from a torch generator: random resampling indices with, per step, the
    identity at episode 0 and one repeated particle at the last episode (as the recorded-step tests' _indices)."""
    g = torch.Generator().manual_seed(seed)
    pf_h0 = torch.rand(E, P, H, generator=g)
    eps = torch.randn(L, E, P, H, generator=g)
    idx = torch.randint(0, P, (L, E, P), generator=g)
    idx[:, 0] = torch.arange(P)
    if E > 1:
        idx[:, E - 1] = torch.randint(0, P, (L, 1), generator=g).expand(L, P)
    return pf_h0, eps, idx


def k13_cell(cell, seed):
    """The cell's parameters moved off the initialisation (+ 0.05 randn) and hid_obs[2].bias raised by 0.15 (the device of the sized PFGRU test's
    cells: most predictions above hid_obs's final ReLU, some clamped at 0), in place."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in cell.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
        cell.hid_obs[2].bias.add_(0.15)
    return cell


def k13_noise(L, E):
    """The gradient blocks' noise term: 3e-4 of the block's scale at the reference's 120-step episodes in more than one workgroup
    (L E >= 120 x 65), 1e-4 at the small cases (see test_pfgru_default_f64_gpu.py for the terms it covers)."""
    return 3e-4 if L * E >= 120 * 65 else 1e-4


def check_k13_grads(got, ref64, L, E, name, scale=1.0, report=None):
    """Every gradient block of the PFGRU (grad_blocks) within scale x (rtol 1e-4 + k13_noise of the block's own largest element + a
    floor of 2e-6 of the cell's largest gradient element); fc_obs.bias, exactly 0 in exact arithmetic, is held to the floor alone.
    scale: the bound's multiple (0.1 for the float32 library path on the CPU).  No allowance for ReLU / |.| kinks: see
    test_pfgru_default_f64_gpu.py.  report: a list that receives (block, worst error / allowance).  Returns the worst ratio."""
    a, b = grad_blocks(got), grad_blocks(ref64)
    floor = 2e-6 * max(float(v.abs().max()) for v in b.values())
    noise = k13_noise(L, E)
    ratios = []
    for blk in b:
        x, y = a[blk].detach().double().cpu(), b[blk].detach().double().cpu()
        assert x.shape == y.shape and bool(torch.isfinite(x).all()), (name, blk)
        bs = float(y.abs().max())
        allowed = scale * (floor if blk == "fc_obs.bias" else 1e-4 * y.abs() + noise * bs + floor)
        ratios.append((blk, float(((x - y).abs() / allowed).max())))
    if report is not None:
        report.extend(ratios)
    bad = [(blk, round(r, 3)) for blk, r in ratios if not r <= 1.0]        # every block over its allowance is named
    assert not bad, (name, bad)
    return max(r for _, r in ratios)


# (T, N, ragged, sort_by_length, (l2, l1, elbo) weights, seed): the cases of test_pfgru_default_f64_gpu.py, each also run through the
# float32 library path on the CPU (test_f64_references.py; the 65 episodes of 120 steps shrink to 8 there)
K13_CASES = [
    (1, 1, False, False, (1.0, 0.0, 1.0), 1), (1, 1, False, False, (1.0, 0.5, 1.0), 2),
    (1, 70, False, False, (1.0, 0.0, 1.0), 3), (1, 70, False, False, (1.0, 0.5, 1.0), 4),
    (120, 1, False, False, (1.0, 0.0, 1.0), 5), (120, 1, False, False, (1.0, 0.5, 1.0), 6),
    (40, 24, True, False, (1.0, 0.0, 1.0), 7), (40, 24, True, True, (1.0, 0.5, 1.0), 8),
    (40, 24, True, True, (1.0, 0.5, 0.0), 9), (40, 24, True, False, (0.0, 1.0, 1.0), 10),
    (120, 65, False, False, (1.0, 0.0, 1.0), 11), (120, 65, False, True, (1.0, 0.5, 1.0), 12),
]


def k13_case_id(c):
    T, N, ragged, srt, (l2, l1, elbo), seed = c
    return f"T{T}-N{N}{'-ragged' if ragged else ''}{'-sorted' if srt else ''}-l2_{l2:g}-l1_{l1:g}-elbo_{elbo:g}"


def k13_reference(cell, B, bp_args, pf_h0, eps, idx):
    """model_loss_f64 of the float64 twin of `cell` on batch B (any device) with its gradients: (ModelLoss64, {name: grad}, cell64)."""
    c64 = f64(cell)
    Bc = batch_to(B, "cpu", torch.float32)
    tar32, bp32 = k13_inputs(Bc, bp_args)
    res = model_loss_f64(c64, Bc.X, tar32, bp32, Bc.valid, Bc.lens, Bc.w_ep, bp_args, pf_h0.cpu(), eps.cpu(), idx.cpu())
    res.loss.backward()
    return res, {k: p.grad for k, p in c64.named_parameters()}, c64


# ------------------------------------------------------------------------------------------------ feed-forward PPO (K7, rs_policy_forward, K6)
FF_BLOCKS = (("a.w1", 704), ("a.b1", 64), ("a.w2", 4096), ("a.b2", 64), ("a.w3", 512), ("a.b3", 8),
             ("c.w1", 704), ("c.b1", 64), ("c.w2", 4096), ("c.b2", 64), ("c.w3", 64), ("c.b3", 1))     # FusedPPOGrad's order
FF_STATS = ("kl", "entropy", "clipfrac", "value_loss", "loss")
FF_WAVES = 2048                      # K7: 256 workgroups x 8 waves, one group of 32 samples per wave and trip
FF_SIZES = (1, 31, 32, 33, 63, 65, 65536, 65537, 65536 + 32 * 1024 + 5, 3 * 65536 + 32 * 7 + 1)
FF_SCALES = {"base": 0.25, "x3": 0.75}            # parameters = randn x scale
FF_CASES = [(M, "base") for M in FF_SIZES] + [(33, "x3"), (65537, "x3")]
FWD_SIZES = (1, 63, 64, 65, 131072, 131073, 131072 + 64 * 1000 + 1)
FF_CLIP, FF_ALPHA, FF_VF = 0.2, 0.1, 0.01


def ff_case_id(c):
    return f"M{c[0]}-{c[1]}"


def ff_trips(M):
    groups = (M + 31) // 32
    return (groups + FF_WAVES - 1) // FF_WAVES


def ff_tail_start(M):
    """First sample of the tail: the last trip's samples where K7 takes more than one trip, the last (full or partial) group otherwise."""
    t = ff_trips(M)
    return (t - 1) * FF_WAVES * 32 if t > 1 else ((M + 31) // 32 - 1) * 32


def ff_weights(M, g):
    """float32 weights, sum 1 (to float32 rounding): half on the tail, half on the samples before it, each spread as uniform(0.25, 1.75).
    A tail of more than one group that ends in a partial group gives half of its own half to that partial group, so that the few
    samples behind the last full group weigh a quarter of the batch.  M <= 32: the tail is the whole batch."""
    def spread(n, total):
        u = 0.25 + 1.5 * torch.rand(n, generator=g, dtype=torch.float64)
        return u * (total / u.sum())
    s = ff_tail_start(M)
    w = torch.empty(M, dtype=torch.float64)
    if s == 0:
        w[:] = spread(M, 1.0)
        return w.float()
    w[:s] = spread(s, 0.5)
    last = (M - 1) // 32 * 32
    if M % 32 and last > s:
        w[s:last] = spread(last - s, 0.25)
        w[last:] = spread(M - last, 0.25)
    else:
        w[s:] = spread(M - s, 0.5)
    return w.float()


def ff_params(ac):
    """The twelve parameters in FusedPPOGrad's order."""
    return [ac.actor[0].weight, ac.actor[0].bias, ac.actor[2].weight, ac.actor[2].bias, ac.actor[4].weight, ac.actor[4].bias,
            ac.critic[0].weight, ac.critic[0].bias, ac.critic[2].weight, ac.critic[2].bias, ac.critic[4].weight, ac.critic[4].bias]


def ff_agent(pset, seed=0):
    """FFActorCritic on the CPU with parameters randn x FF_SCALES[pset]; "x3" is the same draw as "base" times 3."""
    from radiation_ppo_amd.ppo import FFActorCritic
    g = torch.Generator().manual_seed(1000 + seed)
    ac = FFActorCritic()
    with torch.no_grad():
        for p in ff_params(ac):
            p.copy_(torch.randn(p.shape, generator=g) * FF_SCALES[pset])
    return ac


def ff_forward_f64(ac64, X):
    """(logits [M, 8], value [M]) of the float64 twin on float32 rows widened."""
    with torch.no_grad():
        x = X.double().cpu()
        return ac64.logits(x), ac64.critic(x).squeeze(-1)


class FFLoss64:
    """What ff_loss_f64 returns.  stats [5]: kl, entropy, clip fraction, value loss, loss; stat_mags [5]: the sums of the absolute
    per-sample terms they are rounded against; grads / mags: twelve tensors each in FusedPPOGrad's order, mags[k][e] the sum over samples
    of the absolute per-sample term of gradient element e; bp_mags: the same sums with the back-propagated error delta replaced by its
    bound without cancellation, |W2|^T (|W3|^T |dz| (1 - h2^2)) (1 - h1^2) (zero for the output layer, which has no dot product behind
    it): the scale the rounding of W3^T dz and W2^T dpre2 is relative to; ratio [M]: the float64 PPO ratios."""
    stats = stat_mags = grads = mags = bp_mags = ratio = None

    def flat(self):
        return torch.cat([g.reshape(-1) for g in self.grads]), torch.cat([m.reshape(-1) for m in self.mags])

    def flat_bp(self):
        return torch.cat([m.reshape(-1) for m in self.bp_mags])


def _ff_backward(seq, x, h1, h2, dz):
    """Gradients and their per-element magnitudes of one 11-64-64-NOUT tanh MLP from the error dz [M, NOUT] at its output: for a
    weight, dW = delta^T a and |delta|^T |a| (|delta_i a_j| = |delta_i| |a_j|: no per-sample gradient is formed); for a bias, the
    column sums of delta and of |delta|."""
    W2, W3 = seq[2].weight, seq[4].weight
    d2 = (dz @ W3) * (1 - h2 * h2)
    d1 = (d2 @ W2) * (1 - h1 * h1)
    # the same chain without cancellation in the two transposed dot products: what their rounding errors are relative to
    u2 = (dz.abs() @ W3.abs()) * (1 - h2 * h2)
    u1 = (u2 @ W2.abs()) * (1 - h1 * h1)
    grads, mags, bps = [], [], []
    for d, u, a in ((d1, u1, x), (d2, u2, h1), (dz, None, h2)):
        grads += [d.t() @ a, d.sum(0)]
        mags += [d.abs().t() @ a.abs(), d.abs().sum(0)]
        bps += [torch.zeros_like(mags[-2]), torch.zeros_like(mags[-1])] if u is None else [u.t() @ a.abs(), u.sum(0)]
    return grads, mags, bps


def ff_loss_f64(ac64, X, act, adv, ret, logp_old, w, clip, alpha, vf):
    """The loss of VecAgentPPO.update_agent's unfused branch (ppo.py; test_ppo_gpu._torch_loss_and_grads writes the same):
    -(sum w min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv) - vf sum w (v - ret)^2 + alpha sum w entropy), the entropy term detached,
    on the float64 twin ac64 with the float32 inputs widened (their rounding is charged to neither side), forward and backward written
    out by hand so that the magnitudes come with the gradients (test_f64_references.py holds the gradients to float64 autograd).
    Magnitudes of the statistics: kl sum w (|logp_old| + |logp|); entropy sum w sum_j p_j (1 + |lp_j|) (the error of lp_j is absolute);
    clip fraction itself; value loss sum w (d^2 + 2 |d| (1 + |v| + |ret|)), d = v - ret; loss: sum w |surr| (1 + |logp|) + vf x the
    value loss's + alpha x the entropy's."""
    res = FFLoss64()
    with torch.no_grad():
        x, adv, ret, lpo, w = (t.detach().double().cpu() for t in (X, adv, ret, logp_old, w))
        act = act.detach().cpu().long()
        M = x.shape[0]
        a1 = torch.tanh(torch.nn.functional.linear(x, ac64.actor[0].weight, ac64.actor[0].bias))
        a2 = torch.tanh(torch.nn.functional.linear(a1, ac64.actor[2].weight, ac64.actor[2].bias))
        lp_all = torch.log_softmax(torch.nn.functional.linear(a2, ac64.actor[4].weight, ac64.actor[4].bias), dim=-1)
        c1 = torch.tanh(torch.nn.functional.linear(x, ac64.critic[0].weight, ac64.critic[0].bias))
        c2 = torch.tanh(torch.nn.functional.linear(c1, ac64.critic[2].weight, ac64.critic[2].bias))
        v = torch.nn.functional.linear(c2, ac64.critic[4].weight, ac64.critic[4].bias).squeeze(-1)
        p = lp_all.exp()
        logp = lp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1)
        ratio = torch.exp(logp - lpo)
        lo, hi = 1 - clip, 1 + clip
        s1, s2 = ratio * adv, torch.clamp(ratio, lo, hi) * adv
        surr = torch.minimum(s1, s2)
        live = ((ratio >= lo) & (ratio <= hi)) | (s1 < s2)                 # where the minimum is the unclipped term: d surr / d ratio = adv
        g_lp = -w * torch.where(live, adv, torch.zeros_like(adv)) * ratio    # d loss / d logp
        onehot = torch.zeros(M, 8, dtype=torch.float64).scatter_(1, act.unsqueeze(-1), 1.0)
        dz_a = g_lp.unsqueeze(-1) * (onehot - p)
        d = v - ret
        dz_c = (2 * vf * w * d).unsqueeze(-1)
        ga, ma, ba = _ff_backward(ac64.actor, x, a1, a2, dz_a)
        gc, mc, bc = _ff_backward(ac64.critic, x, c1, c2, dz_c)
        res.grads, res.mags, res.bp_mags = ga + gc, ma + mc, ba + bc
        ent_s = -(p * lp_all).sum(-1)
        kl, ent, cf, vl, sur = (w * (lpo - logp)).sum(), (w * ent_s).sum(), (w * ((ratio > hi) | (ratio < lo)).double()).sum(), \
            (w * d * d).sum(), (w * surr).sum()
        res.stats = torch.stack([kl, ent, cf, vl, -(sur - vf * vl + alpha * ent)])
        m_ent = (w * (p * (1 + lp_all.abs())).sum(-1)).sum()
        m_vl = (w * (d * d + 2 * d.abs() * (1 + v.abs() + ret.abs()))).sum()
        m_sur = (w * surr.abs() * (1 + logp.abs())).sum()
        res.stat_mags = torch.stack([(w * (lpo.abs() + logp.abs())).sum(), m_ent, cf, m_vl, m_sur + vf * m_vl + alpha * m_ent])
        res.ratio = ratio
    return res


def _ff_forward_terms(s1, s2, s3):
    """(E_h1, E_h2, E_out) of ff_error_model, in U and before SAFETY, for layers whose parameters have rms s1, s2, s3."""
    S1 = 12 * s1 * 0.8                                 # sum |w1 x| + |b1|: depth 11 + 1
    E_h1 = (12 ** 0.5 + 1) * S1 + 4                    # layer 1 dot (11 + 1 deep, MFMA k-chain) + tanh
    S2 = 65 * s2                                       # sum |w2 h1| + |b2| <= 65 s: depth 64 (+ bias)
    E_h2 = 8 * s2 * E_h1 + (8 + 1) * S2 + 4            # h1's error through W2, layer 2 dot, tanh
    S3 = 65 * s3
    E_out = 8 * s3 * E_h2 + (8 + 1) * S3 + 1           # h2's error through W3, the 2 x 32 fmaf chains + pair add + bias (depth 64)
    return E_h1, E_h2, E_out


def _ff_lp_term(E_out):
    # log-probabilities: (out - mx) - lse with lse = __logf(sum of eight __expf): two logits' errors, the two subtractions (2), the
    # eight-term sum (sqrt(8) + 1 on terms <= 1), __expf 1 + its argument's scaling (terms near 1: <= 1), __logf 1 + 1
    return 2 * E_out + 2 + 3.8 + 2 + 2


def ff_error_model(pset):
    """The float32 error model of the feed-forward kernels, in units of U, for parameters randn x s (s = FF_SCALES[pset]) and
    standard-normal inputs (E|x| = 0.8, |tanh| <= 1), term by term after the module docstring: a dot product of depth n carries
    sqrt(n) U of the sum of its absolute terms in expectation, plus 1 U of that sum for the rounding of the 2 log2(e) prescale folded
    into W1 / b1 / W2 / b2; rs_tanh_scaled adds 4 U absolute (v_exp_f32 1, the scaling of its argument <= 0.5: |x| sech^2 x <= 0.45,
    1 + e 0.5, v_rcp_f32 1, fma 0.5, rounded up) and passes the pre-activation's error on with tanh' <= 1; an error e of the inputs of a
    dot product of depth n with weights of rms s comes out as sqrt(n) s e (independent signs).  E|tanh'| over the units (gain) is 0.5
    at s = 0.25 (pre-activations of std ~1.2) and 0.15 at s = 0.75 (std ~5: most units saturated); 1 / gain is what the relative error
    of 1 - h^2 costs per unit of the error of h, summed over samples.  SAFETY multiplies everything: the model is an expectation.

    Returns E_logit (absolute error of a logit or of the value, in U), and k, the multiple of U mag every gradient element and every
    statistic is allowed (see test_ppo_ff_f64_gpu.py's docstring for the backward terms)."""
    s = FF_SCALES[pset]
    gain = {"base": 0.5, "x3": 0.15}[pset]
    SAFETY = 2.0
    E_h1, E_h2, E_out = _ff_forward_terms(s, s, s)
    E_lp = _ff_lp_term(E_out)
    # p_j = __expf(lp_j): relative E_lp + 1 + |lp_j| (argument scaling at lp ~ -20: 20; such p_j are 2e-9 and weigh nothing: kept)
    E_p = E_lp + 21
    # ratio = __expf(logp - lpo): E_lp + subtraction 1 + __expf 1 + |logp - lpo| < 1;  g_lp = -w dr ratio: 2 products
    E_glp = E_lp + 3 + 2
    E_dz = E_glp + E_p + 1                             # dz_j = g_lp (1[a = j] - p_j)
    # dpre2 = (W3^T dz) (1 - h2^2): h2's error in 1 - h2^2 (2 E_h2 / gain), the fma pair (3);  dW2's term dpre2 h1 adds h1's error
    # (relative to E|h1| ~ 0.5).  dpre1 = (W2^T dpre2) (1 - h1^2): 2 E_h1 / gain, 3;  dW1's term dpre1 x: x is exact.
    # The rounding of the two transposed dot products themselves (depth 8 and 64) is relative to the sum of their ABSOLUTE terms, not to
    # their result: over many samples the two differ by ~sqrt(depth), but at a lone sample (M = 1, or a tail of one sample that holds
    # half of the weight) the unit whose 64 terms cancel best decides a whole row of dW1.  It is therefore charged to bp_mag, the
    # magnitude without cancellation, at FF_K_BP = SAFETY (sqrt(64) + 1), and not to k.
    E_d2 = E_dz + 2 * E_h2 / gain + 3
    E_d1 = E_d2 + 2 * E_h1 / gain + 3
    # sums over samples: a wave's MFMA accumulators over trips x 32 <= 128 samples (sqrt(128) = 11.3), the 8-wave LDS sum (2.8), the
    # 256 slabs as 16 chunks of 16 (4 + 4);  float32 torch on the CPU sums M <= 2e5 samples in its GEMM's blocks: its sqrt(M) <= 444
    # sits inside what SAFETY adds to the forward terms (>= 2000 U at either parameter set)
    E_sum = 11.3 + 2.8 + 8
    k = SAFETY * (E_d1 + 2 * E_h2 + E_sum)             # + h2's / h1's relative error in the dW3 / dW2 term (E_h / 0.5)
    return dict(E_h1=E_h1, E_h2=E_h2, E_logit=SAFETY * E_out, E_lp=SAFETY * E_lp, k=k)


FF_K_BP = 2.0 * (64 ** 0.5 + 1)      # see ff_error_model: the transposed dot products' own rounding, on bp_mags
FF_RTOL = 4 * U                      # the roundings that are relative to the result itself: the last add of the slab sum and the bucket store
FF_TINY = 1e-30                      # 2^-126 x 1e8: products of w ~ 1e-6 and small factors may pass through float32's subnormal range


def ff_ratios(got_stats, got_grads, ref, pset):
    """[(block, worst |got - ref| / allowed)] over the five statistics and the twelve gradient blocks, allowed = FF_RTOL |ref| +
    k U mag + FF_TINY with k = ff_error_model(pset)['k'], where a gradient's k U mag is U (k mag + FF_K_BP bp_mag).  got_grads: flat [10441] or the twelve tensors."""
    k = ff_error_model(pset)["k"]
    out = []
    gs = torch.as_tensor(got_stats).detach().double().cpu().reshape(5)
    for q, name in enumerate(FF_STATS):
        allowed = FF_RTOL * abs(float(ref.stats[q])) + k * U * float(ref.stat_mags[q]) + FF_TINY
        err = abs(float(gs[q]) - float(ref.stats[q]))
        out.append((name, err / allowed if err == err else float("inf")))
    if not torch.is_tensor(got_grads):
        got_grads = torch.cat([g.reshape(-1) for g in got_grads])
    gg = got_grads.detach().double().cpu().reshape(-1)
    rg, rm = ref.flat()
    assert gg.shape == rg.shape, (gg.shape, rg.shape)
    ratio = (gg - rg).abs() / (FF_RTOL * rg.abs() + U * (k * rm + FF_K_BP * ref.flat_bp()) + FF_TINY)
    ratio = torch.where(torch.isfinite(gg), ratio, torch.full_like(ratio, float("inf")))
    o = 0
    for name, n in FF_BLOCKS:
        out.append((name, float(ratio[o:o + n].max())))
        o += n
    return out


def check_ff(got_stats, got_grads, ref, pset, name, report=None):
    """Every statistic and gradient block within the rule (ff_ratios); every block over its allowance is named.  report: a list that
    receives a line `name | block ratio ...`."""
    ratios = ff_ratios(got_stats, got_grads, ref, pset)
    if report is not None:
        report.append(f"{name} | " + " ".join(f"{b} {r:.4f}" for b, r in ratios))
    bad = [(b, round(r, 3)) for b, r in ratios if not r <= 1.0]
    assert not bad, (name, bad)
    return ratios


class FFCase:
    pass


_FF_CACHE = {}


def ff_case(M, pset, zero_rows=0):
    """One case of the K7 tests, built once on the CPU and shared: the float32 agent `ac`, its float64 twin, the float32 batch
    (X, act, adv, ret, lpo, w) and the float64 reference `ref`.  adv / ret are randn; logp_old = logp64(act) - log(target ratio), rounded
    to float32, targets from target_ratios (a third below, inside, above the clip range, 0.02 off its edges); asserted: no sample's
    float64 ratio from the ROUNDED logp_old lies within 0.01 of 1 +- clip (a condition, not an allowance: zero samples are excused).
    zero_rows: that many scattered rows get w = 0, X x 1e3 and adv x 1e6 (all finite), the other weights are renormalised; the
    reference is computed with those rows deleted."""
    key = (M, pset, zero_rows)
    if key in _FF_CACHE:
        return _FF_CACHE[key]
    c = FFCase()
    g = torch.Generator().manual_seed(7 * M + len(pset) + zero_rows)
    c.M, c.pset = M, pset
    c.ac = ff_agent(pset)
    c.ac64 = f64(c.ac)
    c.X = torch.randn(M, 11, generator=g)
    c.act = torch.randint(0, 8, (M,), generator=g)
    c.adv, c.ret = torch.randn(M, generator=g), torch.randn(M, generator=g)
    c.w = ff_weights(M, g)
    keep = torch.ones(M, dtype=torch.bool)
    if zero_rows:
        dead = torch.randperm(M, generator=g)[:zero_rows]
        keep[dead] = False
        c.X[dead] *= 1e3
        c.adv[dead] *= 1e6
        c.w[dead] = 0.0
        c.w = (c.w.double() / c.w.double().sum()).float()
    lg, _ = ff_forward_f64(c.ac64, c.X)
    lp64 = torch.log_softmax(lg, dim=-1).gather(-1, c.act.unsqueeze(-1)).squeeze(-1)
    c.lpo = (lp64 - torch.log(target_ratios(M, g, FF_CLIP))).float()
    c.keep = keep
    c.batch = (c.X, c.act, c.adv, c.ret, c.lpo, c.w)
    c.ref = ff_loss_f64(c.ac64, *(t[keep] for t in c.batch), FF_CLIP, FF_ALPHA, FF_VF)
    r = torch.exp(lp64 - c.lpo.double())
    assert float(torch.minimum((r - (1 - FF_CLIP)).abs(), (r - (1 + FF_CLIP)).abs()).min()) >= 0.01, "a ratio within 0.01 of a clip edge"
    assert bool(torch.isfinite(c.X).all()) and bool(torch.isfinite(c.adv).all()) and bool(torch.isfinite(c.lpo).all())
    _FF_CACHE[key] = c
    return c


def ff_torch32(c, rows=None):
    """The project's float32 torch path on the CPU for case c (FFActorCritic.evaluate + the loss, autograd): (stats [5], flat gradients).
    rows: a boolean mask of the samples to keep (c.keep where the case has zero-weight rows, which the reference is computed without)."""
    ac = copy.deepcopy(c.ac)
    X, act, adv, ret, lpo, w = c.batch if rows is None else (t[rows] for t in c.batch)
    logp, v, ent = ac.evaluate(X, act)
    ratio = torch.exp(logp - lpo)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1 - FF_CLIP, 1 + FF_CLIP) * adv)
    vl = (w * (v - ret) ** 2).sum()
    loss = -((w * surr).sum() - FF_VF * vl + FF_ALPHA * (w * ent).sum().detach())
    loss.backward()
    clipped = (ratio > 1 + FF_CLIP) | (ratio < 1 - FF_CLIP)
    stats = torch.stack([(w * (lpo - logp)).sum(), (w * ent).sum(), (w * clipped.float()).sum(), vl, loss]).detach()
    return stats, torch.cat([p.grad.reshape(-1) for p in ff_params(ac)])


# nn.Linear's default initialisation, uniform(+-1 / sqrt(fan_in)), has rms 1 / sqrt(3 fan_in); the collector test multiplies it by 3
K6_INIT_SCALES = (3 / 33 ** 0.5, 3 / 192 ** 0.5, 3 / 192 ** 0.5)       # 0.52 for the 11-input layer, 0.22 for the two 64-input layers


def fwd_tolerance(pset):
    """close()'s constants for a logit, a value, a log-probability from the forward half of the model: rtol 4 U (the output's own
    roundings), no noise term, tiny = the absolute error E_logit U (E_lp U for a log-probability).  pset: a parameter set's name, or
    the three layers' rms scales (the same terms and the same SAFETY = 2, with each layer's own scale)."""
    if isinstance(pset, str):
        m = ff_error_model(pset)
    else:
        E_out = _ff_forward_terms(*pset)[2]
        m = dict(E_logit=2.0 * E_out, E_lp=2.0 * _ff_lp_term(E_out))
    return dict(rtol=4 * U, noise=0.0, tiny=m["E_logit"] * U), dict(rtol=4 * U, noise=0.0, tiny=m["E_lp"] * U)


def close_ratio(got, ref, rtol, noise, tiny):
    """close()'s worst error / allowance, as a number (for the results file)."""
    a, b = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(b.abs().max()) if b.numel() else 0.0
    return float(((a - b).abs() / (rtol * b.abs() + noise * scale + tiny)).max()) if b.numel() else 0.0


# ------------------------------------------------------------------------------------------------ RAD-TEAM actor loss, heads (rs_cnn_loss.hip)
AL_SIZES = (1, 63, 64, 65, 255, 256, 257, 577)     # the edges of a 64-lane wave and of a 256-lane block; 577 = 2 x 256 + 64 + 1
AL_CLIPS = (0.2, 0.1)
AL_CASES = [(S, clip) for S in AL_SIZES for clip in AL_CLIPS]
AL_ZERO = (257, 0.2, 40)             # the zero-weight-rows case: (S, clip, rows with w = 0)
AL_STATS = ("kl", "entropy", "clipfrac", "loss")
HEAD_SIZES = (1, 63, 64, 65, 130)
HEAD_AGENTS = 3
HEAD_K2 = 2.0 * (33 ** 0.5 + 1)      # SAFETY x a sequential fmaf chain of depth 32 behind the bias (+ 1: the result's own rounding), on mag2
HEAD_K3 = 2.0 * (17 ** 0.5 + 1)      # the same for the chain of depth 16, on mag3


def al_case_id(c):
    return f"S{c[0]}-clip{c[1]:g}"


def wave_start(S):
    """First sample of the last 64-lane wave of rs_actor_loss (full or partial)."""
    return (S + 63) // 64 * 64 - 64


def wave_weights(S, g):
    """ff_weights with the 64-lane wave as the group: float32 weights, sum 1, half of it on the last wave (full or partial), half on
    the samples before it, each half spread as uniform(0.25, 1.75).  S <= 64: the one wave is the whole batch."""
    def spread(n, total):
        u = 0.25 + 1.5 * torch.rand(n, generator=g, dtype=torch.float64)
        return u * (total / u.sum())
    s = wave_start(S)
    w = torch.empty(S, dtype=torch.float64)
    if s == 0:
        w[:] = spread(S, 1.0)
    else:
        w[:s] = spread(s, 0.5)
        w[s:] = spread(S - s, 0.5)
    return w.float()


def bootstrap_mask(N, g):
    """The bootstrap round's env mask [N] uint8 of the collector tests: p = 0.5, env 0 set, env 1 clear; past 128 envs one whole
    64-group (64..127) is left without a masked env and the last env is set."""
    mask = (torch.rand(N, generator=g) < 0.5).to(torch.uint8)
    mask[0] = 1
    if N > 1:
        mask[1] = 0
    if N > 128:
        mask[64:128] = 0
        mask[N - 1] = 1
    return mask


class ActorLoss64:
    """What actor_loss_f64 returns.  stats [4]: kl, entropy, clip fraction, loss; stat_mags [4]: the sums of the absolute per-sample
    terms they are rounded against (ff_loss_f64's, without the value-loss and alpha parts); dlogits [S, 8] and dl_mags [S, 8] =
    |g_lp| (1[a = j] + p_j); ratio [S]: the float64 PPO ratios."""
    stats = stat_mags = dlogits = dl_mags = ratio = None


def actor_loss_f64(logits, act, adv, logp_old, w, clip):
    """compute_loss_pi behind the logits (the unfused branch of CNNAgentPPO.update_agent: loss = -sum w min(ratio adv, clamp(ratio, 1 -
    clip, 1 + clip) adv), statistics kl = sum w (logp_old - logp), sum w entropy, sum w [ratio outside the clip range]) on the float32
    inputs widened, forward and backward written out by hand as ff_loss_f64 does behind its forward pass (test_f64_references.py
    holds dlogits to float64 autograd): live = inside | (s1 < s2), g_lp = -w live adv ratio, d_j = g_lp (1[a = j] - p_j)."""
    res = ActorLoss64()
    with torch.no_grad():
        lg, adv, lpo, w = (t.detach().double().cpu() for t in (logits, adv, logp_old, w))
        act = act.detach().cpu().long()
        S = lg.shape[0]
        lp_all = torch.log_softmax(lg, dim=-1)
        p = lp_all.exp()
        logp = lp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1)
        ratio = torch.exp(logp - lpo)
        lo, hi = 1 - clip, 1 + clip
        s1, s2 = ratio * adv, torch.clamp(ratio, lo, hi) * adv
        surr = torch.minimum(s1, s2)
        live = ((ratio >= lo) & (ratio <= hi)) | (s1 < s2)
        g_lp = -w * torch.where(live, adv, torch.zeros_like(adv)) * ratio
        onehot = torch.zeros(S, 8, dtype=torch.float64).scatter_(1, act.unsqueeze(-1), 1.0)
        res.dlogits = g_lp.unsqueeze(-1) * (onehot - p)
        res.dl_mags = g_lp.abs().unsqueeze(-1) * (onehot + p)
        cf = (w * ((ratio > hi) | (ratio < lo)).double()).sum()
        res.stats = torch.stack([(w * (lpo - logp)).sum(), (w * -(p * lp_all).sum(-1)).sum(), cf, -(w * surr).sum()])
        res.stat_mags = torch.stack([(w * (lpo.abs() + logp.abs())).sum(), (w * (p * (1 + lp_all.abs())).sum(-1)).sum(), cf,
                                     (w * surr.abs() * (1 + logp.abs())).sum()])
        res.ratio = ratio
    return res


class ALCase:
    pass


_AL_CACHE = {}


def al_case(S, clip, zero_rows=0):
    """One case of the rs_actor_loss tests, built once on the CPU and shared: float32 logits = randn x 1.5, act, adv = randn, w =
    wave_weights, logp_old = logp64(act) - log(target ratio) rounded to float32 with the targets of target_ratios(S, g, clip, margin =
    0.02), as ff_case builds it.  The LAST sample's advantage gets the sign that leaves its gate live (ratio above the range: adv < 0,
    below it: adv > 0): where the last wave is that one sample (S = 65, 257, 577) a lost wave must show in dlogits, which a clipped
    sample's zero row would hide.  Asserted (conditions, not allowances): no float64 ratio from the ROUNDED logp_old within 0.01 of
    1 +- clip; every input finite; S >= 63: all three ratio regions and both advantage signs occur.
    zero_rows: that many scattered rows get w = 0 and adv x 1e6 (finite), the other weights are renormalised; the reference is
    computed with those rows deleted (c.keep)."""
    key = (S, clip, zero_rows)
    if key in _AL_CACHE:
        return _AL_CACHE[key]
    c = ALCase()
    g = torch.Generator().manual_seed(11 * S + int(round(1000 * clip)) + zero_rows)
    c.S, c.clip = S, clip
    c.logits = torch.randn(S, 8, generator=g) * 1.5
    c.act = torch.randint(0, 8, (S,), generator=g)
    c.adv = torch.randn(S, generator=g)
    c.w = wave_weights(S, g)
    target = target_ratios(S, g, clip, margin=0.02)
    if float(target[-1]) > 1 + clip:
        c.adv[-1] = -c.adv[-1].abs()
    elif float(target[-1]) < 1 - clip:
        c.adv[-1] = c.adv[-1].abs()
    keep = torch.ones(S, dtype=torch.bool)
    if zero_rows:
        dead = torch.randperm(S, generator=g)[:zero_rows]
        keep[dead] = False
        c.adv[dead] *= 1e6
        c.w[dead] = 0.0
        c.w = (c.w.double() / c.w.double().sum()).float()
    lp64 = torch.log_softmax(c.logits.double(), dim=-1).gather(-1, c.act.unsqueeze(-1)).squeeze(-1)
    c.lpo = (lp64 - torch.log(target)).float()
    c.keep = keep
    c.batch = (c.logits, c.act, c.adv, c.lpo, c.w)
    c.ref = actor_loss_f64(*(t[keep] for t in c.batch), clip)
    r = torch.exp(lp64 - c.lpo.double())
    assert float(torch.minimum((r - (1 - clip)).abs(), (r - (1 + clip)).abs()).min()) >= 0.01, "a ratio within 0.01 of a clip edge"
    assert all(bool(torch.isfinite(t).all()) for t in (c.logits, c.adv, c.lpo, c.w))
    if S >= 63:
        assert bool((r < 1 - clip).any()) and bool((r > 1 + clip).any()) and bool(((r > 1 - clip) & (r < 1 + clip)).any()), "a ratio region is empty"
        assert bool((c.adv > 0).any()) and bool((c.adv < 0).any())
    c.spread = float((c.logits.max(dim=-1).values - c.logits.min(dim=-1).values).max())
    _AL_CACHE[key] = c
    return c


def al_spread():
    """The largest logit spread max_j lg_j - min_j lg_j over every case of the rs_actor_loss tests (AL_CASES and AL_ZERO)."""
    return max([al_case(S, clip).spread for S, clip in AL_CASES] + [al_case(*AL_ZERO).spread])


def actor_error_model(spread):
    """The float32 error model of rs_actor_loss in units of U: the E_lp, E_p, E_glp, E_dz lines of ff_error_model with E_out = 0 (the
    logits are inputs, exact), at its SAFETY = 2, plus the rounding of lg_j - mx, up to 0.5 ulp of the largest logit spread <= spread
    U absolute (the feed-forward cases keep |lg - mx| near 1 and count it as 1).  k_dl: the multiple of U |g_lp| (1[a = j] + p_j) an
    element of dlogits is allowed; k_stat: the same per-sample term plus the 64-lane butterfly that forms a wave's row of stats, depth
    6, one rounding of the partial sum per level (the host adds the rows in float64: nothing)."""
    SAFETY = 2.0
    E_lp = _ff_lp_term(0.0) + spread
    E_p = E_lp + 21
    E_glp = E_lp + 3 + 2
    E_dz = E_glp + E_p + 1
    return dict(E_lp=SAFETY * E_lp, k_dl=SAFETY * E_dz, k_stat=SAFETY * (E_dz + 6))


def actor_ratios(got_stats, got_dl, ref, model=None):
    """[(block, worst |got - ref| / allowed)] over the four statistics and dlogits (left out when got_dl is None), allowed = FF_RTOL |ref|
    + k U mag + FF_TINY with k = actor_error_model(al_spread())'s k_stat / k_dl."""
    m = model or actor_error_model(al_spread())
    out = []
    gs = torch.as_tensor(got_stats).detach().double().cpu().reshape(4)
    for q, name in enumerate(AL_STATS):
        allowed = FF_RTOL * abs(float(ref.stats[q])) + m["k_stat"] * U * float(ref.stat_mags[q]) + FF_TINY
        err = abs(float(gs[q]) - float(ref.stats[q]))
        out.append((name, err / allowed if err == err else float("inf")))
    if got_dl is not None:
        gd = got_dl.detach().double().cpu()
        assert gd.shape == ref.dlogits.shape, (gd.shape, ref.dlogits.shape)
        ratio = (gd - ref.dlogits).abs() / (FF_RTOL * ref.dlogits.abs() + m["k_dl"] * U * ref.dl_mags + FF_TINY)
        ratio = torch.where(torch.isfinite(gd), ratio, torch.full_like(ratio, float("inf")))
        out.append(("dlogits", float(ratio.max())))
    return out


def check_actor(got_stats, got_dl, ref, name, report=None):
    """Every statistic and dlogits within the rule (actor_ratios); every block over its allowance is named.  report: a list that
    receives a line `name | block ratio ...`."""
    ratios = actor_ratios(got_stats, got_dl, ref)
    if report is not None:
        report.append(f"{name} | " + " ".join(f"{b} {r:.4f}" for b, r in ratios))
    bad = [(b, round(r, 3)) for b, r in ratios if not r <= 1.0]
    assert not bad, (name, bad)
    return ratios


def actor_torch32(logits, act, adv, lpo, w, clip):
    """The unfused branch of CNNAgentPPO.update_agent behind the logits, as ppo_cnn.py writes it, in the inputs' dtype on their
    device: (stats [4] = kl, entropy, clip fraction, loss; d loss / d logits by autograd)."""
    lg = logits.detach().clone().requires_grad_(True)
    logp_all = torch.log_softmax(lg, dim=-1)
    logp = logp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1)
    ratio = torch.exp(logp - lpo)
    clip_adv = torch.clamp(ratio, 1 - clip, 1 + clip) * adv
    loss = -(w * torch.min(ratio * adv, clip_adv)).sum()
    loss.backward()
    with torch.no_grad():
        ent = -(logp_all.exp() * logp_all).sum(-1)
        clipped = (ratio > 1 + clip) | (ratio < 1 - clip)
        stats = torch.stack([(w * (lpo - logp)).sum(), (w * ent).sum(), (w * clipped.to(w.dtype)).sum(), loss.detach()])
    return stats, lg.grad


def cnn_head_f64(seq64, y1):
    """Layers [7:11] of CNNActor.actor / CNNCritic.critic (ReLU, Linear(32, 16), ReLU, Linear(16, OUT)) of the float64 twin seq64 on a
    float32 y1 [N, 32] widened: (out [N, OUT], mag3 = |W3| h2 + |b3|, carried = |W3| mag2 with mag2 = |W2| relu(y1) + |b2|) -- the
    sums of absolute terms the output layer's and the hidden layer's dot products are rounded against, the latter carried through
    |W3| (ReLU passes an error on with slope <= 1)."""
    with torch.no_grad():
        W2, b2, W3, b3 = seq64[8].weight, seq64[8].bias, seq64[10].weight, seq64[10].bias
        h1 = torch.relu(y1.detach().double().cpu())
        h2 = torch.relu(h1 @ W2.t() + b2)
        out = h2 @ W3.t() + b3
        mag2 = h1 @ W2.abs().t() + b2.abs()
        return out, h2 @ W3.abs().t() + b3.abs(), mag2 @ W3.abs().t()


def head_ratio(got, out64, mag3, carried):
    """Worst |got - ref| / (FF_RTOL |ref| + U (HEAD_K2 carried + HEAD_K3 mag3) + FF_TINY) over the outputs of a head."""
    a = got.detach().double().cpu().reshape(out64.shape)
    ratio = (a - out64).abs() / (FF_RTOL * out64.abs() + U * (HEAD_K2 * carried + HEAD_K3 * mag3) + FF_TINY)
    ratio = torch.where(torch.isfinite(a), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max()) if ratio.numel() else 0.0


def draw_ratios(act, logp, act64, lp64, cdf64, u):
    """check_draw's two rules as numbers: (edge, logp, differing).  edge: over the lanes whose action differs from the float64 draw, the
    largest distance of the uniform from its nearest CDF step / the 1e-5 inside which a differing draw is excused (0 when none
    differs); logp: the worst error / (1e-5 |ref| + 5e-6) on the lanes with the same action; differing: their number (<= 2 allowed)."""
    act, logp, u = act.cpu(), logp.cpu(), u.cpu()
    dist = (cdf64[:, :-1] - u.double().unsqueeze(-1)).abs().amin(dim=1)
    same = act == act64
    edge = float(dist[~same].max()) / 1e-5 if bool((~same).any()) else 0.0
    ref = lp64.gather(-1, act64.unsqueeze(-1)).squeeze(-1)
    lp = close_ratio(logp[same], ref[same], rtol=1e-5, noise=0.0, tiny=5e-6)
    return edge, lp, int((~same).sum())


class HeadCase:
    pass


_HEAD_CACHE = {}


def head_case(N, A=HEAD_AGENTS):
    """One case of the rs_cnn_head tests, built once on the CPU and shared.  Every agent has its own CNNActor (the layers behind the
    first Linear x 3: visibly non-uniform policies, as in the collector test) and its own CNNCritic, its own y1 = randn x 2 (both
    ReLUs gate both ways) for either, and its own column of u [N, A]; mask: bootstrap_mask.  actor_ref[a] = (logits64, mag3, carried,
    act64, lp64, cdf64), critic_ref[a] = (value64 [N], mag3 [N], carried [N])."""
    if (N, A) in _HEAD_CACHE:
        return _HEAD_CACHE[(N, A)]
    from radiation_ppo_amd.maps import CNNActor, CNNCritic
    c = HeadCase()
    c.N, c.A = N, A
    g = torch.Generator().manual_seed(1000 * N + A)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(500 + N)
        c.actors, c.critics = [CNNActor() for _ in range(A)], [CNNCritic() for _ in range(A)]
    with torch.no_grad():
        for ac in c.actors:
            for p in ac.actor[7:].parameters():
                p.mul_(3.0)
    c.y1a, c.y1c = torch.randn(A, N, 32, generator=g) * 2, torch.randn(A, N, 32, generator=g) * 2
    c.u = torch.rand(N, A, generator=g)
    c.mask = bootstrap_mask(N, g)
    c.actor_ref, c.critic_ref = [], []
    for a in range(A):
        out, mag3, car = cnn_head_f64(f64(c.actors[a].actor), c.y1a[a])
        c.actor_ref.append((out, mag3, car) + tuple(draw_f64(out, c.u[:, a])))
        v, m3, cr = cnn_head_f64(f64(c.critics[a].critic), c.y1c[a])
        c.critic_ref.append((v.squeeze(-1), m3.squeeze(-1), cr.squeeze(-1)))
    assert bool(torch.isfinite(c.y1a).all()) and bool(torch.isfinite(c.y1c).all())
    _HEAD_CACHE[(N, A)] = c
    return c
