#!/usr/bin/env python3
"""Generate tests/golden/bpf_a2c.npz by running the REAL reference's BPF-A2C pieces (algos/test_environment/eval/core.py:
RNNModelActorCritic :440-498 with SeqPt :297-336, ParticleFilter :528-620, FIC.particle_FIM :686-694, StatBuff :53-81) on recorded
draws.

Like make_bpf_fic.py this runs only where the reference is at hand; its output is plain data.  The reference file is imported
unmodified, with make_grad_search.py's placeholder modules and make_bpf_fic.py's ReplayRng.  eval/test_policy.py itself cannot be
imported here (it needs visilibity and statsmodels), so the 'bpf-a2c' closure of its select_model (:109-156) is recorded through the
classes' own methods: `ac.pi._distribution` for the actor (:142), `ParticleFilter.track` for the estimate (:117) and
`FIC.particle_FIM` -- the closure's own expression (:119-126, 146-153) -- for every matrix; the initial bound (:127-135) is
particle_FIM on the filter's xp_init and wp_init with scale @ uni_probs (:362-365) as its scale.

Every case is one filter and one actor walked for STEPS steps: the reading at the detector (Poisson at the inverse-square rate of a
fixed source), StatBuff, track, the standardised and clipped observation (:400, 422), the actor on that observation and the estimate
over the search area's side (:141), the sampled action, and the detector moved by the controller's table (:18-27).  Recorded per
step: reading, detector, the statistics' mean and deviation, the standardised observation [11], the estimate, the actor's normalised
logits, its hidden state before and after, the action, the particles and weights, the matrix at the detector and at each of the 8
sim_step positions; per case the prior's particles, the initial bound and the bound's recursion B_t (:435) with numpy.  The actor's
weights are recorded under their state_dict names.
Cases: NP in {64, 100} x thresh in {1 (resamples at every step), 0.1}.  The clip never bites in a walk this short -- after n readings a
running z-score is at most (n - 1) / sqrt(n) --, so the GPU tests set the statistics themselves to reach it."""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_bpf_fic import ReplayRng  # noqa: E402
from make_grad_search import REF, _install_placeholders  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
STEPS = 6
MOVES = np.array([(-100, 0), (-71, 71), (0, 100), (71, 71), (100, 0), (71, -71), (0, -100), (-71, -71)], dtype=np.float64)
NOISE = [15.0, 1.0, 1]
AREA_MAX = 2200.0                                                  # search_area[2][1] of the 2700 cm box with observation_area [200, 500]


def main():
    _install_placeholders()
    sys.path.insert(0, os.path.join(REF, "algos", "test_environment", "eval"))
    if not hasattr(np, "infty"):
        np.infty = np.inf
    try:
        import visilibity  # noqa: F401
        raise SystemExit("visilibity is installed: record through eval/test_policy.py's own closure instead")
    except ImportError:
        pass
    import torch
    from numpy.linalg import inv
    import core                                                    # the reference's file, unmodified
    scale = np.diag(np.array([1e10, 1, 1]))
    uni_probs = np.diag(np.array([(1 / (1e3 - 1e2)), (1 / (25e2 + 0)), (1 / (25e2 + 0))]))
    sigma = np.array([NOISE[1], NOISE[0], NOISE[0]])
    pro_covar = inv(np.diag(np.square(sigma)))
    ac = core.RNNModelActorCritic(SimpleNamespace(shape=(11,)), SimpleNamespace(n=8), hidden=[24], hidden_sizes_pol=[32], hidden_sizes_rec=[24],
                                  hidden_sizes_val=[32], net_type="rnn", pad_dim=2, batch_s=1, seed=20240611)
    ac.eval()
    out = {"w_" + k: v.detach().numpy().copy() for k, v in ac.state_dict().items() if k.startswith("pi.")}
    cases = [(NP, thresh) for NP in (64, 100) for thresh in (1, 0.1)]
    for c, (NP, thresh) in enumerate(cases):
        src = np.random.default_rng(3000 + c)
        source, inten, bkg = np.array([1300.0, 1000.0]), 600.0, 25
        det = np.array([900.0, 1400.0])
        rng = ReplayRng(src)
        pf = core.ParticleFilter(nParticles=NP, noise_params=NOISE, thresh=thresh, s_size=3, rng=rng, L=1, k=0.0, alpha=0.6, fim_thresh=0.36,
                                 interval=[75, 75], bkg=bkg, scale=scale)
        fic = core.FIC(nParticles=2, bkg=bkg, rng=rng, scale=scale)              # particle_FIM only: it reads self.bkg and self.scale
        stat = core.StatBuff()
        torch.manual_seed(500 + c)
        hidden = ac.pi._reset_state()
        rec = {k: [] for k in ("reading", "det", "mu", "sig", "obs_std", "est", "logp", "h_before", "h_after", "act", "xp", "w", "F_det", "F_sim",
                               "bound")}
        for t in range(STEPS):
            lam = inten * 1e4 / np.sum((det - source) ** 2) + bkg
            reading = float(src.poisson(lam))
            stat.update(reading)
            est = pf.track(np.append(reading, det)).copy()
            obs = np.concatenate(([reading], det / AREA_MAX, src.random(8)))
            obs_std = obs.copy()
            obs_std[0] = np.clip((obs[0] - stat.mu) / stat.sig_obs, -8, 8)
            xp, w = pf.xp_prev[:, t, :], pf.wp_prev[:, t, :]
            fic.scale = scale
            F_det = fic.particle_FIM(det, xp, w, 3)
            if t == 0:
                fic.scale = scale @ uni_probs
                bound = fic.particle_FIM(det, pf.xp_init, pf.wp_init, 3)
                fic.scale = scale
                out[f"c{c}_xp_init"] = pf.xp_init.copy()
            else:
                bound = pro_covar + F_det - np.square(pro_covar) @ inv(rec["bound"][-1] + pro_covar)
            with torch.no_grad():
                x_obs = torch.FloatTensor(np.append(obs_std, est[1:] / AREA_MAX)[None, None, :])
                h0 = hidden.clone()
                dist, hidden, _ = ac.pi._distribution(x_obs, hidden=hidden)
                act = int(dist.sample().item())
            F_sim = np.array([fic.particle_FIM(det + MOVES[a], xp, w, 3) for a in range(8)])
            for k, v in (("reading", reading), ("det", det.copy()), ("mu", float(stat.mu)), ("sig", float(stat.sig_obs)), ("obs_std", obs_std),
                         ("est", est), ("logp", dist.logits.numpy().reshape(-1).copy()), ("h_before", h0.numpy().reshape(-1).copy()),
                         ("h_after", hidden.numpy().reshape(-1).copy()), ("act", act), ("xp", xp.copy()), ("w", w[:, 0].copy()),
                         ("F_det", F_det), ("F_sim", F_sim), ("bound", bound)):
                rec[k].append(v)
            det = det + MOVES[act]
        for k, v in rec.items():
            out[f"c{c}_{k}"] = np.asarray(v)
        out[f"c{c}_meta"] = np.array([NP, thresh, bkg], dtype=np.float64)
    out["params"] = np.array([NOISE[0], NOISE[1], 1e2, 1e3, 0.0, 25e2, AREA_MAX])          # sigma_xy, sigma_I, intensity, coord, area_max
    path = os.path.join(OUT, "bpf_a2c.npz")
    np.savez_compressed(path, **out)
    print("bpf_a2c.npz:", len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
