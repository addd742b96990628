#!/usr/bin/env python3
"""Generate tests/golden/bpf_fic.npz by running the REAL reference's bootstrap particle filter and RID-FIM controller
(algos/test_environment/eval/core.py: ParticleFilter :528-620, FIC :655-764, ssp :767-799) on recorded draws.

Like make_grad_search.py this runs only where the reference is at hand; its output is plain data.  The reference file is imported
unmodified, with make_grad_search.py's placeholder modules (numba's jit as the identity, so ssp runs as plain Python; gym's spaces as
empty classes).  Two things are set from outside, neither in the reference's file: `np.infty` (the reference's spelling, gone from
numpy 2) is made a name for np.inf, and `core.ssp` is wrapped by a function that records its arguments and result.

The filter's rng is ReplayRng: uniform(low, high, size) returns low + (high - low) * u and normal(loc, scale, size) loc + scale * z
for recorded arrays u in [0, 1) and z standard normal, so tests/_bpf_ref.py consumes the same u and z.

Every case is a FIC with L = 1 walked for STEPS steps: track on the reading at the detector, then the controller over eight candidate
positions (the look-ahead stood in by a table: the move's offset, or the current position where the case blocks the move), then the
detector moves to the chosen candidate.  Recorded per step: reading, detector, candidates, the latch before and after, the draws, the
particles after the prior / process model and after the step, weights, estimate, nEff, ssp's weights, uniforms and indices (where it
ran), renyi_div and trace(particle_FIM) of all eight moves by the class's own methods, and optim_action's action and score.
Cases: NP in {64, 100} x thresh in {1 (resamples at every step), 0.1}; readings below 76 (the z window is cut at 1) and above; blocked
moves at steps 1 and 3; `near` cases start beside the source, where the Renyi divergence passes fim_thresh and the latch falls."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_grad_search import REF, _install_placeholders  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
STEPS = 6
MOVES = np.array([(-100, 0), (-71, 71), (0, 100), (71, 71), (100, 0), (71, -71), (0, -100), (-71, -71)], dtype=np.float64)
PARAMS = dict(noise_params=[15.0, 1.0, 1], alpha=0.6, fim_thresh=0.36, interval=[75, 75])


class ReplayRng:
    def __init__(self, source):
        self.source, self.log = source, []

    def _take(self, kind, size):
        shape = tuple(np.atleast_1d(size))
        a = self.source.random(shape) if kind == "u" else self.source.standard_normal(shape)
        self.log.append((kind, a))
        return a

    def uniform(self, low=0.0, high=1.0, size=None):
        return low + (high - low) * self._take("u", size)

    def normal(self, loc, scale, size):
        return loc + scale * self._take("z", size)


def main():
    _install_placeholders()
    sys.path.insert(0, os.path.join(REF, "algos", "test_environment", "eval"))
    if not hasattr(np, "infty"):
        np.infty = np.inf
    import core                                                    # the reference's file, unmodified
    calls = []
    real_ssp = core.ssp

    def recording_ssp(W, M, u):
        idx = real_ssp(W, M, u)
        calls.append((W[:, 0].copy(), u.copy(), idx.copy()))
        return idx
    core.ssp = recording_ssp
    scale = np.diag(np.array([1e10, 1, 1]))
    out = {}
    cases = [(NP, thresh, near) for NP in (64, 100) for thresh in (1, 0.1) for near in (False, True)]
    tripped = short = blocked_seen = 0
    for c, (NP, thresh, near) in enumerate(cases):
        src = np.random.default_rng(1000 + c)
        source, inten, bkg = np.array([1200.0, 900.0]), 600.0, 20
        det = np.array([1100.0, 700.0]) if near else np.array([300.0, 2100.0])
        rng = ReplayRng(src)
        fic = core.FIC(nParticles=NP, bkg=bkg, rng=rng, thresh=thresh, L=1, scale=scale, **PARAMS)
        state = {"det": det, "blocked": ()}
        fic.FIM_step = lambda act: state["det"] + (0.0 if act in state["blocked"] else MOVES[act])
        rec = {k: [] for k in ("reading", "det", "cand", "latch_before", "latch_after", "prior_u", "normals", "resample_u", "xp_moved", "xp", "w",
                               "est", "neff", "ssp_w", "ssp_idx", "resampled", "J_renyi", "J_fish", "act", "score")}
        for t in range(STEPS):
            lam = inten * 1e4 / np.sum((state["det"] - source) ** 2) + bkg
            reading = float(src.poisson(lam))
            short += reading < 76
            state["blocked"] = {1: (0, 7), 3: (2, 3, 4)}.get(t, ())
            blocked_seen += len(state["blocked"])
            rng.log, n_calls = [], len(calls)
            meas = np.append(reading, state["det"])
            est = fic.bpf.track(meas).copy()
            draws = {k: [a for kind, a in rng.log if kind == k] for k in "uz"}
            if t == 0:
                prior_u = np.hstack((draws["u"][0][:, None], draws["u"][1]))
                res_u = draws["u"][2:]
                normals = np.zeros((NP, 3))
            else:
                prior_u, res_u, normals = np.zeros((NP, 3)), draws["u"], draws["z"][0]
            resampled = len(calls) > n_calls
            assert len(res_u) == int(resampled)
            xp, w = fic.bpf.xp_prev[:, t, :].copy(), fic.bpf.wp_prev[:, t, 0].copy()
            cand = np.array([fic.FIM_step(a) for a in range(8)])
            latch = int(fic.RDIV_FLAG)
            z = np.arange(np.clip(reading - PARAMS["interval"][0], 1, np.inf), reading + PARAMS["interval"][1], 1)
            Jr = np.array([fic.renyi_div(z, cand[a], fic.bpf.xp_prev[:, t, :], fic.bpf.wp_prev[:, t, :]) for a in range(8)])
            Jf = np.array([np.trace(fic.particle_FIM(cand[a], fic.bpf.xp_prev[:, t, :], fic.bpf.wp_prev[:, t, :], 3)) for a in range(8)])
            act, score = fic.optim_action(meas, est, step=t)
            tripped += latch == 1 and fic.RDIV_FLAG == 0
            for k, v in (("reading", reading), ("det", state["det"].copy()), ("cand", cand), ("latch_before", latch), ("latch_after", int(fic.RDIV_FLAG)),
                         ("prior_u", prior_u), ("normals", normals), ("resample_u", res_u[0] if resampled else np.zeros(NP - 1)),
                         ("xp", xp), ("w", w), ("est", est), ("neff", fic.bpf.nEff[t]), ("resampled", resampled),
                         ("ssp_w", calls[-1][0] if resampled else np.zeros(NP)), ("ssp_idx", calls[-1][2] if resampled else np.zeros(NP, dtype=np.int64)),
                         ("J_renyi", Jr), ("J_fish", Jf), ("act", int(act)), ("score", float(score))):
                rec[k].append(v)
            state["det"] = cand[int(act)].copy()
        for k, v in rec.items():
            if k != "xp_moved":
                out[f"c{c}_{k}"] = np.asarray(v)
        out[f"c{c}_meta"] = np.array([NP, thresh, bkg], dtype=np.float64)
    assert tripped > 0 and short > 0 and blocked_seen > 0, (tripped, short, blocked_seen)
    out["params"] = np.array([15.0, 1.0, 0.6, 0.36, 75, 75, 1e2, 1e3, 0.0, 25e2])      # sigma_xy, sigma_I, alpha, fim_thresh, interval, intensity, coord
    np.savez_compressed(os.path.join(OUT, "bpf_fic.npz"), **out)
    print("bpf_fic.npz:", len(cases), "cases,", tripped, "latch trips,", int(short), "readings below 76,", os.path.getsize(os.path.join(OUT, "bpf_fic.npz")), "bytes")


if __name__ == "__main__":
    main()
