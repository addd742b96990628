"""What the GPU tests of the particle filter and the RID-FIM controller share: a filter on a fresh env, and one track call / one
controller round compared pair by pair with the numpy restatement (tests/_bpf_ref.py), each from the state the kernel read."""
import numpy as np
import torch

import _bpf_ref as R

SEED = 77


def open_filter(N, A, obst, NP, **kw):
    from radiation_ppo_amd.bpf import BootstrapParticleFilter
    from radiation_ppo_amd.envs import RadSearchVec
    vec = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=SEED)
    vec.reset()
    return vec, BootstrapParticleFilter(vec, nParticles=NP, **kw)


def _params(bpf):
    p = bpf.params
    return dict(thresh=p.thresh, sigma_xy=p.sigma_xy, sigma_I=p.sigma_I, intensity=tuple(p.intensity), coord=tuple(p.coord), alpha=p.alpha,
                fim_thresh=p.fim_thresh, interval=tuple(p.interval))


def _snapshot(bpf):
    return {k: getattr(bpf, k).clone() for k in ("xp", "w", "logw", "estimate", "neff", "rdiv", "flags")}


def check_track(vec, bpf, obs, alive, first, call):
    """one track call -- call(obs, alive, first) is bpf.track or bpf.track_composed -- against the restatement, pair by pair"""
    from radiation_ppo_amd import _lib
    N, A, NP, P = bpf.N, bpf.A, bpf.NP, _params(bpf)
    before = _snapshot(bpf)
    u, z, ru = (t.cpu().numpy() for t in bpf.draws())
    call(obs, alive, first)
    torch.cuda.synchronize()
    after = _snapshot(bpf)
    b, a_ = ({k: v.cpu().numpy() for k, v in s.items()} for s in (before, after))
    det = np.stack([vec.state("x").t().cpu().numpy(), vec.state("y").t().cpu().numpy()], axis=-1).astype(np.float64)
    bkg, live, k = vec.state("bkg").cpu().numpy().reshape(-1), alive.cpu().numpy() != 0, obs[..., 0].double().cpu().numpy()
    worst = [0.0, 0.0, 0]      # weight error / SUM allowance: on pairs held to SUM alone, on pairs with a term under RULE; pairs held to SUM
    for n in range(N):
        for a in range(A):
            if not live[n]:
                for key in b:
                    assert b[key][n, a].tobytes() == a_[key][n, a].tobytes(), ("a finished lane was written", n, a, key)
                continue
            o = R.track(b["xp"][n, a].T, b["logw"][n, a], k[n, a], det[n, a], float(bkg[n]), first, P, u[n, a].T, z[n, a].T, ru[n, a])
            assert bool(a_["flags"][n, a] & _lib.RS_BPF_RESAMPLED) == o["resampled"] and not a_["flags"][n, a] & _lib.RS_BPF_ERR_SSP, (n, a)
            assert o["ok"]
            assert np.array_equal(a_["xp"][n, a].T.view(np.uint64), np.ascontiguousarray(o["xp"]).view(np.uint64)), ("particles", n, a)
            # weights: per particle, SUM alone unless the particle's (or, through the sum, another's) exponent falls under RULE
            tol, sum_only = R.weight_allowance(NP, o["M_last"] if o["resampled"] else o["M_first"], o["w"])
            dw = np.abs(a_["w"][n, a] - o["w"])
            assert (dw <= tol * o["w"] + 1e-300).all(), ("weights", n, a, sum_only, (dw / np.maximum(tol * o["w"], 1e-300)).max())
            ratio = float((dw / np.maximum(R.eps_sum(NP) * o["w"], 1e-300)).max())        # against SUM alone: asserted above where sum_only
            worst[0 if sum_only else 1] = max(worst[0 if sum_only else 1], ratio)
            worst[2] += int(sum_only)
            tol1, _ = R.weight_allowance(NP, o["M_first"], o["w_first"])
            q = np.sum(np.square(o["w_first"]))
            v = 1 / q
            rel_q = 2 * float(np.sum(np.square(o["w_first"]) * tol1)) / q + R.eps_sum(NP)
            slack = 1 if abs(v - (np.floor(v) + 0.5)) <= rel_q * v else 0
            assert abs(a_["neff"][n, a] - o["neff"]) <= slack, ("neff", n, a, a_["neff"][n, a], o["neff"])
            mag = ((o["w"] * (tol + R.eps_sum(NP)))[:, None] * np.abs(o["xp"])).sum(axis=0)
            assert (np.abs(a_["estimate"][n, a] - o["est"]) <= mag).all(), ("estimate", n, a)
            wk = a_["w"][n, a]
            assert np.array_equal(np.isneginf(a_["logw"][n, a]), wk == 0)
            with np.errstate(divide="ignore"):
                lg = np.log(wk)
            pos = wk > 0
            assert (np.abs(a_["logw"][n, a][pos] - lg[pos]) <= 8 * R.U * np.maximum(np.abs(lg[pos]), 1.0)).all()
            if first:
                assert a_["rdiv"][n, a] == 1
            else:
                assert a_["rdiv"][n, a] == b["rdiv"][n, a]
    return worst


def check_act(vec, bpf, obs, alive, call):
    """one controller round -- call(obs, alive, act8, J, J_fish) is bpf.act or bpf.act_composed -- against the restatement.  Returns
    (rows, rows excused as undecided in float64 -- the top-two gap inside twice the row's allowance --, the action rows, the worst
    errors against the summation bound).  The latch must follow the float64 rule on every row."""
    N, A, P = bpf.N, bpf.A, _params(bpf)
    cand = vec.peek(lam=False, meas=False)[0].cpu().numpy().astype(np.float64)
    xp, w, latch0 = bpf.xp.cpu().numpy(), bpf.w.cpu().numpy(), bpf.rdiv.cpu().numpy().copy()
    a8 = torch.full((N, A), -7, dtype=torch.int8, device="cuda")
    J = torch.full((N, A, 8), float("nan"), dtype=torch.float64, device="cuda")
    Jf = torch.full_like(J, float("nan"))
    call(obs, alive, a8, J, Jf)
    torch.cuda.synchronize()
    act, J, Jf, latch1 = a8.cpu().numpy(), J.cpu().numpy(), Jf.cpu().numpy(), bpf.rdiv.cpu().numpy()
    bkg, live, x0 = vec.state("bkg").cpu().numpy().reshape(-1), alive.cpu().numpy() != 0, obs[..., 0].double().cpu().numpy()
    rows = excused = 0
    worst = [0.0, 0.0, 0]          # J error / SUM allowance: on rows held to SUM alone, on rows with a term under RULE; rows held to SUM
    for n in range(N):
        for a in range(A):
            if not live[n]:
                assert act[n, a] == 8 and latch1[n, a] == latch0[n, a], (n, a)
                continue
            o = R.controller(xp[n, a].T, w[n, a], cand[n, a], x0[n, a], float(bkg[n]), int(latch0[n, a]), P)
            assert (np.abs(Jf[n, a] - o["J_fish"]) <= o["tolF"]).all(), ("J_fish", n, a, Jf[n, a] - o["J_fish"], o["tolF"])
            tol_sum = R.controller(xp[n, a].T, w[n, a], cand[n, a], x0[n, a], float(bkg[n]), int(latch0[n, a]), P, eval_term=False)["tolJ"]
            sum_only = bool((o["tolJ"] == tol_sum).all())          # no pmf of this row falls under RULE: the summation bound alone
            dJ = np.abs(J[n, a] - o["J"])
            assert (dJ <= o["tolJ"]).all(), ("J", n, a, x0[n, a], latch0[n, a], sum_only, dJ, o["tolJ"])
            ratio = float((dJ / np.maximum(tol_sum, 1e-300)).max())
            worst[0 if sum_only else 1] = max(worst[0 if sum_only else 1], ratio)
            worst[2] += int(sum_only)
            same = (cand[n, a][:, None, :] == cand[n, a][None, :, :]).all(axis=2)
            assert all(J[n, a, i].tobytes() == J[n, a, j].tobytes() for i in range(8) for j in range(8) if same[i, j]), ("bit-equal J", n, a)
            assert act[n, a] == int(np.argmax(J[n, a]))            # the kernel's own J: the first index of the maximum
            assert latch1[n, a] == o["latch"], ("latch", n, a, o["J"].max())      # transitions are exact
            rows += 1
            if act[n, a] != o["act"]:
                assert o["near"], ("action", n, a, act[n, a], o["act"], o["J"])
                excused += 1
    return rows, excused, act, worst
