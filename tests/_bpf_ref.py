"""Plain numpy float64 restatement of the reference's bootstrap particle filter and RID-FIM controller
(algos/test_environment/eval/core.py: ParticleFilter :528-620, FIC :655-764, ssp :767-799) for ONE (env, agent) pair, taking every
draw as an array, and the error allowances the tests hold the kernels (and this file, against the reference's recorded values) to.
Particles are rows [NP, 3] = (intensity, x, y) as in the reference; the kernels keep them [3, NP].

The allowances, in units of u = 2^-53:
  SUM     a float64 sum of n terms taken in another order differs to first order by at most n * 2u relative to the sum of the
          magnitudes.  The figure for p_z and p_za -- sums of NP terms inside a sum over Z readings, the recurrence between two
          direct evaluations and the two logs -- is (NP + 3 Z) * 2^-52 relative; `eps_sum` returns it.
  EVAL    the reference evaluates pmf(z; lam) = exp(xlogy(z, lam) - gammaln(z + 1) - lam).  The three terms have magnitude M =
          z |log lam| + gammaln(z + 1) + lam (about 9e4 at a reading of 5000), their roundings and the last-bit differences between two
          math libraries' log and lgamma shift the exponent by up to EVAL_ULPS * u * M, and exp turns that into a RELATIVE error of the
          pmf.  This is the reference formula's own uncertainty -- no float64 evaluation of it, the reference's included, is defined
          more sharply -- and it is not part of SUM.  EVAL_ULPS = 6: product 1/2, log 1, lgamma 2, two subtractions 1/2 each, exp 1,
          rounded up.  Where two evaluations share one libm (this file against the reference's recording) it is not used.
  RULE    EVAL is applied term by term, and only to a term whose exponent is so large that the reference's own half-ulp rounding of
          it, u * M, already exceeds the SUM allowance of the sum the term enters: u * M > eps_sum (M > 2 NP for a weight, M >
          2 (NP + 3 Z) for a pmf; with 100 particles and 150 readings that is a reading above about 110).  Every other term, row and
          pair is held to SUM alone.  `eval_rel` is the rule."""
import numpy as np
from scipy.special import gammaln, xlogy

U = 2.0 ** -53
EVAL_ULPS = 6.0


def eps_sum(NP, Z=0):
    return (NP + 3 * Z) * 2.0 ** -52


def eval_rel(M, es):
    """RULE: the EVAL allowance of terms of exponent magnitude M entering a sum whose SUM allowance is es; 0 where u * M <= es"""
    M = np.where(np.isfinite(M), M, 0.0)
    return np.where(U * M > es, EVAL_ULPS * U * M, 0.0)


def rate(xp, det, bkg):
    """measModel (core.py:594-596)"""
    R = np.square(np.linalg.norm(xp[:, 1:] - det, axis=1))
    return np.round(xp[:, 0] * 1e4 / R) + bkg


def weigh(xp, logw, k, det, bkg):
    """poisson_ll and the reweighting (core.py:566-571): (logw, w, neff, M) -- M: the magnitude of each log-weight's terms (EVAL)"""
    lam = rate(xp, det, bkg)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = xlogy(k, lam), gammaln(k + 1)
        logw = logw + (t0 - t1 - lam)
        w = np.exp(logw - logw.max())
    w = w / w.sum()
    return logw, w, np.round(1 / np.sum(np.square(w))), np.abs(t0) + t1 + lam


def ssp(W, u):
    """ssp (core.py:767-799) on W [NP], statement for statement; returns (parent of every child, None if the counts do not add up --
    the reference raises ValueError there --, child counts)"""
    N = M = W.shape[0]
    MW = M * W
    nr_children = np.floor(MW).astype(np.int64)
    xi = MW - nr_children
    i, j = 0, 1
    for k in range(N - 1):
        delta_i = min(xi[j], 1. - xi[i])
        delta_j = min(xi[i], 1. - xi[j])
        sum_delta = delta_i + delta_j
        pj = delta_i / sum_delta if sum_delta > 0. else 0.
        if u[k] < pj:
            j, i = i, j
            delta_i = delta_j
        if xi[j] < 1. - xi[i]:
            xi[i] += delta_i
            j = k + 2
        else:
            xi[j] -= delta_i
            nr_children[i] += 1
            i = k + 2
    if np.sum(nr_children) == M - 1:
        last_ij = i if j == k + 2 else j
        if xi[last_ij] > 0.99:
            nr_children[last_ij] += 1
    if np.sum(nr_children) != M:
        return None, nr_children
    return np.arange(N).repeat(nr_children), nr_children


def track(xp, logw, k, det, bkg, first, P, prior_u=None, normals=None, resample_u=None):
    """ParticleFilter.track (core.py:554-591).  xp [NP, 3] and logw [NP] are the state before the call (ignored with first); P has
    thresh, sigma_xy, sigma_I, intensity, coord; prior_u / normals [NP, 3], resample_u [NP - 1].  Returns a dict: xp_moved (after
    prior or process model), xp, w, logw, est, neff, resampled, idx (None without a resampling or where ssp fails), ok, M_first /
    M_last (EVAL magnitudes of the first and the last weighing, the state's own |logw| included)."""
    NP = len(logw)
    if first:
        xp = np.empty((NP, 3))
        xp[:, 0] = P["intensity"][0] + (P["intensity"][1] - P["intensity"][0]) * prior_u[:, 0]
        xp[:, 1:] = P["coord"][0] + (P["coord"][1] - P["coord"][0]) * prior_u[:, 1:]
        logw = np.log(np.full(NP, 1 / NP))
    else:
        noise = np.array([P["sigma_I"], P["sigma_xy"], P["sigma_xy"]]) * normals
        xp = xp.copy()
        xp[:, 1:] = xp[:, 1:] + noise[:, 1:]
        xp[:, 0] = np.clip(xp[:, 0] + noise[:, 0], 0, np.inf)
    out = dict(xp_moved=xp.copy(), idx=None, ok=True)
    prev = np.where(np.isfinite(logw), np.abs(logw), 0.0)
    logw, w, neff, M = weigh(xp, logw, k, det, bkg)
    out["M_first"] = out["M_last"] = M + prev
    out["w_first"] = w
    out["resampled"] = bool(neff < P["thresh"] * NP)
    if out["resampled"]:
        idx, _ = ssp(w, resample_u)
        out["idx"], out["ok"] = idx, idx is not None
        if idx is not None:
            xp = xp[idx]
        logw, w, _, out["M_last"] = weigh(xp, np.zeros(NP), k, det, bkg)
    with np.errstate(divide="ignore"):
        out.update(xp=xp, w=w, est=np.sum(w[:, None] * xp, axis=0), logw=np.log(w), neff=neff)
    return out


def weight_allowance(NP, M, w):
    """relative allowance on every normalised weight w_p = e_p / S, per particle: SUM for the normalising sum, EVAL (under RULE) for
    the particle's own exponent, and for S the weighted mean of the particles' EVAL terms (dS / S = sum_q w_q d_q).  Returns
    (allowance [NP], True where no term of the pair needs EVAL: the pair is held to SUM alone)"""
    es = eps_sum(NP)
    d = eval_rel(M, es)
    return es + d + float(np.sum(w * d)), not d.any()


def fisher(xp, w, det, bkg):
    """np.trace(particle_FIM) with scale = diag(1e10, 1, 1) (core.py:686-694); returns (J_fish, sum of the terms' magnitudes)"""
    pred = xp.copy()
    pred[:, 0] = pred[:, 0] * 1e4
    denom = np.sum(np.square(det - pred[:, 1:]), axis=1)
    grad_xy = (2 * (det - pred[:, 1:])) * (pred[:, 0] / np.square(denom))[:, None]
    grad = np.hstack(((1 / denom)[:, None], grad_xy))
    J = np.einsum('ij,ikl->ijk', grad, grad[:, :, None]) * (1 / (pred[:, 0] / denom + bkg))[:, None, None]
    Js = (J @ np.diag([1e10, 1.0, 1.0])) * w[:, None, None]
    return float(np.trace(Js.sum(axis=0))), float(np.abs(np.trace(Js, axis1=1, axis2=2)).sum())


def window(x0, interval):
    return np.arange(np.clip(x0 - interval[0], 1, np.inf), x0 + interval[1], 1)


def renyi(xp, w, det, bkg, z, alpha, eval_term=True):
    """renyi_div (core.py:696-701) with the rule that a z whose p_z is 0 contributes 0.  Returns (J, allowance on J): SUM (and, with
    eval_term, EVAL under RULE, weighted by each particle's share of p_z and p_za) on p_z and p_za, propagated to first order through
    J = c sum_z p_z (log p_za - alpha log p_z): |dJ| <= |c| sum_z p_z (e_z |log p_za - alpha log p_z| + e_za + alpha e_z)."""
    if len(z) == 0:
        return (1 / (alpha - 1)) * 0.0, 0.0
    lam = rate(xp, det, bkg)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t0, t1 = xlogy(z[None, :], lam), gammaln(z + 1)[None, :]
        l_hood = np.exp(t0 - t1 - lam)
        M = np.abs(t0) + t1 + lam
        p_z = (w[:, None] * l_hood).sum(axis=0)
        p_za = (w[:, None] * l_hood ** alpha).sum(axis=0)
        on = p_z > 0
        B = np.where(on, np.log(p_za) - alpha * np.log(p_z), 0.0)
        es = eps_sum(len(w), len(z))
        d = np.where(l_hood > 0, eval_rel(M, es), 0.0) if eval_term else np.zeros_like(M)          # RULE, term by term
        m_z = np.where(on, (w[:, None] * l_hood * d).sum(axis=0) / np.where(on, p_z, 1.0), 0.0)
        m_za = np.where(on, (w[:, None] * l_hood ** alpha * d).sum(axis=0) / np.where(on, p_za, 1.0), 0.0)
    e_z, e_za = es + m_z, es + alpha * m_za
    c = 1 / (alpha - 1)
    J = c * np.where(on, p_z * B, 0.0).sum()
    return float(J), float(abs(c) * (p_z * (e_z * np.abs(B) + e_za + alpha * e_z)).sum())


def controller(xp, w, cand, x0, bkg, latch, P, eval_term=True):
    """FIC.optim_action with L = 1 (core.py:703-764) on the eight candidate positions cand [8, 2].  Returns a dict: J, J_fish [8], their
    allowances tolJ, tolF [8], act (first index of the maximum), latch (after), near (the top-two gap of J is inside twice the
    allowance: the argmax is not decided in float64)."""
    z = window(x0, P["interval"])
    J, Jf, tJ, tF = np.zeros(8), np.zeros(8), np.zeros(8), np.zeros(8)
    for a in range(8):
        Jf[a], mag = fisher(xp, w, cand[a], bkg)
        tF[a] = (len(w) + 16) * 2.0 ** -52 * mag
        if latch:
            J[a], tJ[a] = renyi(xp, w, cand[a], bkg, z, P["alpha"], eval_term)
        else:
            J[a], tJ[a] = Jf[a], tF[a]
    act = int(J.argmax())
    order = np.sort(J)[::-1]
    distinct = order[order < order[0]]
    near = bool(distinct.size and order[0] - distinct[0] <= 2 * tJ.max())
    new_latch = 0 if (latch == 1 and J.max() > P["fim_thresh"]) else latch
    return dict(J=J, J_fish=Jf, tolJ=tJ, tolF=tF, act=act, latch=new_latch, near=near)
