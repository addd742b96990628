"""The bootstrap particle filter and the RID-FIM controller of the reference's evaluation ('rid-fim' in
algos/test_environment/eval/test_policy.py:184-231, 573-574; ParticleFilter, FIC and ssp in eval/core.py:528-620, 655-764, 767-799)
for every (env, agent) pair of a RadSearchVec at once: one filter over (intensity, x, y) per pair, nothing shared between agents.

`BootstrapParticleFilter` owns the state tensors (float64) and runs the HIP kernels of csrc/rs_bpf.hip -- `track` (rs_bpf_track),
`act` (rs_ridfim_eval_step) and `fim` (rs_bpf_fim: the particles' 3 x 3 Fisher information matrix, which 'bpf-a2c' scores its moves by
and the Fisher analysis records).  `track_composed`, `act_composed` and `fim_composed` are the same rounds composed from rs_bpf_draws,
rs_peek and float64 torch ops on the same state: the A/B form of the evaluation runners, not a fallback -- without the library nothing
here runs.  `pcrb` is the posterior Cramer-Rao bound's recursion on the recorded matrices (test_policy.py:368-371, 435), on the host."""
import ctypes as C
from types import SimpleNamespace

import torch

from . import _lib


class BootstrapParticleFilter:
    """One bootstrap particle filter per (env, agent) pair of `vec`, with the RID-FIM controller's latch.

    Defaults are the reference's for 'rid-fim' (test_policy.py:573-574 through FIC.__init__, core.py:656-668): nParticles 6000,
    noise_params [15, 1, 1] -- proSigma = [noise_params[1], noise_params[0], noise_params[0]] (core.py:540), so 15 cm on x and y and 1
    on the intensity --, thresh 1 (a resampling at every step), intensity [1e2, 1e3] in the filter's units (x 1e4 in the measurement
    model), coord [0, 25e2], alpha 0.6, fim_thresh 0.36, interval [75, 75].
    The env's area is 2700 cm wide, so the reference's prior box [0, 2500]^2 does not cover its last 200 cm: a source there starts
    outside every particle.  The default is kept; `coord` is a parameter.

    State (float64 unless noted): xp [N, A, 3, NP], w and logw [N, A, NP], estimate [N, A, 3] (xpHatMean), neff [N, A],
    rdiv [N, A] uint8 (RDIV_FLAG: 1 = Renyi divergence, 0 = Fisher information), flags [N, A] int32 (RS_BPF_RESAMPLED,
    RS_BPF_ERR_SSP)."""

    def __init__(self, vec, nParticles: int = 6000, noise_params=(15.0, 1.0, 1.0), thresh: float = 1.0, intensity=(1e2, 1e3),
                 coord=(0.0, 25e2), alpha: float = 0.6, fim_thresh: float = 0.36, interval=(75, 75)):
        NP = int(nParticles)
        if NP < 2:
            raise ValueError("nParticles must be at least 2")
        if alpha == 1 or min(interval) < 0 or sum(interval) > _lib.RS_BPF_MAX_WINDOW:
            raise ValueError(f"alpha must not be 1 and interval must be non-negative with a sum of at most {_lib.RS_BPF_MAX_WINDOW}")
        self.vec, self.lib, self.NP = vec, vec.lib, NP
        N, A, dev = vec.num_envs, vec.number_agents, vec.device
        self.N, self.A = N, A
        self.params = SimpleNamespace(num_particles=NP, sigma_xy=float(noise_params[0]), sigma_I=float(noise_params[1]), thresh=float(thresh),
                                      intensity=(float(intensity[0]), float(intensity[1])), coord=(float(coord[0]), float(coord[1])),
                                      alpha=float(alpha), fim_thresh=float(fim_thresh), interval=(int(interval[0]), int(interval[1])))
        self._p = self._s = None
        self.configure()
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            self.xp = torch.zeros(N, A, 3, NP, **f64)
            self.w = torch.zeros(N, A, NP, **f64)
            self.logw = torch.zeros(N, A, NP, **f64)
            self.estimate = torch.zeros(N, A, 3, **f64)
            self.neff = torch.zeros(N, A, **f64)
            self.rdiv = torch.ones(N, A, dtype=torch.uint8, device=dev)
            self.flags = torch.zeros(N, A, dtype=torch.int32, device=dev)
            nbytes = self.lib.rs_bpf_scratch_bytes(N * A, NP)
            self.scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        p = lambda t: t.data_ptr()
        self._s = C.c_void_p()
        _lib.check(self.lib.rs_bpf_state_create(N * A, p(self.xp), p(self.w), p(self.logw), p(self.estimate), p(self.neff), p(self.rdiv),
                                                p(self.flags), p(self.scratch), self.scratch.numel() * 8, C.byref(self._s)), "rs_bpf_state_create")

    def configure(self, **changes):
        """(re)build the library's parameter object from `params`, after setting the fields given (thresh=..., alpha=..., ...)"""
        for k, v in changes.items():
            if not hasattr(self.params, k) or k == "num_particles":
                raise ValueError(f"no such filter parameter to change: {k}")
            setattr(self.params, k, v)
        P, new = self.params, C.c_void_p()
        _lib.check(self.lib.rs_bpf_params_create(P.num_particles, P.sigma_xy, P.sigma_I, P.thresh, (C.c_double * 2)(*P.intensity),
                                                 (C.c_double * 2)(*P.coord), P.alpha, P.fim_thresh, (C.c_int32 * 2)(*P.interval),
                                                 C.byref(new)), "rs_bpf_params_create")
        if self._p:
            self.lib.rs_bpf_params_destroy(self._p)
        self._p = new

    def __del__(self):
        if getattr(self, "_p", None):
            self.lib.rs_bpf_params_destroy(self._p)
        if getattr(self, "_s", None):
            self.lib.rs_bpf_state_destroy(self._s)
        self._p = self._s = None

    @staticmethod
    def bytes_per_pair(nParticles: int) -> int:
        """device memory of one pair's state and scratch (8 particle-sized float64 rows and the child counts)"""
        return int(nParticles) * (8 * 8 + 4) + 64

    # ---- the HIP rounds
    def track(self, obs: torch.Tensor, alive: torch.Tensor, first: bool) -> torch.Tensor:
        """ParticleFilter.track on the reading obs[n, a, 0] at the agent's position, for the lanes with alive[n] != 0 (uint8 [N]);
        first: draw the prior and set the latch instead of the process model.  Returns `estimate`."""
        _lib.check(self.lib.rs_bpf_track(self.vec._h, self._p, self._s, obs.data_ptr(), alive.data_ptr(), 1 if first else 0,
                                         self.vec._stream()), "rs_bpf_track")
        return self.estimate

    def act(self, obs: torch.Tensor, alive: torch.Tensor, act8: torch.Tensor, J: torch.Tensor = None, J_fish: torch.Tensor = None) -> torch.Tensor:
        """FIC.optim_action (L = 1): rs_step's action rows into act8 [N, A] int8 (8 on finished lanes); J, J_fish [N, A, 8] float64."""
        _lib.check(self.lib.rs_ridfim_eval_step(self.vec._h, self._p, self._s, obs.data_ptr(), alive.data_ptr(), act8.data_ptr(),
                                                None if J is None else J.data_ptr(), None if J_fish is None else J_fish.data_ptr(),
                                                self.vec._stream()), "rs_ridfim_eval_step")
        return act8

    def fim(self, alive: torch.Tensor, pos: torch.Tensor = None, prior: bool = False, F: torch.Tensor = None,
            trace: torch.Tensor = None) -> torch.Tensor:
        """FIC.particle_FIM (core.py:686-694; rs_bpf_fim): the particles' Fisher information matrix F [N, A, 3, 3] float64 at pos
        [N, A, 2] float64 (None: every agent's present position), F[i][j] = sum_p w_p g_i g_j s c_j with the column scale
        c = (1e10, 1, 1).  prior: the initial bound (test_policy.py:127-135) -- the prior's particles, regenerated from the draws
        `track(first=True)` consumes at the env's present step, weights 1 / NP, c = (1e10 / (I_hi - I_lo), 1 / (c_hi - c_lo),
        1 / (c_hi - c_lo)).  trace [N, A], where given, receives the diagonal's sum.  Rows of finished lanes (alive[n] == 0) are not
        written; without an F a zeroed one is made.
        One difference from the reference, on purpose: its `FIM` and 'rid-fim' `init_est` branches index a 2-vector detector position
        with [1:], which broadcasts y over both axes (test_policy.py:121, 197, 206); here the position is the detector's (x, y), as
        the `act` branches and 'bpf-a2c''s `init_est` have it."""
        if F is None:
            F = torch.zeros(self.N, self.A, 3, 3, dtype=torch.float64, device=self.vec.device)
        _lib.check(self.lib.rs_bpf_fim(self.vec._h, self._p, self._s, alive.data_ptr(), None if pos is None else pos.data_ptr(),
                                       1 if prior else 0, F.data_ptr(), None if trace is None else trace.data_ptr(), self.vec._stream()),
                   "rs_bpf_fim")
        return F

    def draws(self):
        """(prior_u [N, A, 3, NP], normals [N, A, 3, NP], resample_u [N, A, NP - 1]): what `track` would consume at the env's step"""
        f64 = dict(dtype=torch.float64, device=self.vec.device)
        u, z, r = (torch.empty(self.N, self.A, 3, self.NP, **f64), torch.empty(self.N, self.A, 3, self.NP, **f64),
                   torch.empty(self.N, self.A, self.NP - 1, **f64))
        _lib.check(self.lib.rs_bpf_draws(self.vec._h, self.NP, u.data_ptr(), z.data_ptr(), r.data_ptr(), self.vec._stream()), "rs_bpf_draws")
        return u, z, r

    # ---- the same rounds composed from the draws, rs_peek and float64 torch ops
    def _det_bkg(self):
        det = torch.stack([self.vec.state("x").t(), self.vec.state("y").t()], dim=-1).double()       # [N, A, 2]
        return det, self.vec.state("bkg").double().view(self.N, 1).expand(self.N, self.A)

    @staticmethod
    def _rate(xp, det, bkg):
        """measModel (core.py:594-596): xp [..., 3, NP], det [..., 2], bkg [...]"""
        ex, ey = xp[..., 1, :] - det[..., 0:1], xp[..., 2, :] - det[..., 1:2]
        nr = torch.sqrt(ex * ex + ey * ey)
        return torch.round(xp[..., 0, :] * 1e4 / (nr * nr)) + bkg.unsqueeze(-1)

    def _weigh(self, xp, logw, k, det, bkg):
        lam = self._rate(xp, det, bkg)
        kk = k.unsqueeze(-1)
        logw = logw + (torch.xlogy(kk, lam) - torch.lgamma(kk + 1) - lam)
        w = torch.exp(logw - logw.max(dim=-1, keepdim=True).values)
        w = w / w.sum(dim=-1, keepdim=True)
        return logw, w, torch.round(1 / (w * w).sum(dim=-1))

    @staticmethod
    def _ssp(W, u):
        """ssp (core.py:767-799) row by row of W [B, NP] with u [B, NP - 1]: (parent index of every child [B, NP], rows whose counts add up)"""
        B, NP = W.shape
        MW = NP * W
        fl = torch.floor(MW)
        pad = lambda t: torch.cat([t, torch.zeros(B, 1, dtype=t.dtype, device=t.device)], dim=1)      # index NP enters at the last step
        xi, cnt = pad(MW - fl), pad(fl.long())
        ar = torch.arange(B, device=W.device)
        i, j = torch.zeros(B, dtype=torch.long, device=W.device), torch.ones(B, dtype=torch.long, device=W.device)
        for k in range(NP - 1):
            xii, xij = xi[ar, i], xi[ar, j]
            di, dj = torch.minimum(xij, 1.0 - xii), torch.minimum(xii, 1.0 - xij)
            sd = di + dj
            pj = torch.where(sd > 0, di / sd, torch.zeros_like(sd))
            sw = u[:, k] < pj
            i, j, di = torch.where(sw, j, i), torch.where(sw, i, j), torch.where(sw, dj, di)
            xii, xij = xi[ar, i], xi[ar, j]
            inc = xij < 1.0 - xii
            xi[ar, i] = torch.where(inc, xii + di, xii)
            xi[ar, j] = torch.where(inc, xij, xij - di)
            cnt[ar, i] += (~inc).long()
            nxt = torch.full_like(i, k + 2)
            i, j = torch.where(inc, i, nxt), torch.where(inc, nxt, j)
        tot = cnt[:, :NP].sum(dim=1)
        last = torch.where(j == NP, i, j)
        add = (tot == NP - 1) & (xi[ar, last] > 0.99)
        cnt[ar, last] += add.long()
        ok = tot + add.long() == NP
        cum = torch.cumsum(cnt[:, :NP], dim=1)
        idx = torch.searchsorted(cum, torch.arange(NP, device=W.device).expand(B, NP).contiguous(), right=True)
        return idx.clamp_(max=NP - 1), ok

    def track_composed(self, obs, alive, first):
        N, A, NP, P = self.N, self.A, self.NP, self.params
        u, z, ru = self.draws()
        det, bkg = self._det_bkg()
        k = obs[..., 0].double()
        live = (alive != 0).view(N, 1).expand(N, A)
        if first:
            lo = torch.tensor([P.intensity[0], P.coord[0], P.coord[0]], dtype=torch.float64, device=u.device).view(1, 1, 3, 1)
            hi = torch.tensor([P.intensity[1], P.coord[1], P.coord[1]], dtype=torch.float64, device=u.device).view(1, 1, 3, 1)
            xp = lo + (hi - lo) * u
            logw = torch.full((N, A, NP), 1.0 / NP, dtype=torch.float64, device=u.device).log()
        else:
            sig = torch.tensor([P.sigma_I, P.sigma_xy, P.sigma_xy], dtype=torch.float64, device=u.device).view(1, 1, 3, 1)
            xp = self.xp + sig * z
            xp[:, :, 0] = xp[:, :, 0].clamp(min=0.0)
            logw = self.logw
        logw, w, neff = self._weigh(xp, logw, k, det, bkg)
        res = live & (neff < P.thresh * NP)
        flags = self.flags & _lib.RS_BPF_ERR_SSP
        if bool(res.any()):
            rows = res.view(-1).nonzero().view(-1)
            idx, ok = self._ssp(w.view(N * A, NP)[rows], ru.view(N * A, NP - 1)[rows])
            xr = xp.view(N * A, 3, NP)[rows]
            gathered = torch.gather(xr, 2, idx.unsqueeze(1).expand(-1, 3, -1))
            xr = torch.where(ok.view(-1, 1, 1), gathered, xr)
            xp.view(N * A, 3, NP)[rows] = xr
            lw2, w2, _ = self._weigh(xr, torch.zeros_like(xr[:, 0]), k.reshape(-1)[rows], det.view(N * A, 2)[rows], bkg.reshape(-1)[rows])
            w.view(N * A, NP)[rows] = w2
            f = flags.view(-1)
            f[rows] |= torch.where(ok, _lib.RS_BPF_RESAMPLED, _lib.RS_BPF_RESAMPLED | _lib.RS_BPF_ERR_SSP).to(f.dtype)
        est = (w.unsqueeze(2) * xp).sum(dim=-1)
        lv3, lv4 = live.unsqueeze(-1), live.view(N, A, 1, 1)
        self.xp.copy_(torch.where(lv4, xp, self.xp))
        self.w.copy_(torch.where(lv3, w, self.w))
        self.logw.copy_(torch.where(lv3, w.log(), self.logw))
        self.estimate.copy_(torch.where(lv3, est, self.estimate))
        self.neff.copy_(torch.where(live, neff, self.neff))
        self.flags.copy_(torch.where(live, flags, self.flags))
        if first:
            self.rdiv.copy_(torch.where(live, torch.ones_like(self.rdiv), self.rdiv))
        return self.estimate

    def act_composed(self, obs, alive, act8, J=None, J_fish=None):
        N, A, NP, P = self.N, self.A, self.NP, self.params
        cand = self.vec.peek(lam=False, meas=False)[0].double().view(N * A, 8, 2)
        _, bkg = self._det_bkg()
        bkg = bkg.reshape(-1)
        xp, w = self.xp.view(N * A, 3, NP), self.w.view(N * A, NP)
        x0 = obs[..., 0].double().reshape(-1)
        zlo = (x0 - P.interval[0]).clamp(min=1.0)
        Z = int(P.interval[0] + P.interval[1])
        t = torch.arange(Z, dtype=torch.float64, device=xp.device)
        Jr = torch.zeros(N * A, 8, dtype=torch.float64, device=xp.device)
        Jf = torch.zeros_like(Jr)
        rows_per = max(1, int(2e7 // (NP * max(Z, 1))))
        coef = 1.0 / (P.alpha - 1.0)
        for b0 in range(0, N * A, rows_per):
            sl = slice(b0, b0 + rows_per)
            I4 = xp[sl, 0] * 1e4
            z = zlo[sl, None] + t                                                     # [b, Z]
            valid = z < (x0[sl, None] + P.interval[1])
            lgz = torch.lgamma(z + 1)
            for mv in range(8):
                c = cand[sl, mv]
                ex, ey = c[:, 0:1] - xp[sl, 1], c[:, 1:2] - xp[sl, 2]
                den = ex * ex + ey * ey
                f = I4 / (den * den)
                g0, g1, g2 = 1.0 / den, (2.0 * ex) * f, (2.0 * ey) * f
                s = 1.0 / (I4 / den + bkg[sl, None])
                Jf[sl, mv] = ((((g0 * g0 * s) * 1e10 + g1 * g1 * s) + g2 * g2 * s) * w[sl]).sum(dim=1)
                lam = self._rate(xp[sl], c, bkg[sl]).unsqueeze(-1)                    # [b, NP, 1]
                pmf = torch.exp(torch.xlogy(z.unsqueeze(1), lam) - lgz.unsqueeze(1) - lam)
                pz = (w[sl].unsqueeze(-1) * pmf).sum(dim=1)
                pza = (w[sl].unsqueeze(-1) * pmf ** P.alpha).sum(dim=1)
                term = torch.where(valid & (pz > 0), pz * (torch.log(pza) - P.alpha * torch.log(pz)), torch.zeros_like(pz))
                Jr[sl, mv] = coef * term.sum(dim=1)
        latch = self.rdiv.view(-1) == 1
        Jk = torch.where(latch.view(-1, 1), Jr, Jf)
        top = Jk.max(dim=1).values
        # np.argmax: the first nan if there is one (top is nan then), else the first index of the maximum
        act = torch.where(top.isnan().view(-1, 1), Jk.isnan(), Jk == top.view(-1, 1)).int().argmax(dim=1)
        live = (alive != 0).view(N, 1).expand(N, A).reshape(-1)
        clear = live & latch & (top > P.fim_thresh)
        self.rdiv.view(-1)[clear] = 0
        act8.copy_(torch.where(live, act, torch.full_like(act, 8)).to(torch.int8).view(N, A))
        if J is not None:
            J.copy_(Jk.view(N, A, 8))
        if J_fish is not None:
            J_fish.copy_(Jf.view(N, A, 8))
        return act8

    def fim_composed(self, alive, pos=None, prior=False, F=None, trace=None):
        """`fim` in float64 torch ops; the prior's particles come from `draws()`"""
        N, A, NP, P = self.N, self.A, self.NP, self.params
        dev = self.vec.device
        det, bkg = self._det_bkg()
        if pos is not None:
            det = pos
        if prior:
            u = self.draws()[0]
            lo = torch.tensor([P.intensity[0], P.coord[0], P.coord[0]], dtype=torch.float64, device=dev).view(1, 1, 3, 1)
            hi = torch.tensor([P.intensity[1], P.coord[1], P.coord[1]], dtype=torch.float64, device=dev).view(1, 1, 3, 1)
            xp, w = lo + (hi - lo) * u, torch.full((N, A, NP), 1.0 / NP, dtype=torch.float64, device=dev)
            c = [1e10 / (P.intensity[1] - P.intensity[0]), 1.0 / (P.coord[1] - P.coord[0]), 1.0 / (P.coord[1] - P.coord[0])]
        else:
            xp, w, c = self.xp, self.w, [1e10, 1.0, 1.0]
        c = torch.tensor(c, dtype=torch.float64, device=dev).view(1, 1, 3, 1)
        xp, w, det, bkg = xp.view(N * A, 3, NP), w.view(N * A, NP), det.reshape(N * A, 2), bkg.reshape(-1)
        Fm = torch.empty(N * A, 3, 3, dtype=torch.float64, device=dev)
        rows_per = max(1, int(2e7 // (9 * NP)))
        for b0 in range(0, N * A, rows_per):
            sl = slice(b0, b0 + rows_per)
            I4 = xp[sl, 0] * 1e4
            ex, ey = det[sl, 0:1] - xp[sl, 1], det[sl, 1:2] - xp[sl, 2]
            den = ex * ex + ey * ey
            f = I4 / (den * den)
            g = torch.stack([1.0 / den, (2.0 * ex) * f, (2.0 * ey) * f], dim=1)         # [b, 3, NP]
            s = 1.0 / (I4 / den + bkg[sl, None])
            Fm[sl] = ((((g.unsqueeze(2) * g.unsqueeze(1)) * s[:, None, None]) * c) * w[sl, None, None]).sum(dim=-1)
        Fm = Fm.view(N, A, 3, 3)
        live = (alive != 0).view(N, 1)
        if F is None:
            F = torch.zeros_like(Fm)
        F.copy_(torch.where(live.view(N, 1, 1, 1), Fm, F))
        if trace is not None:
            trace.copy_(torch.where(live, (Fm[..., 0, 0] + Fm[..., 1, 1]) + Fm[..., 2, 2], trace))
        return F


def pcrb(F0, R, noise_params=(15.0, 1.0, 1.0)):
    """The posterior Cramer-Rao bound's recursion as the reference writes it (test_policy.py:368-371, 435), on the host in numpy, batched
    over the leading axes:  D = inv(diag(sigma^2)) with sigma = (noise_params[1], noise_params[0], noise_params[0]),  B_0 = F0,
    B_t = D + R_t - np.square(D) @ inv(B_{t-1} + D)  -- np.square is elementwise, as in the reference.
    F0 [..., 3, 3]: the initial bound (`fim(prior=True)`); R [T, ..., 3, 3]: the matrix at the detector after steps 1..T (`fim`).
    Returns B [T + 1, ..., 3, 3]; from the first step at which a lane's R_t or B_{t-1} is not finite (a finished lane's rows are nan) its
    B_t is nan."""
    import numpy as np
    F0, R = np.asarray(F0, dtype=np.float64), np.asarray(R, dtype=np.float64)
    sigma = np.array([noise_params[1], noise_params[0], noise_params[0]], dtype=np.float64)
    D = np.linalg.inv(np.diag(np.square(sigma)))
    B = np.full((R.shape[0] + 1,) + F0.shape, np.nan)
    B[0] = F0
    for t in range(1, B.shape[0]):
        M = B[t - 1] + D
        ok = np.isfinite(M).all(axis=(-2, -1)) & np.isfinite(R[t - 1]).all(axis=(-2, -1))
        if ok.any():
            B[t][ok] = D + R[t - 1][ok] - np.square(D) @ np.linalg.inv(M[ok])
    return B
