"""rs_bpf_fim on the GPU against the numpy restatement of the reference's FIC.particle_FIM (tests/_bpf_a2c_ref.py), in its three forms
-- at the agent's position, at a given position, and the initial bound from the prior's particles -- and `fim_composed`, the same
matrix in float64 torch ops.  State and observation are test_ridfim_gpu's generator's on a real env.

Every entry of the matrix is held to the summation bound the project uses for J_fish, (NP + 16) * 2^-52 times the sum of the
magnitudes of the entry's terms (tests/_bpf_a2c_ref.py: tol), computed by the restatement; nothing is fitted.  `trace` is the sum of
the kernel's own diagonal within 2 ulp; rows of finished lanes keep a sentinel byte for byte; a particle exactly at the position
gives the restatement's nan pattern in both forms."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _bpf_a2c_ref as R2  # noqa: E402
from _bpf_drive import open_filter as _open  # noqa: E402
from test_ridfim_gpu import _craft  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(3, 1, 2, 0), (1, 1, 64, 0), (5, 1, 100, 3), (35, 2, 257, 0), (35, 2, 64, 3)]
SENTINEL = -1234.5


def _alive(N):
    return torch.from_numpy((np.arange(N) % 3 != 1).astype(np.uint8)).cuda()      # holes from N = 2 on


def _run(call, bpf, alive, pos, prior):
    F = torch.full((bpf.N, bpf.A, 3, 3), SENTINEL, dtype=torch.float64, device="cuda")
    tr = torch.full((bpf.N, bpf.A), SENTINEL, dtype=torch.float64, device="cuda")
    call(alive, pos=pos, prior=prior, F=F, trace=tr)
    torch.cuda.synchronize()
    return F.cpu().numpy(), tr.cpu().numpy()


def _check(vec, bpf, alive, pos, prior, call):
    """one launch against the restatement, pair by pair; returns the worst error as a share of the bound"""
    N, A, NP, P = bpf.N, bpf.A, bpf.NP, bpf.params
    F, tr = _run(call, bpf, alive, pos, prior)
    xp, w = bpf.xp.cpu().numpy(), bpf.w.cpu().numpy()
    u = bpf.draws()[0].cpu().numpy()
    det = np.stack([vec.state("x").t().cpu().numpy(), vec.state("y").t().cpu().numpy()], axis=-1).astype(np.float64)
    if pos is not None:
        det = pos.cpu().numpy()
    bkg, live = vec.state("bkg").cpu().numpy().reshape(-1), alive.cpu().numpy() != 0
    worst = 0.0
    for n in range(N):
        for a in range(A):
            if not live[n]:
                assert (F[n, a] == SENTINEL).all() and tr[n, a] == SENTINEL, ("a finished lane was written", n, a)
                continue
            if prior:
                want, mag = R2.fim_prior(R2.prior_particles(u[n, a].T, P.intensity, P.coord), det[n, a], float(bkg[n]), P.intensity, P.coord)
            else:
                want, mag = R2.fim(xp[n, a].T, w[n, a], det[n, a], float(bkg[n]))
            assert np.array_equal(np.isnan(F[n, a]), np.isnan(want)), (n, a, F[n, a], want)
            ok = np.isfinite(want)
            err, bound = np.abs(F[n, a] - want)[ok], R2.tol(NP, mag)[ok]
            assert (err <= bound).all(), (n, a, prior, err, bound)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if ok.any() else 0.0)
            own = (F[n, a, 0, 0] + F[n, a, 1, 1]) + F[n, a, 2, 2]
            if np.isfinite(own):
                assert abs(tr[n, a] - own) <= 2 * np.spacing(abs(own)), (n, a, tr[n, a], own)
            else:
                assert np.isnan(tr[n, a]) == np.isnan(own)
    return worst


@pytest.mark.parametrize("N,A,NP,obst", CASES)
def test_the_matrix_in_its_three_forms_and_composed(N, A, NP, obst):
    vec, bpf = _open(N, A, obst, NP)
    rng = np.random.default_rng(N * 1000 + NP)
    for t in range(2):
        vec.step(torch.from_numpy(rng.integers(0, 8, size=(N, A)).astype(np.int8)).cuda())
    _craft(vec, bpf, rng)
    alive = _alive(N)
    pos = torch.from_numpy(rng.uniform(0.0, 2700.0, (N, A, 2))).cuda()
    for name, call in (("fused", bpf.fim), ("composed", bpf.fim_composed)):
        worst = [_check(vec, bpf, alive, None, False, call), _check(vec, bpf, alive, pos, False, call), _check(vec, bpf, alive, None, True, call),
                 _check(vec, bpf, alive, pos, True, call)]
        print(f"N={N} A={A} NP={NP} obst={obst} {name}: worst error {max(worst[:2]):.3f} of the summation bound on the state's particles, "
              f"{max(worst[2:]):.3f} on the prior's")


def test_trace_is_j_fish_of_the_controller():
    """at a candidate position of the look-ahead the trace is the controller's J_fish: the same terms, summed entry by entry here"""
    N, A, NP = 6, 2, 100
    vec, bpf = _open(N, A, 0, NP)
    rng = np.random.default_rng(3)
    obs = _craft(vec, bpf, rng)
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    a8 = torch.zeros(N, A, dtype=torch.int8, device="cuda")
    Jf = torch.zeros(N, A, 8, dtype=torch.float64, device="cuda")
    bpf.act(obs, alive, a8, None, Jf)
    cand = vec.peek(lam=False, meas=False)[0].double()
    for mv in (0, 3):
        _, tr = _run(bpf.fim, bpf, alive, cand[:, :, mv].contiguous(), False)
        assert np.allclose(tr, Jf[:, :, mv].cpu().numpy(), rtol=(NP + 16) * 2.0 ** -52, atol=0.0)


def test_a_particle_exactly_at_the_position_is_numpy_s_nan_in_both_forms():
    N, A, NP = 2, 1, 64
    vec, bpf = _open(N, A, 0, NP)
    rng = np.random.default_rng(9)
    xp = np.empty((N, A, 3, NP))
    xp[:, :, 0], xp[:, :, 1:] = rng.uniform(100, 1000, (N, A, NP)), rng.uniform(0, 2500, (N, A, 2, NP))
    xp[0, 0, 1, 5], xp[0, 0, 2, 5] = float(vec.state("x")[0, 0]), float(vec.state("y")[0, 0])
    bpf.xp.copy_(torch.from_numpy(xp))
    bpf.w.fill_(1.0 / NP)
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    want, _ = R2.fim(xp[0, 0].T, np.full(NP, 1.0 / NP), xp[0, 0, 1:, 5], float(vec.state("bkg").view(-1)[0]))
    assert np.isnan(want).all()
    for call in (bpf.fim, bpf.fim_composed):
        _check(vec, bpf, alive, None, False, call)
        F, tr = _run(call, bpf, alive, None, False)
        assert np.isnan(F[0]).all() and np.isnan(tr[0]).all() and np.isfinite(F[1]).all() and np.isfinite(tr[1]).all()


def test_refusals_with_a_handle():
    from radiation_ppo_amd import _lib
    vec, bpf = _open(2, 1, 0, 16)
    other, _ = _open(3, 1, 0, 16)
    w, bad = 4096, _lib.RS_ERR_INVALID_ARG
    assert bpf.lib.rs_bpf_fim(vec._h, bpf._p, bpf._s, None, None, 0, w, None, None) == bad
    assert bpf.lib.rs_bpf_fim(vec._h, bpf._p, bpf._s, w, None, 0, None, None, None) == bad
    assert bpf.lib.rs_bpf_fim(other._h, bpf._p, bpf._s, w, None, 0, w, None, None) == bad          # num_pairs is not this handle's
