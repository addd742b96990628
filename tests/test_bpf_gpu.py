"""rs_bpf_track on the GPU against the numpy restatement of the reference's ParticleFilter.track and ssp (tests/_bpf_ref.py, itself held
to the reference's recorded values by tests/test_bpf_cpu.py).  Every track call is compared on its own: the restatement starts from
the state the kernel read and consumes the draws rs_bpf_draws wrote for that step, so nothing drifts.

Bit for bit: the particles after the prior, the process model and the gather (hence the resampler's indices), the resampling
decision, finished lanes.  Under a bound: weights, nEff, the estimate.  The bound on a weight is the summation bound NP * 2^-52
(relative) and nothing else, except for particles whose log-likelihood xlogy(k, lam) - gammaln(k + 1) - lam (plus the carried |logw|)
has terms of a magnitude M so large that the reference's own half-ulp rounding of it exceeds that bound (u M > NP 2^-52, RULE in
tests/_bpf_ref.py): those get 6 u M on top, the uncertainty of the formula under two math libraries, and through the normalising sum
every weight of the pair gets the weighted mean of these terms.  A pair with no such particle (k = 0 and small readings) is held to
the summation bound alone; the test prints how the kernel stands against that bound on both kinds of pair.  Nothing in the allowance is
fitted to the kernel's output.  nEff = rint(1 / sum w^2) may differ by one only where 1 / sum w^2 lies within its allowance of a
half-integer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _bpf_ref as R  # noqa: E402,F401
from _bpf_drive import SEED, check_track, open_filter as _open  # noqa: E402,F401

pytestmark = pytest.mark.gpu

# (envs, agents, particles, obstructions): 1, 5 and 70 pairs; NP below, above and far from a multiple of 64, above the workgroup's 256
# lanes (257), the smallest (2) and one past the resampler's 512-step staging chunk (600)
CASES = [(1, 1, 64, 0), (5, 1, 100, 3), (35, 2, 257, 0), (70, 1, 100, 3), (3, 2, 2, 0), (2, 1, 600, 3)]


def _alive(N):
    return torch.from_numpy((np.arange(N) % 4 != 2).astype(np.uint8)).cuda()


@pytest.mark.parametrize("thresh", [1.0, 0.1])
@pytest.mark.parametrize("N,A,NP,obst", CASES)
def test_track_step_by_step(N, A, NP, obst, thresh):
    vec, bpf = _open(N, A, obst, NP, thresh=thresh)
    rng = np.random.default_rng(NP + A)
    alive = _alive(N)
    resampled = 0
    worst = check_track(vec, bpf, vec.obs, alive, True, bpf.track)
    merge = lambda x, y: [max(x[0], y[0]), max(x[1], y[1]), x[2] + y[2]]
    resampled += int((bpf.flags & 1).sum())
    for t in range(3):
        vec.step(torch.from_numpy(rng.integers(0, 8, size=(N, A)).astype(np.int8)).cuda())
        worst = merge(worst, check_track(vec, bpf, vec.obs, alive, False, bpf.track))
        resampled += int((bpf.flags & 1).sum())
    print(f"N={N} A={A} NP={NP} obst={obst} thresh={thresh}: worst weight error {worst[0]:.3f} of the summation bound on the {worst[2]} "
          f"pair-steps held to it alone, {worst[1]:.3f} of it on the others; {resampled} resamplings")
    if thresh == 1.0 and NP > 2:
        assert resampled > 0


def test_infinite_log_weights_first_again_and_readings():
    """a crafted state whose logw holds -inf entries (weights of 0: no children, -inf again afterwards); readings of 0, 40 and 5000;
    `first` on a used state: the prior is drawn again, the latch goes back up"""
    N, A, NP = 6, 1, 100
    vec, bpf = _open(N, A, 0, NP, thresh=1.0)
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    check_track(vec, bpf, vec.obs, alive, True, bpf.track)
    vec.step(torch.full((N, A), 2, dtype=torch.int8, device="cuda"))
    bpf.logw[:, :, ::3] = float("-inf")
    obs = vec.obs.clone()
    obs[0, 0, 0], obs[1, 0, 0], obs[2, 0, 0] = 0.0, 40.0, 5000.0
    check_track(vec, bpf, obs, alive, False, bpf.track)
    bpf.configure(thresh=0.0)                                      # no resampling: the zero weights stay and their logw is -inf
    bpf.logw[:, :, ::3] = float("-inf")
    check_track(vec, bpf, obs, alive, False, bpf.track)
    assert torch.isneginf(bpf.logw[:, :, ::3]).all() and (bpf.w[:, :, ::3] == 0).all()
    bpf.configure(thresh=1.0)
    bpf.rdiv.zero_()
    used = bpf.xp.clone()
    check_track(vec, bpf, vec.obs, _alive(N), True, bpf.track)
    assert (bpf.rdiv.cpu().numpy()[:, 0] == (np.arange(N) % 4 != 2)).all() and not torch.equal(used, bpf.xp)


def test_draws_are_uniform_and_normal():
    vec, bpf = _open(4, 2, 0, 1000)
    u, z, ru = (t.cpu().numpy() for t in bpf.draws())
    assert u.min() >= 0 and u.max() < 1 and ru.min() >= 0 and ru.max() < 1 and abs(u.mean() - 0.5) < 0.01 and abs(ru.mean() - 0.5) < 0.02
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1) < 0.03 and abs((z ** 4).mean() - 3) < 0.3
    assert abs(np.corrcoef(z[:, :, 0].ravel(), z[:, :, 1].ravel())[0, 1]) < 0.03
    assert len(np.unique(u)) == u.size                             # no two pairs, particles or components share a draw
    vec.step(torch.zeros(4, 2, dtype=torch.int8, device="cuda"))
    assert not np.array_equal(bpf.draws()[0].cpu().numpy(), u)     # keyed by the step


def test_refusals_on_a_live_handle():
    import ctypes as C
    from radiation_ppo_amd import _lib
    vec, bpf = _open(3, 1, 0, 64)
    lib = vec.lib
    alive = torch.ones(3, dtype=torch.uint8, device="cuda")
    a8 = torch.zeros(3, 1, dtype=torch.int8, device="cuda")
    p = lambda t: t.data_ptr()
    assert lib.rs_bpf_track(vec._h, bpf._p, bpf._s, p(vec.obs), p(alive), 1, vec._stream()) == 0
    fields = [p(t) for t in (bpf.xp, bpf.w, bpf.logw, bpf.estimate, bpf.neff, bpf.rdiv, bpf.flags, bpf.scratch)]
    for pairs, nbytes in ((4, bpf.scratch.numel() * 8), (3, 8)):                 # not the handle's N * A; too little scratch
        st = C.c_void_p()
        assert lib.rs_bpf_state_create(pairs, *fields, nbytes, C.byref(st)) == 0
        assert lib.rs_bpf_track(vec._h, bpf._p, st, p(vec.obs), p(alive), 1, vec._stream()) == _lib.RS_ERR_INVALID_ARG
        assert lib.rs_ridfim_eval_step(vec._h, bpf._p, st, p(vec.obs), p(alive), p(a8), None, None, vec._stream()) == _lib.RS_ERR_INVALID_ARG
        lib.rs_bpf_state_destroy(st)
    assert lib.rs_ridfim_eval_step(vec._h, bpf._p, bpf._s, p(vec.obs), p(alive), None, None, None, vec._stream()) == _lib.RS_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        bpf.configure(num_particles=3)
    with pytest.raises(RuntimeError):
        bpf.configure(sigma_xy=-1.0)
    torch.cuda.synchronize()
