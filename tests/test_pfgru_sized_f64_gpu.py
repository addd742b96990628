"""rs_pfgru_sized_step_recorded (csrc/rs_pfgru_sized.hip, the <H, true> instantiations) at every width H = 8, 16, .., 64 against
PFGRUCell.forward in float64 on the CPU.  The recorded form takes the noise and the resampling indices as inputs, so the whole step
-- gates, reparameterisation, observation likelihood, resampled weights, weighted mean and hid_obs -- is held to float64 with no
near-tie exception.  Several (owner, env) sets share a workgroup (the kernel packs 6), N = 1, 6, 7, 200 (7: a second workgroup with
one set), A = 1, 3, 8 owners with their own weights, the mask on alternate steps, carry_hidden on and off, 4 steps."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16, 24, 32, 40, 48, 56, 64)
P = 40


def _cells(A, H):
    from radiation_ppo_amd.pfgru import PFGRUCell
    cells = []
    for a in range(A):
        torch.manual_seed(100 * H + a)
        c = PFGRUCell(hidden_size=H)
        with torch.no_grad():
            for p in c.parameters():
                p.mul_(2.0)                                    # livelier gates than the default initialisation (test_pfgru_sized_gpu)
            c.hid_obs[2].bias.add_(0.75)                       # most predictions above hid_obs's final ReLU, some clamped at 0
        cells.append(c)
    return cells


def _indices(A, N, t, g):
    """Random resampling indices, with (owner a, env 0) the identity on even steps and one repeated particle on odd ones, and the
    last env the other of the two."""
    idx = torch.randint(0, P, (A, N, P), generator=g)
    ident, rep = torch.arange(P), torch.full((P,), int(torch.randint(0, P, (1,), generator=g)))
    idx[:, 0] = ident if t % 2 == 0 else rep
    if N > 1:
        idx[:, N - 1] = rep if t % 2 == 0 else ident
    return idx


@pytest.mark.parametrize("carry", [True, False])
@pytest.mark.parametrize("H", WIDTHS)
def test_sized_recorded_step_matches_float64(H, carry):
    """pred, h and p against the float64 cell stepped from its own float64 state (carry on: the kernel's state stays in its quad-major
    buffers from step to step; carry off: the kernel writes no state back, so h and p keep their bits and the reference steps from the
    initial state every time).  Masked-out envs keep the bits of pred, h and p.
    Tolerances: h1 = (1 - z) n + z h0 with z a sz_sigmoid of a K = H + 3 term sum (<= ~8 u of its |terms|, then rcp + exp2: ~4 u +
    u |x|) and n a tanh of mu + eps softplus(var) (two more such sums and a log / exp2 / rcp chain); |h| <= ~1, so ~2e-6 per step,
    carried through up to 4 steps: rtol 2e-5, atol 1e-5 of the scale.  p (log weights, |p| ~ 3-10): log-softmax with sz_exp / sz_log
    (1 ulp of |p| ~ 1e-6 each, a few per step): rtol 2e-5, atol 1e-5 of the scale.  pred: the weighted mean of 40 particles, then a
    24-unit and a 2-unit layer with ReLUs; outputs whose float64 pre-activations (or a hidden unit's) lie within 1e-4 of a ReLU kink are
    left out, where float32 may take the other branch (R.hid_obs_fragile); the others rtol 1e-4, atol 1e-5 of the scale plus 2e-6
    absolute (an output near 0 is a sum of 24 terms of ~0.1 that cancel: the mean particle's ~1e-6 error carried through the two
    layers does not shrink with it).  All within the bounds of the float32 check of the same outputs (test_pfgru_sized_gpu: rtol 1e-4,
    atol 2e-5)."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.pfgru import PredictorBank, pack_sized_weights
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kept = counted = 0                                                 # pred outputs compared (non-zero ones) / of the live envs
    for N in (1, 6, 7, 200):
        for A in (1, 3, 8):
            key = (H, carry, N, A)
            cells = _cells(A, H)
            c64 = [R.f64(c) for c in cells]
            w = pack_sized_weights([c.cuda() for c in cells])
            g = torch.Generator().manual_seed(H * 1000 + N * 10 + A)
            h0 = torch.rand(A, N, P, H, generator=g)
            p0 = torch.log_softmax(torch.randn(A, N, P, generator=g), dim=-1)
            hq = PredictorBank.to_quads(h0).cuda().contiguous()
            pk = p0.cuda().contiguous()
            pred = torch.full((N, A, 2), -5.0, device="cuda")
            ref_h, ref_p = h0.double(), p0.double()
            for t in range(4):
                kt = key + (t,)
                obs = torch.rand(N, A, 11, generator=g)
                obs[..., 0] = torch.randint(0, 4000, (N, A), generator=g).float() / 100.0 - 10.0
                eps = torch.randn(A, N, P, H, generator=g)
                idx = _indices(A, N, t, g)
                mask = None if t % 2 == 0 else (torch.rand(N, generator=g) < 0.6).to(torch.uint8)
                if mask is not None and N > 1:
                    mask[0], mask[N - 1] = 1, 0
                hq_before, p_before, pred_before = hq.clone(), pk.clone(), pred.clone()
                # device copies held by name until the launch has run (a temporary's block could be handed to the next copy)
                oc, ec, ic = obs.cuda(), eps.cuda().contiguous(), idx.to(torch.int32).cuda().contiguous()
                mc = None if mask is None else mask.cuda()
                _lib.check(lib.rs_pfgru_sized_step_recorded(w.data_ptr(), oc.data_ptr(), hq.data_ptr(), pk.data_ptr(), ec.data_ptr(), ic.data_ptr(),
                                                            None if mc is None else mc.data_ptr(), 1 if carry else 0, 0.7, pred.data_ptr(),
                                                            N, A, H, st), "rs_pfgru_sized_step_recorded")
                torch.cuda.synchronize()
                on = torch.ones(N, dtype=torch.bool) if mask is None else mask.bool()
                got_h, got_p, got_pred = PredictorBank.from_quads(hq.cpu()), pk.cpu(), pred.cpu()
                new_h, new_p = ref_h.clone(), ref_p.clone()
                for a in range(A):
                    pr64, h1, p1, mean = R.pfgru_step_f64(c64[a], obs[:, a, :3].double(), ref_h[a], ref_p[a], eps[a].double(), idx[a])
                    keep = ~R.hid_obs_fragile(c64[a], mean, 1e-4) & on.view(N, 1)
                    kept += int((keep & (pr64 != 0)).sum()); counted += 2 * int(on.sum())
                    R.close(got_pred[:, a][keep], pr64[keep], f"pfgru pred {kt} a={a}", rtol=1e-4, noise=1e-5, tiny=2e-6)
                    if carry:
                        R.close(got_h[a][on], h1[on], f"pfgru h {kt} a={a}", rtol=2e-5, noise=1e-5)
                        R.close(got_p[a][on], p1[on], f"pfgru p {kt} a={a}", rtol=2e-5, noise=1e-5)
                        new_h[a][on], new_p[a][on] = h1[on], p1[on]
                # masked-out envs: not a bit of pred, h or p changes; carry off: no state is written at all
                off = ~on
                assert torch.equal(pred.cpu()[off], pred_before.cpu()[off]), kt
                if carry:
                    assert torch.equal(hq.cpu()[:, off], hq_before.cpu()[:, off]) and torch.equal(pk.cpu()[:, off], p_before.cpu()[:, off]), kt
                    ref_h, ref_p = new_h, new_p
                else:
                    assert torch.equal(hq, hq_before) and torch.equal(pk, p_before), kt
            assert not math.isnan(float(pred.sum()))
    # most compared predictions are non-trivial: neither left out by the kink mask nor clamped to 0 by the final ReLU
    assert kept >= 0.6 * counted, (kept, counted)
