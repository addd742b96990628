"""The PFGRU training pass at the widths of the sized kernels (csrc/rs_pfgru_sized_train.hip: rs_pfgru_sized_train, rs_pfgru_sized_draws)
against float64 on the CPU, through RNNAgentPPO.model_pass_hip / update_model -- test_pfgru_default_f64_gpu.py's K13 tests at H = 8 .. 64.
The references (tests/_f64_ref.py: k13_batch, k13_draws, k13_cell, k13_reference / model_loss_f64) follow cell.h_dim and are used as they
are; the bounds are K13's own (see check_grads); the float32 library path is held to a tenth of them at these widths in
test_pfgru_sized_train_cpu.py."""
import ctypes as C
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

P = 40
WIDTHS = (8, 16, 32, 40, 64)            # one per occupancy tier of the sized kernels, and both ends
DEFAULT, WITH_L1, L1_ONLY = (1.0, 0.0, 1.0), (1.0, 0.5, 1.0), (0.0, 1.0, 1.0)


# Seeds (cell perturbation, batch and draws alike) at which the float64 reference meets the K13 test's condition that fewer than 20 % of
# the location outputs are clamped by hid_obs's final ReLU: at 8 and 16 units R.k13_cell's perturbation alone decides the sign of an
# output for about half of the seeds (a whole output column clamped: 0.5), 6 does so at 40 units; found on the CPU with the float64
# reference alone, before the kernel existed.
RAGGED_SEEDS = {8: (1, 3, 5, 6), 16: (1, 3, 5, 6), 32: (1, 3, 5, 6), 40: (1, 3, 5, 9), 64: (1, 3, 5, 6)}


def _cases():
    """(H, T, N, ragged, sort_by_length, (l2, l1, elbo), seed); the one-step shapes first, so that an addressing fault shows there."""
    out = []
    for (T, N), seed in (((1, 1), 1), ((1, 70), 3)):
        for H in WIDTHS:
            out.append((H, T, N, False, False, DEFAULT, seed))
    for H in WIDTHS:
        seeds = iter(RAGGED_SEEDS[H])
        for srt in (True, False):
            for wts in (DEFAULT, WITH_L1):
                out.append((H, 40, 24, True, srt, wts, next(seeds)))
    out.append((32, 40, 24, True, False, L1_ONLY, 7))
    out.append((64, 120, 3, False, False, DEFAULT, 4))
    return out


CASES = _cases()


def _case_id(c):
    H, T, N, ragged, srt, (l2, l1, elbo), _ = c
    return f"H{H}-T{T}-N{N}{'-ragged' if ragged else ''}{'-sorted' if srt else ''}-l2_{l2:g}-l1_{l1:g}-elbo_{elbo:g}"


def block_rows(H):
    """_f64_ref.BLOCK_ROWS at width H: the mu / var split of fc_n's rows is at H (there it is fixed at 24)."""
    one = (("", slice(None)),)
    return {"fc_z": one, "fc_r": one, "fc_n": (("[mu]", slice(0, H)), ("[var]", slice(H, 2 * H))), "fc_obs": one, "hid_obs.0": one,
            "hid_obs.2": one}


def grad_blocks(grads, H):
    out = {}
    for name, g in grads.items():
        layer, kind = name.rsplit(".", 1)
        for blk, rows in block_rows(H)[layer]:
            out[f"{layer}.{kind}{blk}"] = g[rows]
    return out


def check_grads(got, ref64, H, name, scale=1.0, report=None):
    """_f64_ref.check_k13_grads with the block table of width H.  K13's bound (test_pfgru_default_f64_gpu.py): every block within
    scale x (rtol 1e-4 + noise 1e-4 of the block's own largest element + a floor of 2e-6 of the cell's largest gradient element);
    fc_obs.bias, exactly 0 in exact arithmetic, is held to the floor alone.  (All cases here are below 120 x 65 step-episodes, where
    K13's noise term is 1e-4.)  No allowance for ReLU / |.| kinks.  Returns the worst ratio; report receives (block, ratio)."""
    a, b = grad_blocks(got, H), grad_blocks(ref64, H)
    floor = 2e-6 * max(float(v.abs().max()) for v in b.values())
    ratios = []
    for blk in b:
        x, y = a[blk].detach().double().cpu(), b[blk].detach().double().cpu()
        assert x.shape == y.shape and bool(torch.isfinite(x).all()), (name, blk)
        allowed = scale * (floor if blk == "fc_obs.bias" else 1e-4 * y.abs() + 1e-4 * float(y.abs().max()) + floor)
        ratios.append((blk, float(((x - y).abs() / allowed).max())))
    if report is not None:
        report.extend(ratios)
    bad = [(blk, round(r, 3)) for blk, r in ratios if not r <= 1.0]
    assert not bad, (name, bad)
    return max(r for _, r in ratios)


def _agent(H, wts, seed, **kw):
    from radiation_ppo_amd.rada2c import BpArgs, RNNAgentPPO
    l2, l1, elbo = wts
    bpa = BpArgs(l2_weight=l2, l1_weight=l1, elbo_weight=elbo, area_scale=2500.0)
    torch.manual_seed(5)
    ag = RNNAgentPPO(id=0, seed=1, bp_args=bpa, actor_critic_args=dict(hidden_sizes_rec=(H,)), **kw)
    assert ag.agent.sized_pfgru and not ag.agent.fused_pfgru and ag.agent.model.h_dim == H
    R.k13_cell(ag.agent.model, seed)
    return ag, bpa


def _report(line):
    """One line per case for the record of measured error ratios (profiles/r06_pfgru_sized_train_error_ratios.txt)."""
    print("sized train f64:", line)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_sized_training_pass_matches_float64(case):
    """rs_pfgru_sized_train through RNNAgentPPO.model_pass_hip with recorded draws (RecordedKernelDraws: the indices are the kernel's
    input, u = NULL) against R.model_loss_f64 + float64 autograd, fed what model_pass_hip hands the kernel.  Widths 8, 16, 32, 40, 64;
    one one-step episode; 70 one-step episodes; ragged episodes of 1 .. 40 steps sorted by length and not, each with the default loss
    weights (1, 0, 1) and with (1, 0.5, 1); the L1 terms alone (0, 1, 1) at 32 units; three 120-step episodes at 64 units.
    Bounds, K13's: the loss within 5e-6 of the sum of its absolute per-(step, episode) terms; the gradients per block (check_grads).
    Fewer than 20 % of the float64 location outputs are clamped by the final ReLU; no kink masking; the recorded indices come back
    untouched on valid steps; a second launch returns the same bits."""
    from radiation_ppo_amd.rada2c import RecordedKernelDraws, unpack_sized_train_grads
    H, T, N, ragged, srt, wts, seed = case
    name = _case_id(case)
    ag, bpa = _agent(H, wts, seed)
    cell = ag.agent.model
    B = R.k13_batch(T, N, seed, ragged, srt, device="cuda")
    L, E = B.X.shape[0], B.X.shape[1]
    pf, eps, idx = R.k13_draws(L, E, 100 + seed, H=H)
    res, g64, _ = R.k13_reference(cell, B, bpa, pf, eps, idx)
    assert res.clamped < 0.2, res.clamped
    if ragged:
        lens = B.lens.tolist()
        assert 1 in lens and T in lens and (lens == sorted(lens, reverse=True)) == srt
    sl = slice(0, E)
    d = RecordedKernelDraws(pf.cuda(), None, eps.cuda(), idx.cuda())
    loss_k, slab, idx_k = ag.model_pass_hip(B, sl, d)
    loss_k, slab = float(loss_k), slab.clone()
    assert torch.equal(idx_k.cpu().long()[B.valid.cpu()], idx[B.valid.cpu()])            # the indices are inputs: untouched
    loss_2, slab_2, _ = ag.model_pass_hip(B, sl, d)
    assert float(loss_2) == loss_k and torch.equal(slab, slab_2), name                   # bitwise repeatable
    lerr = abs(loss_k - float(res.loss.detach())) / (5e-6 * float(res.mags))
    rep = []
    try:
        worst = check_grads(unpack_sized_train_grads(cell, slab), g64, H, name, report=rep)
    finally:
        _report(f"{name} L {L} E {E} loss {lerr:.4f} kinks {res.kinks}/{res.samples} clamped {res.clamped:.3f} | "
                + " ".join(f"{k} {v:.4f}" for k, v in rep))
    assert math.isfinite(loss_k) and lerr <= 1.0, (name, loss_k, float(res.loss.detach()), lerr)
    assert worst <= 1.0


@pytest.mark.parametrize("H", [16, 64])
def test_sized_training_pass_with_hashed_draws_matches_float64(H):
    """The pass through KernelDraws(H=H) (rs_pfgru_sized_draws: the kernel picks the resampling indices) on the ragged case: the
    float64 reference fed the kernel's own indices, the same bounds; and the indices against the float64 inverse CDF of the same
    uniforms, continued from the kernel's choice so that one moved index cannot cascade: all but 2 of the valid (step, episode) rows
    take the same 40 particles (the cap of test_k13_with_hashed_draws_matches_float64)."""
    from radiation_ppo_amd.rada2c import KernelDraws, unpack_sized_train_grads
    seed = 8
    name = f"hashed H{H}"
    ag, bpa = _agent(H, WITH_L1, seed)
    cell = ag.agent.model
    B = R.k13_batch(40, 24, seed, True, True, device="cuda")
    L, E = B.X.shape[0], B.X.shape[1]
    kd = KernelDraws(B.key * 64 + 1, L, H=H)
    loss_k, slab, idx = ag.model_pass_hip(B, slice(0, E), kd)
    loss_k, slab, idx = float(loss_k), slab.clone(), idx.clone().cpu().long()
    valid = B.valid.cpu()
    assert int(idx[valid].min()) >= 0 and int(idx[valid].max()) < P
    idx = torch.where(valid.unsqueeze(-1), idx, torch.zeros_like(idx))
    pf, eps, u = kd._pf.cpu(), kd._eps.cpu(), kd._u.cpu()
    res, g64, c64 = R.k13_reference(cell, B, bpa, pf, eps, idx)
    lerr = abs(loss_k - float(res.loss.detach())) / (5e-6 * float(res.mags))
    rep = []
    try:
        check_grads(unpack_sized_train_grads(cell, slab), g64, H, name, report=rep)
    finally:
        _report(f"{name} L {L} E {E} loss {lerr:.4f} | " + " ".join(f"{k} {v:.4f}" for k, v in rep))
    assert lerr <= 1.0, (loss_k, float(res.loss.detach()))
    same = tot = 0
    with torch.no_grad():
        h, p = pf.double(), torch.full((E, P), math.log(1 / P), dtype=torch.float64)
        X3 = B.X[..., :3].cpu().double()
        for t in range(L):
            _, (hu, _) = c64(X3[t], (h, p), eps[t].double(), resample_u=u[t])
            _, (h, p) = c64(X3[t], (h, p), eps[t].double(), resample_idx=idx[t])
            ok = ((hu - h).abs().amax(dim=(1, 2)) < 1e-12) & valid[t]
            same += int(ok.sum()); tot += int(valid[t].sum())
    assert same >= tot - 2, (same, tot)


@pytest.mark.parametrize("H", [8, 64])
def test_sized_kernel_draws_equal_hash_draws(H):
    """rs_pfgru_sized_draws against the torch composition of the same counter hash (HashDraws(keys, H=H)): the uniforms bit for bit,
    the normals within float32 rounding of the library log / cos (the tolerance of test_kernel_draws_equal_hash_draws)."""
    from radiation_ppo_amd.rada2c import HashDraws, KernelDraws
    keys = (torch.arange(257, dtype=torch.int64, device="cuda") * 7919 + 12345) * 64 + 3
    L = 9
    kd, hd = KernelDraws(keys, L, H=H), HashDraws(keys, H=H)
    assert kd.pf_h0().shape == (257, P, H) and torch.equal(kd.pf_h0(), hd.pf_h0())
    for t in range(L):
        assert torch.equal(kd.resample(t)["resample_u"], hd.resample(t)["resample_u"]), t
        assert torch.allclose(kd.eps(t), hd.eps(t), rtol=2e-6, atol=2e-6), (t, float((kd.eps(t) - hd.eps(t)).abs().max()))


def _raw(ag, B, pf, eps, idx, w=None, steps=None, episodes=None, hidden=None):
    """rs_pfgru_sized_train on batch B with recorded draws on fresh buffers, as model_pass_hip launches it: (return code, per-episode
    losses [E], gradient slabs [E, grad floats]) before model_pass_hip sums them; loss and slab start at 7."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.rada2c import pack_sized_train_weights
    lib = _lib.load()
    a = ag.bp_args
    H = ag.agent.rec
    X = B.X.contiguous()
    L, E = X.shape[0], X.shape[1]
    tar, bp = R.k13_inputs(B, a)
    tar, bp = tar.contiguous(), bp.contiguous()
    lens, w_ep = B.lens.contiguous(), B.w_ep.float().contiguous()
    dev = X.device
    hs = torch.empty(L, E, 40, H, dtype=torch.float32, device=dev)
    ps = torch.empty(L, E, 2, 40, dtype=torch.float32, device=dev)
    gates = torch.empty(L, E, 4, 40, H, dtype=torch.float32, device=dev)
    ng = lib.rs_pfgru_sized_train_grad_floats(H)
    loss = torch.full((E,), 7.0, dtype=torch.float32, device=dev)
    slab = torch.full((E, ng), 7.0, dtype=torch.float32, device=dev)
    wp = pack_sized_train_weights(ag.agent.model)
    pfc, epc, ic = pf.cuda().contiguous(), eps.cuda().contiguous(), idx.to(torch.int32).cuda().contiguous()
    assert pfc.shape == (E, 40, H) and epc.shape == (L, E, 40, H) and ic.shape == (L, E, 40) and tar.shape == (L, E, 2) and bp.shape == (L, E)
    assert int(lens.max()) <= L and int(lens.min()) >= 1 and int(ic.min()) >= 0 and int(ic.max()) < 40
    rc = lib.rs_pfgru_sized_train(wp.data_ptr() if w is None else w, X.data_ptr(), tar.data_ptr(), bp.data_ptr(), lens.data_ptr(), w_ep.data_ptr(),
                                  pfc.data_ptr(), epc.data_ptr(), None, hs.data_ptr(), ps.data_ptr(), gates.data_ptr(), ic.data_ptr(), loss.data_ptr(),
                                  slab.data_ptr(), L if steps is None else steps, E if episodes is None else episodes,
                                  float(ag.agent.model.resamp_alpha), float(a.l2_weight), float(a.l1_weight), float(a.elbo_weight),
                                  H if hidden is None else hidden, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, loss, slab


def _take(B, keep):
    from radiation_ppo_amd.rada2c import EpisodeBatch
    return EpisodeBatch(X=B.X[:, keep], act=B.act[:, keep], adv=B.adv[:, keep], ret=B.ret[:, keep], logp=B.logp[:, keep], src=B.src[:, keep],
                        valid=B.valid[:, keep], lens=B.lens[keep], w_ep=B.w_ep[keep], key=B.key[keep])


@functools.lru_cache(maxsize=None)
def _ragged_32():
    seed = 8
    ag, _ = _agent(32, WITH_L1, seed)
    B = R.k13_batch(40, 24, seed, True, False, device="cuda")
    return ag, B, R.k13_draws(B.X.shape[0], B.X.shape[1], 100 + seed, H=32)


def test_sized_zero_weight_episodes_have_zero_rows_and_leave_the_others_alone():
    """At 32 units: episodes with w_ep = 0 (every third one, the first and the last among them) get slab rows and losses of exactly 0,
    and the other episodes' rows and losses are bit for bit those of a launch without the zero-weight episodes (one workgroup per
    episode: an episode's arithmetic does not depend on its neighbours)."""
    ag, B, (pf, eps, idx) = _ragged_32()
    B = _take(B, torch.arange(B.lens.shape[0], device="cuda"))
    L, E = B.X.shape[0], B.X.shape[1]
    zero = torch.zeros(E, dtype=torch.bool)
    zero[0::3] = True; zero[E - 1] = True
    B.w_ep = torch.where(zero.cuda(), torch.zeros_like(B.w_ep), B.w_ep)
    rc, loss, slab = _raw(ag, B, pf, eps, idx)
    assert rc == 0
    assert bool((slab[zero.cuda()] == 0).all()) and bool((loss[zero.cuda()] == 0).all())
    keep = (~zero).nonzero().squeeze(1)
    assert int(B.lens[keep.cuda()].max()) == L                                     # the same padded length in both launches
    rc, loss_b, slab_b = _raw(ag, _take(B, keep.cuda()), pf[keep], eps[:, keep], idx[:, keep])
    assert rc == 0
    assert torch.equal(slab[keep.cuda()], slab_b) and torch.equal(loss[keep.cuda()], loss_b)
    assert float(slab_b.abs().max()) > 0 and bool(torch.isfinite(slab_b).all())


def test_sized_train_entry_points_check_their_arguments_before_launching():
    """Hidden 0, 12, 72, a NULL weights pointer and steps = 0 return RS_ERR_INVALID_ARG (1) and launch nothing (loss and slab keep
    their fill); episodes = 0 is a successful no-op.  The same for rs_pfgru_sized_draws."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    ag, B, (pf, eps, idx) = _ragged_32()
    for kw in (dict(hidden=0), dict(hidden=12), dict(hidden=72), dict(w=0), dict(steps=0), dict(episodes=-1)):
        rc, loss, slab = _raw(ag, B, pf, eps, idx, **kw)
        assert rc == 1, kw
        assert bool((loss == 7).all()) and bool((slab == 7).all()), kw
    rc, loss, slab = _raw(ag, B, pf, eps, idx, episodes=0)
    assert rc == 0 and bool((loss == 7).all()) and bool((slab == 7).all())
    keys = torch.arange(4, dtype=torch.int64, device="cuda")
    h0 = torch.full((4, 40, 16), 7.0, device="cuda")
    ep = torch.full((2, 4, 40, 16), 7.0, device="cuda")
    u = torch.full((2, 4, 40), 7.0, dtype=torch.float64, device="cuda")
    args = lambda **k: (k.get("keys", keys.data_ptr()), k.get("E", 4), k.get("L", 2), k.get("H", 16), h0.data_ptr(), ep.data_ptr(), u.data_ptr(), None)
    for k in (dict(H=0), dict(H=12), dict(H=72), dict(keys=None), dict(L=0), dict(E=-1)):
        assert lib.rs_pfgru_sized_draws(*args(**k)) == 1, k
    assert lib.rs_pfgru_sized_draws(*args(E=0)) == 0
    torch.cuda.synchronize()
    assert bool((h0 == 7).all()) and bool((ep == 7).all()) and bool((u == 7).all())
    for Hb in (0, 12, 72):
        assert lib.rs_pfgru_sized_train_weight_floats(Hb) == 0 and lib.rs_pfgru_sized_train_grad_floats(Hb) == 0


class _IdxDraws:
    """The draws of a KernelDraws object with the resampling indices the kernel took (test_rada2c_gpu._KernelIdxDraws)."""

    def __init__(self, kd, idx):
        self.kd, self.idx = kd, idx

    def pf_h0(self):
        return self.kd.pf_h0()

    def eps(self, t):
        return self.kd.eps(t)

    def resample(self, t):
        return dict(resample_idx=self.idx[t].long())


def test_update_model_at_rec_16_runs_the_sized_pass_and_matches_the_library_path():
    """RNNAgentPPO(hidden_sizes_rec=(16,)).update_model on a ragged (40, 24) batch: the pass goes through rs_pfgru_sized_train (one
    timed call per iteration and chunk, draws from rs_pfgru_sized_draws on the keys B.key * 64 + 1 + it); after one Adam step the
    parameters match the library path (use_k13 = False) on the same keys within the post-Adam bound K13 is held to
    (test_rows_f_golden_gpu.py: 5e-6 + 1e-4 |p| where the gradient is above 1e-6, one learning-rate step 5e-3 everywhere) and the
    reported loss to rtol 1e-4.  The library path is handed the indices the kernel took, as in
    test_update_model_on_k13_equals_autograd_path: they are constants of the backward pass on both sides."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.rada2c import KernelDraws, RNNAgentPPO
    B = R.k13_batch(40, 24, 8, True, False, device="cuda")
    L, E = B.X.shape[0], B.X.shape[1]
    res, taken = [], {}
    for hip in (True, False):
        torch.manual_seed(6)
        ag = RNNAgentPPO(id=0, seed=1, train_pfgru_iters=1, actor_critic_args=dict(hidden_sizes_rec=(16,)))
        assert ag.agent.sized_pfgru
        R.k13_cell(ag.agent.model, 8)
        ag.use_k13 = hip
        if hip:
            orig = ag.model_pass_hip

            def recording(Bx, sl, d, _orig=orig):
                out = _orig(Bx, sl, d)
                assert isinstance(d, KernelDraws) and d._pf.shape[-1] == 16
                taken[sl.start] = out[2].clone()
                return out
            ag.model_pass_hip = recording
            _lib.EVENTS = {}
            try:
                loss = ag.update_model(B)
                events = {k: len(v) for k, v in _lib.EVENTS.items()}
            finally:
                _lib.EVENTS = None
            assert events.get("rs_pfgru_sized_train") == 1 and "rs_pfgru_train" not in events, events
            assert list(taken) == [0] and ag.k13_particle_steps == [40 * int(B.lens.sum())]
        else:
            loss = ag.update_model(B, draws_for=lambda it, sl: _IdxDraws(KernelDraws(B.key[sl] * 64 + 1 + it, L, H=16), taken[sl.start]))
        res.append((loss, {k: v.detach().clone() for k, v in ag.agent.model.named_parameters()},
                    {k: v.grad.detach().clone() for k, v in ag.agent.model.named_parameters()}))
    (la, pa, _), (lb, pb, gb) = res
    assert math.isfinite(la) and abs(la - lb) <= 1e-4 * abs(lb), (la, lb)
    for k in pa:
        diff = (pa[k] - pb[k]).abs()
        big = gb[k].abs() > 1e-6
        assert bool((diff[big] <= 5e-6 + 1e-4 * pb[k][big].abs()).all()) and bool((diff <= 5e-3 + 1e-6).all()), (k, float(diff.max()))
