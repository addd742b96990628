"""CPU-side checks of the PFGRU training pass at the widths of the sized kernels (csrc/rs_pfgru_sized_train.hip): the packer and the
unpacker against the library's own sizes, the new symbols, and the fairness of the float64 bound at wider layers -- the float32 library
path (RNNAgentPPO.model_loss + autograd on the CPU) stays within a tenth of the bound the kernel is held to in
test_pfgru_sized_train_gpu.py, as test_f64_references.py shows at 24 units."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402
from test_pfgru_sized_train_gpu import check_grads  # noqa: E402

WIDTHS = (8, 16, 24, 32, 40, 48, 56, 64)


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


def test_sized_train_symbols_exist(lib):
    for name in ("rs_pfgru_sized_train", "rs_pfgru_sized_draws", "rs_pfgru_sized_train_weight_floats", "rs_pfgru_sized_train_grad_floats"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("H", WIDTHS)
def test_pack_and_unpack_round_trip(lib, H):
    """pack_sized_train_weights fills rs_pfgru_sized_train_weight_floats(H) floats with every parameter in both layouts;
    unpack_sized_train_grads maps every parameter to its own range of a slab of rs_pfgru_sized_train_grad_floats(H) floats: a slab
    that numbers its floats comes back as distinct numbers, each parameter's in its documented place, all inside the slab."""
    from radiation_ppo_amd.pfgru import PFGRUCell
    from radiation_ppo_amd.rada2c import pack_sized_train_weights, sized_train_floats, unpack_sized_train_grads
    torch.manual_seed(H)
    cell = PFGRUCell(hidden_size=H)
    nw, ng = lib.rs_pfgru_sized_train_weight_floats(H), lib.rs_pfgru_sized_train_grad_floats(H)
    assert (nw, ng) == sized_train_floats(H) and nw > 0 and ng > 0
    w = pack_sized_train_weights(cell)
    assert w.shape == (nw,) and w.dtype == torch.float32
    K, Rr = H + 3, 2 * H
    zr = torch.cat([cell.fc_z.weight, cell.fc_r.weight], 0).detach()
    o = 0
    for blk in (zr.t(), torch.cat([cell.fc_z.bias, cell.fc_r.bias]), cell.fc_n.weight.t(), cell.fc_n.bias, zr, cell.fc_n.weight,
                cell.fc_obs.weight, cell.fc_obs.bias, cell.hid_obs[0].weight.t(), cell.hid_obs[0].bias, cell.hid_obs[0].weight,
                cell.hid_obs[2].weight, cell.hid_obs[2].bias):
        n = blk.numel()
        assert torch.equal(w[o:o + n], blk.detach().reshape(-1)), o
        o += n
    assert o == 4 * K * Rr + 2 * Rr + K + 1 + 48 * H + 74 and 0 <= nw - o < 16 and bool((w[o:] == 0).all())
    slab = torch.arange(ng, dtype=torch.float32)
    by_name = unpack_sized_train_grads(cell, slab)
    seen = torch.zeros(ng, dtype=torch.int32)
    for name, p in cell.named_parameters():
        g = by_name[name]
        assert g.shape == p.shape, name
        seen[g.reshape(-1).long()] += 1
    assert set(by_name) == {n for n, _ in cell.named_parameters()}
    assert int(seen.max()) == 1 and int(seen.sum()) == sum(p.numel() for p in cell.parameters())      # distinct ranges
    C = H + 4
    assert by_name["fc_z.weight"][1, 2] == C + 2 and by_name["fc_r.bias"][0] == H * C + H + 3
    assert by_name["fc_n.weight"][H, 0] == 2 * H * C + H * C and by_name["fc_obs.bias"][0] == 4 * H * C + 24 * (H + 1) + 50 + C - 1
    assert by_name["hid_obs.0.bias"][1] == 4 * H * C + (H + 1) + H and by_name["hid_obs.2.weight"][1, 0] == 4 * H * C + 24 * (H + 1) + 25


@pytest.mark.parametrize("H", [8, 32, 64])
def test_float32_library_path_stays_within_a_tenth_of_the_bound(H):
    """RNNAgentPPO.model_loss + autograd in float32 on the CPU against R.model_loss_f64 on the ragged (40, 24) case with the L1 terms
    on: the loss within 0.1 x 5e-6 of the sum of its absolute terms, every gradient block within 0.1 x K13's bound (check_grads).  The
    bound the kernel is held to was fixed for 24 units; this shows it leaves the same room at K = H + 3 = 11, 35 and 67 term sums."""
    from radiation_ppo_amd.rada2c import BpArgs, RecordedDraws, RNNAgentPPO
    seed = 3                                   # (fewer than 20 % of the outputs clamped at all three widths: test_pfgru_sized_train_gpu.py)
    B = R.k13_batch(40, 24, seed, True, True)
    bpa = BpArgs(l2_weight=1.0, l1_weight=0.5, elbo_weight=1.0, area_scale=2500.0)
    torch.manual_seed(5)
    ag = RNNAgentPPO(id=0, seed=1, bp_args=bpa, device="cpu", actor_critic_args=dict(hidden_sizes_rec=(H,)))
    cell = R.k13_cell(ag.agent.model, seed)
    L, E = B.X.shape[0], B.X.shape[1]
    pf, eps, idx = R.k13_draws(L, E, 100 + seed, H=H)
    res, g64, _ = R.k13_reference(cell, B, bpa, pf, eps, idx)
    assert res.clamped < 0.2, res.clamped
    cell.train()
    loss32 = ag.model_loss(B, slice(0, E), RecordedDraws(pf, None, eps, idx))
    loss32.backward()
    lerr = abs(float(loss32.detach()) - float(res.loss.detach())) / (5e-6 * float(res.mags))
    rep = []
    worst = check_grads({k: p.grad for k, p in cell.named_parameters()}, g64, H, f"library H{H}", scale=0.1, report=rep)
    print(f"library path H{H} L {L} E {E}: loss {lerr:.4f} of the bound, worst block {0.1 * worst:.4f} of the bound | "
          + " ".join(f"{k} {0.1 * v:.4f}" for k, v in rep))
    assert lerr <= 0.1
