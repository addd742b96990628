"""The empty-unit algebra of the occupancy-aware tiled trunk (tests/_cnn_sized_occ_ref.py) against autograd in float64, without a
GPU: occupied units from autograd, empty units from the shortcut, the sum against autograd of the whole nn.Sequential trunk on the
dense stack; and the shared inputs hold every class of unit the kernels tell apart."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_sized_occ_ref as R  # noqa: E402

SIDES = [34, 35, 64, 147]
S, A, AGENT = 12, 2, 1


def _case(M):
    from radiation_ppo_amd.maps import CNNActor, CNNCritic, actor_stack_from
    torch.manual_seed(M)
    actor, critic = CNNActor(map_dim=(M, M)).double(), CNNCritic(map_dim=(M, M)).double()
    R.set_biases(actor.actor, M)
    R.set_biases(critic.critic, M + 1)
    maps, cells, pcells = R.occ_inputs(M, S, A, AGENT, seed=M)
    return actor, critic, maps, cells, pcells, actor_stack_from(maps, cells, pcells, AGENT).double()


@pytest.mark.parametrize("M", SIDES)
def test_empty_unit_shortcut_equals_autograd(M):
    actor, critic, maps, cells, pcells, dense_actor = _case(M)
    for name, seq, dense, agent in (("actor", actor.actor, dense_actor, AGENT), ("critic", critic.critic, maps.double(), -1)):
        assert float(seq[0].bias.detach().min()) < 0 < float(seq[0].bias.detach().max())            # channels with c1 = 0 and with c1 > 0
        empty = R.empty_ref(maps, cells, pcells, agent)
        ref_seq = copy.deepcopy(seq)
        x = dense
        for layer in list(ref_seq)[:6]:
            x = layer(x)
        wgt = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(M + 7))
        (x * wgt).sum().backward()
        want = [ref_seq[0].weight.grad, ref_seq[0].bias.grad, ref_seq[3].weight.grad, ref_seq[3].bias.grad]
        got, a2 = R.trunk_grads_with_shortcut(seq, dense, empty, wgt)
        assert torch.equal(a2.flatten(1), x.detach())
        for k, g, w in zip(("dW1", "db1", "dW2", "db2"), got, want):
            # float64 round-off: both sides sum up to n = S * P * P <= 6.4e4 terms in different orders; the worst case is n * 2^-53 =
            # 7e-12 of the terms' magnitudes, which stay within an order of magnitude of the largest gradient
            scale = max(float(w.abs().max()), 1e-30)
            assert float((g - w).abs().max()) <= 1e-10 * scale, (name, M, k, float((g - w).abs().max()), scale)
        # the shortcut is not vacuous: the empty units carry gradient
        short = R.empty_unit_grads((wgt.view(x.shape[0], 16, M // 2, M // 2) * (x.view(x.shape[0], 16, M // 2, M // 2) > 0)).detach(),
                                   R.unit_masks(empty, M), seq[0].bias.detach(), seq[3].weight.detach())
        assert float(short[2].abs().max()) > 0 and float(short[1].abs().max()) > 0 and float(short[3].abs().max()) > 0


@pytest.mark.parametrize("M", SIDES)
def test_inputs_hold_every_unit_class(M):
    _, _, maps, cells, pcells, _ = _case(M)
    nt, P = R.tiles_per_side(M), M // 2
    kinds = [R.KINDS[i % len(R.KINDS)] for i in range(S)]
    flags = R.flags_ref(maps)
    empty = R.empty_ref(maps, cells, pcells, AGENT).view(S, nt, nt)
    zero_window = (flags == 0).view(S, nt, nt)
    special = torch.tensor([k in ("zero", "dense") for k in kinds])
    for i, k in enumerate(kinds):                                    # an all-zero image and a fully dense image
        if k == "zero":
            assert bool(empty[i].all()) and float(maps[i].abs().sum()) == 0
        if k == "dense":
            assert not bool(empty[i].any()) and bool((maps[i] != 0).all())
    assert "zero" in kinds and "dense" in kinds
    rest = empty[~special]
    assert int((~rest).sum()) >= 1 and 2 * int(rest.sum()) >= rest.numel()          # an occupied unit; at least half empty
    edge = torch.zeros(nt, nt, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    corner = torch.zeros(nt, nt, dtype=torch.bool)
    for y in (0, -1):
        for x in (0, -1):
            corner[y, x] = True
    assert bool((rest & edge).any()) and bool((rest & corner).any())                # empty on an edge, empty in a corner
    if nt > 2:                                                                      # (two tiles a side: every unit is both)
        assert bool((rest & edge & ~corner).any())
    if M == 147:
        assert bool((rest & ~edge).any())                                           # empty away from the map's edge
    if P == 17:
        assert bool(rest[:, 1, :].any()) and bool(rest[:, :, 1].any())              # the one-cell-wide tiles of P = 17
    # an empty unit next to an occupied one
    occupied = ~rest
    near = torch.zeros_like(rest)
    near[:, 1:] |= occupied[:, :-1]
    near[:, :-1] |= occupied[:, 1:]
    near[:, :, 1:] |= occupied[:, :, :-1]
    near[:, :, :-1] |= occupied[:, :, 1:]
    assert bool((rest & near).any())
    # a unit whose window is all zero but holds the owner's cell in its 3-pixel ring outside the tile
    found = False
    for name, at in (("loc", cells[:, AGENT]), ("pc", pcells[:, AGENT])):
        inside = R.cell_in_window(at, M).view(S, nt, nt)
        r, c = torch.div(at, M, rounding_mode="floor"), at % M
        for ty in range(nt):
            for tx in range(nt):
                in_tile = (r >= 32 * ty) & (r < 32 * ty + 32) & (c >= 32 * tx) & (c < 32 * tx + 32)
                hit = zero_window[:, ty, tx] & inside[:, ty, tx] & ~in_tile
                found |= bool(hit.any())
                assert not bool((hit & empty[:, ty, tx]).any())
    assert found
    assert bool((pcells[:, AGENT] == -1).any()) and bool((cells[:, AGENT] == -1).any())
    # a critic has no owner cells: the ring units are empty for it
    assert int(R.empty_ref(maps, None, None, -1).sum()) > int(empty.sum())


def test_flag_rule_on_nan_and_negative_zero():
    M = 64
    maps = torch.zeros(3, 4, M, M)
    maps[0, 2, 40, 10] = float("nan")              # tile (1, 0) only: row 40 is outside tile row 0's window [0, 35)
    maps[1, 1, 5, 5] = -0.0
    maps[2, 0, 31, 31] = 1.0                       # pixel 31 lies in the windows of both tiles of an axis
    f = R.flags_ref(maps)
    assert f.tolist() == [[0, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]]
