"""The cases, the teams and the host-side model of the any-side RAD-TEAM (CNN) team kernels (tests/test_cnn_sized_team_eval_gpu.py,
tests/test_cnn_sized_team_step_gpu.py, through tests/_cnn_team_drive.py) and their CPU self-check (tests/test_cnn_sized_team_eval_cpu.py).

The rule is tests/_cnn_team_ref.py's, in its one copy there (its docstring; reference / value_ratios / ratios / passes / torch32), with
the first layer's term taken at the case's depth: a dot product of depth flat = 16 P P behind the bias, K1 = k1(flat) =
2 (sqrt(flat + 1) + 1).  At these depths the rule is loose -- the float32 torch composition sits at 0.07 of the y1 allowance at depth 256
and at 0.0003 at depth 85 264, a dropped tail of 4 terms would pass --, which is why the GPU tests also have an exact one-hot check of the
first layer, at the k listed here: onehot_ks (the evaluation head's wave quarters) and onehot_ks_sliced (the k-split step head's)."""
import torch

import _cnn_team_ref as T

DRAW_CAP = T.DRAW_CAP
SCALE = T.SCALE
# pooled side P -> the map side M the team is built for (P = M // 2).  Wave quarters of 4 P P floats: 2 pieces (P = 4), 3 pieces + 4
# floats (5), tail 16 (14), tail 4 (15), tail 0 (16) and the walls-off depth 85 264 (73: 666 pieces + 4 floats)
SIDE = {4: 8, 5: 11, 14: 28, 15: 31, 16: 33, 73: 147}
HEAD_CASES = ([(15, N, 3) for N in (1, 31, 32, 33, 63, 64, 65, 130)] + [(73, 64, 8), (73, 33, 2), (73, 130, 2)]
              + [(P, N, 2) for P in (4, 5, 14, 16) for N in (1, 65)])


def flat_of(P):
    return 16 * P * P


def k1(flat):
    return 2.0 * ((flat + 1) ** 0.5 + 1)


def master_lanes(P, A):
    """every case's lanes are the first N of its team's master lanes: the largest N among the cases of (P, A)"""
    return max(n for p, n, a in HEAD_CASES if (p, a) == (P, A))


def random_maps(N, A, M, seed, density=0.02):
    """Heat maps as a walls-off run produces them, on the CPU: (maps [N, 4, M, M], cells [N, A] int64, pcells [N, A] int64): sparse
    planes, z-scored readings of both signs, every owner somewhere; lanes 3 mod 7 are fresh maps (both cells -1), agents 0 and A - 1
    share a cell on the lanes 5 mod 7."""
    g = torch.Generator().manual_seed(seed)
    maps = torch.rand(N, 4, M, M, generator=g) * (torch.rand(N, 4, M, M, generator=g) < density)
    maps[:, 1] = maps[:, 1] * 6 - 3 * (maps[:, 1] != 0)
    cells = torch.randint(0, M * M, (N, A), generator=g)
    pcells = torch.where(torch.rand(N, A, generator=g) < 0.6, torch.randint(0, M * M, (N, A), generator=g), torch.full((N, A), -1))
    lane = torch.arange(N)
    cells[lane % 7 == 5, A - 1] = cells[lane % 7 == 5, 0]
    maps[:, 0] = torch.round(maps[:, 0] * 3)
    maps[:, 0].view(N, M * M).scatter_add_(1, cells, torch.ones(N, A))
    fresh = lane % 7 == 3
    cells[fresh], pcells[fresh] = -1, -1
    return maps.contiguous(), cells.contiguous(), pcells.contiguous()


def shortcut_units(maps, cells, pcells):
    """The host-side model of the trunk's empty-window rule: bool [N, A, nt, nt], True where the (agent, image, tile) unit does not
    evaluate conv1 -- every element of the tile's 38 x 38 x 4 input window (origin 32 t - 3, clipped to the map) == 0.0 and neither of
    the agent's cells inside that window."""
    N, _, M, _ = maps.shape
    A = cells.shape[1]
    nt = (M // 2 + 15) // 16
    nz = (maps != 0).any(dim=1)                                     # a NaN is != 0, -0.0 is not
    out = torch.zeros(N, A, nt, nt, dtype=torch.bool)
    for ty in range(nt):
        for tx in range(nt):
            r0, c0 = 32 * ty - 3, 32 * tx - 3
            empty = ~nz[:, max(r0, 0):r0 + 38, max(c0, 0):c0 + 38].flatten(1).any(dim=1)
            for a in range(A):
                hit = torch.zeros(N, dtype=torch.bool)
                for at in (cells[:, a], pcells[:, a]):
                    r, c = torch.div(at, M, rounding_mode="floor") - r0, at % M - c0
                    hit |= (at >= 0) & (r >= 0) & (r < 38) & (c >= 0) & (c < 38)
                out[:, a, ty, tx] = empty & ~hit
    return out


class Team:
    pass


_TEAMS = {}


def team(P, A):
    """A actors for SIDE[P] maps (CNNActor, the three Linear layers x SCALE), the master maps (2 % dense) and u / alive of the master
    lanes; built once per (P, A) on the CPU."""
    if (P, A) in _TEAMS:
        return _TEAMS[P, A]
    from radiation_ppo_amd.maps import CNNActor
    t = Team()
    t.A, t.P, t.M, t.flat, t.N = A, P, SIDE[P], flat_of(P), master_lanes(P, A)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7300 + 10 * P + A)
        t.actors = [CNNActor(map_dim=(t.M, t.M)) for _ in range(A)]
    with torch.no_grad():
        for ac in t.actors:
            assert ac.actor[6].weight.shape == (32, t.flat)
            ac.actor[0].bias.uniform_(-0.05, 0.15)
            ac.actor[3].bias.uniform_(-0.1, 0.1)
            for i in (6, 8, 10):
                for p in ac.actor[i].parameters():
                    p.mul_(SCALE)
    t.maps, t.cells, t.pcells = random_maps(t.N, A, t.M, seed=4300 + 10 * P + A)
    g = torch.Generator().manual_seed(199 + 10 * P + A)
    t.u = torch.rand(t.N, A, generator=g)
    t.alive = (torch.rand(t.N, generator=g) < 0.6).to(torch.uint8)
    t.alive[0] = 1
    _TEAMS[P, A] = t
    return t


def trunk_cpu(t):
    """a2 [A, N, flat] by torch's convolutions on the CPU (the CPU self-check's stand-in for the trunk kernel)."""
    from radiation_ppo_amd.maps import actor_stack_from
    with torch.no_grad():
        return torch.stack([t.actors[a].actor[:6](actor_stack_from(t.maps, t.cells, t.pcells, a)) for a in range(t.A)]).contiguous()


def reference(seq, a2, u):
    """_cnn_team_ref.reference with K1 at a2's depth: the float64 policy round of one agent on a float32 a2 [N, flat] and u [N]."""
    return T.reference(seq, a2, u, k1(a2.shape[1]))


ratios, passes, torch32, distinct_actions, alive_for, clone_seq = T.ratios, T.passes, T.torch32, T.distinct_actions, T.alive_for, T.clone_seq


def onehot_ks(P):
    """The k at which the exact check puts its one-hot rows: per wave quarter its first and last float, the first and last float of
    its tail behind the whole 32-float pieces, the piece boundary 31 / 32 and the lane halves' boundaries 15 / 16 (and 7 / 8 of a
    16-float tail)."""
    kw = 4 * P * P
    np_, tail = kw // 32, kw % 32
    ks = set()
    for w in range(4):
        rel = {0, kw - 1, 15, 16, 31, 32, 32 * (np_ - 1), 32 * np_ - 1}
        if tail:
            rel |= {32 * np_, 32 * np_ + tail - 1}
        if tail == 16:
            rel |= {32 * np_ + 7, 32 * np_ + 8}
        ks |= {w * kw + k for k in rel}
    return sorted(ks)


def onehot_ks_sliced(flat, sl):
    """The k of the exact check of the k-split step head, from its slice length: in the first, a middle and the last slice, per wave
    quarter (a quarter of the slice length, cut at the slice's end) its first and last float, 15 / 16, 31 / 32, the last float of its
    whole pieces, the first and last float of a tail and 7 / 8 inside it; and both sides of every slice boundary."""
    n_sl, q = -(-flat // sl), sl // 4
    ks = set()
    for s in sorted({0, n_sl // 2, n_sl - 1}):
        L = min(sl, flat - s * sl)
        for w in range(4):
            lw = max(0, min(q, L - w * q))
            np_, tail = lw // 32, lw % 32
            rel = {0, lw - 1, 15, 16, 31, 32, 32 * np_ - 1}
            if tail:
                rel |= {32 * np_, 32 * np_ + 7, 32 * np_ + 8, 32 * np_ + tail - 1}
            ks |= {s * sl + w * q + k for k in rel if 0 <= k < lw}
    for s in range(1, n_sl):
        ks |= {s * sl - 1, s * sl}
    assert all(0 <= k < flat for k in ks) and {0, flat - 1} <= ks
    return sorted(ks)
