"""The tiled CNN trunk for heat maps of any side (rs_cnn_sized_forward / _backward / _infer through maps.SizedConvTrunk and the
collector) against the same modules' nn.Sequential evaluated by PyTorch in float64 on the CPU on the dense stacks of
maps.actor_stack_from; at 27 x 27 against K9 / K10; and the walls-off collector and update routed through it.
Tolerance: fp32 with a different summation order -- rtol 2e-4 plus a noise term relative to the tensor's scale."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SEED = 289714752


def _random_inputs(S, A, M, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    MM = M * M
    maps = torch.rand(S, 4, M, M, device="cuda", generator=g) * (torch.rand(S, 4, M, M, device="cuda", generator=g) < 0.1)
    maps[:, 1] = maps[:, 1] * 6 - 3                       # z-scored readings take both signs
    cells = torch.randint(0, MM, (S, A), device="cuda", generator=g)
    pcells = torch.where(torch.rand(S, A, device="cuda", generator=g) < 0.6, torch.randint(0, MM, (S, A), device="cuda", generator=g),
                         torch.full((S, A), -1, device="cuda", dtype=torch.int64))
    maps[:, 0] = torch.round(maps[:, 0] * 3)
    maps[:, 0].reshape(S, MM).scatter_add_(1, cells, torch.ones(S, A, device="cuda"))
    # corners, the last row and column (dropped by the pool for odd M, kept for even M) and empty one-hots
    corners = [0, M - 1, MM - M, MM - 1, (M - 1) * M + M // 2, (M // 2) * M + M - 1]
    for i in range(S):
        cells[i, 0] = corners[i % len(corners)]
        pcells[i, A - 1] = corners[(i + 3) % len(corners)]
    if S > 4:
        cells[3, 0] = -1
        pcells[4, A - 1] = -1
    return maps.contiguous(), cells.contiguous(), pcells.contiguous()


def _close(a, b, name, noise=2e-5):
    """b is the float64 reference.  fp32 sums carry ~sqrt(n) * 6e-8 relative noise against the largest element: a weight gradient at
    147 sums 5 329 pooled pixels per image over up to 67 images (n ~ 3.6e5 -> ~4e-5 of the scale in the worst case, ~1e-5 typically),
    so the gradients get noise 1e-4; a2 sums 72 + 54 terms and keeps 2e-5."""
    a = a.detach().double().cpu()
    scale = max(float(b.abs().max()), 1e-6)
    assert torch.allclose(a, b, rtol=2e-4, atol=noise * scale + 1e-6), (name, float((a - b).abs().max()), scale)


def _fragile(seq64, dense64, eps=2e-6):
    """The a2 elements [S, 16 P P] next to a kink of the network in float64, where fp32 and fp64 may legitimately take different
    branches: a conv2 pre-activation within eps of 0, or a pooled cell in the element's 3 x 3 receptive field whose pool window has a
    near-tie (margin within eps) or whose winner's conv1 pre-activation is within eps of 0.  Per element, not per image: at 147 every
    image has some of its 85 264 outputs near a kink."""
    z1 = F.conv2d(dense64, seq64[0].weight, seq64[0].bias, padding=1)
    S, M = dense64.shape[0], dense64.shape[-1]
    P = M // 2
    z1 = z1[:, :, :2 * P, :2 * P]
    blocks = F.unfold(z1, kernel_size=2, stride=2).view(S, 8, 4, P * P)
    rb = torch.relu(blocks)
    distinct = (rb.max(dim=2, keepdim=True).values - rb).abs()
    near_tie = ((distinct > 0) & (distinct < eps)).any(dim=2)
    near_kink = blocks.max(dim=2).values.abs() < eps
    bad_cell = (near_tie | near_kink).any(dim=1).view(S, 1, P, P).double()
    bad_cell = F.max_pool2d(bad_cell, 3, stride=1, padding=1) > 0           # the conv2 outputs that read such a cell
    p1 = F.max_pool2d(torch.relu(z1), 2, 2)
    z2 = F.conv2d(p1, seq64[3].weight, seq64[3].bias, padding=1)
    return (bad_cell | (z2.abs() < eps)).flatten(1)


def _modules(M, seed):
    from radiation_ppo_amd.maps import CNNActor, CNNCritic
    torch.manual_seed(seed)
    actor, critic = CNNActor(map_dim=(M, M)).cuda(), CNNCritic(map_dim=(M, M)).cuda()
    with torch.no_grad():                                  # make biases matter (pool ties on empty regions, ReLU gates)
        for m in (actor.actor, critic.critic):
            m[0].bias.uniform_(-0.05, 0.15)
            m[3].bias.uniform_(-0.1, 0.1)
    return actor, critic


def _check_trunk(seq, maps, cells, pcells, agent, dense64, name):
    """SizedConvTrunk's a2 and the four conv parameter gradients against the float64 trunk seq[0:6] on the dense input."""
    from radiation_ppo_amd.maps import SizedConvTrunk
    seq64 = copy.deepcopy(seq).double().cpu()
    conv = [seq[0].weight, seq[0].bias, seq[3].weight, seq[3].bias]
    for p in conv:
        p.grad = None
    a2 = SizedConvTrunk.apply(maps, cells, pcells, agent, *conv, True)
    ref = dense64
    for layer in list(seq64)[:6]:
        ref = layer(ref)
    _close(a2, ref.detach(), f"{name} a2")
    keep = ~_fragile(seq64, dense64)
    assert keep.float().mean() >= 0.9
    wgt = torch.randn_like(a2) * keep.cuda()
    (a2 * wgt).sum().backward()
    (ref * wgt.double().cpu()).sum().backward()
    conv64 = [seq64[0].weight, seq64[0].bias, seq64[3].weight, seq64[3].bias]
    for k, g1, p0 in zip(("dW1", "db1", "dW2", "db2"), conv, conv64):
        _close(g1.grad, p0.grad, f"{name} {k}", noise=1e-4)


@pytest.mark.parametrize("M", [28, 31, 64, 147, 148])
@pytest.mark.parametrize("S", [1, 3, 67])
def test_sized_trunk_matches_float64(M, S):
    from radiation_ppo_amd.maps import actor_stack_from
    actor, critic = _modules(M, seed=M * 100 + S)
    for A in (1, 3):
        maps, cells, pcells = _random_inputs(S, A, M, seed=M + S + A)
        agent = A - 1
        dense64 = actor_stack_from(maps, cells, pcells, agent).double().cpu()
        _check_trunk(actor.actor, maps, cells, pcells, agent, dense64, f"actor M={M} S={S} A={A}")
    _check_trunk(critic.critic, maps, None, None, -1, maps.double().cpu(), f"critic M={M} S={S}")


@pytest.mark.parametrize("M,S", [(8, 1), (8, 67), (9, 3), (34, 3), (34, 67), (35, 1), (35, 67), (256, 1), (256, 3)])
def test_sized_trunk_at_the_ends_of_its_range_matches_float64(M, S):
    """test_sized_trunk_matches_float64 at the ends of the accepted sides (8: one 4 x 4 tile, 9: the odd row / column dropped by the
    pool; 256: 8 x 8 tiles of 16) and at M = 34 / 35, where P = 17 = 16 + 1: the second tile column and row are one pooled cell wide
    and their halo lies mostly outside the map.  At 256, S <= 3 keeps the float64 CPU reference within seconds."""
    test_sized_trunk_matches_float64(M, S)


def test_sized_trunk_on_walls_off_maps():
    """K5's own maps at 147 x 147: a walls-off env with 2 owners and obstacles after 30 lock-steps (detectors leave the search area)."""
    import numpy as np
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import HeatMaps, actor_stack_from
    N, A, L = 48, 2, 120
    env = RadSearchVec(N, number_agents=A, obstruction_count=3, enforce_grid_boundaries=False, seed=SEED)
    hm = HeatMaps(env, steps_per_episode=L, enforce_boundaries=False)
    assert hm.map_dimensions == (147, 147)
    obs = env.reset()[0]
    rng = np.random.default_rng(5)
    for t in range(30):
        pred = torch.rand(N, A, 2, generator=torch.Generator().manual_seed(t)).cuda() * 1.2
        hm.update(obs, pred)
        acts = rng.integers(0, 9, size=(N, A)).astype(np.int8)
        acts[: N // 2, 0] = 0                                   # half the owners walk out of the search area
        obs = env.step(torch.from_numpy(acts).cuda())[0]
    hm.update(obs)
    maps = hm.shared_maps().clone()
    cells, pcells = hm.field("cell").long().contiguous(), hm.field("pred_cell").long().contiguous()
    assert float(maps[:, 3].abs().sum()) > 0                    # obstacles are on the maps
    actor, critic = _modules(147, seed=3)
    for a in range(A):
        _check_trunk(actor.actor, maps, cells, pcells, a, actor_stack_from(maps, cells, pcells, a).double().cpu(), f"K5 maps a={a}")
    _check_trunk(critic.critic, maps, None, None, -1, maps.double().cpu(), "K5 maps critic")


def test_sized_trunk_equals_k9_k10_at_27():
    """At 27 x 27 the tiled kernels and K9 / K10 implement the same contract: a2 and the gradients agree to fp32 summation order."""
    from radiation_ppo_amd.maps import ConvTrunk, SizedConvTrunk
    S, A = 193, 3
    actor, critic = _modules(27, seed=27)
    maps, cells, pcells = _random_inputs(S, A, 27, seed=27)
    for seq, c, pc, agent in ((actor.actor, cells, pcells, 1), (critic.critic, None, None, -1)):
        conv = [seq[0].weight, seq[0].bias, seq[3].weight, seq[3].bias]
        out = []
        for fn in (ConvTrunk, SizedConvTrunk):
            for p in conv:
                p.grad = None
            a2 = fn.apply(maps, c, pc, agent, *conv, True)
            (a2 * torch.linspace(-1, 1, a2.shape[1], device="cuda")).sum().backward()
            out.append([a2.detach()] + [p.grad.clone() for p in conv])
        for k, x, y in zip(("a2", "dW1", "db1", "dW2", "db2"), *out):
            _close(x, y.double().cpu(), f"agent={agent} {k}", noise=1e-4)


def test_sized_backward_is_deterministic():
    """No float atomics: two backward calls on the same inputs write identical slabs."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    S, A, M = 300, 2, 147
    P = M // 2
    actor, _ = _modules(M, seed=1)
    maps, cells, pcells = _random_inputs(S, A, M, seed=1)
    seq = actor.actor
    a2 = torch.empty(S, 16 * P * P, device="cuda")
    p1 = torch.empty(S, P * P, 8, device="cuda")
    amax = torch.empty(S, P * P, 8, dtype=torch.uint8, device="cuda")
    mask = torch.empty(S, P * P, dtype=torch.int16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rs_cnn_sized_forward(maps.data_ptr(), cells.data_ptr(), pcells.data_ptr(), A, 1, S, M, seq[0].weight.data_ptr(),
                                        seq[0].bias.data_ptr(), seq[3].weight.data_ptr(), seq[3].bias.data_ptr(), a2.data_ptr(),
                                        p1.data_ptr(), amax.data_ptr(), mask.data_ptr(), st))
    da2 = torch.randn_like(a2)
    rows = lib.rs_cnn_sized_slab_rows(S, M, 6)
    assert rows > 1
    slabs = []
    for _ in range(2):
        slab = torch.full((rows, lib.rs_cnn_sized_slab_row(6)), float("nan"), device="cuda")
        _lib.check(lib.rs_cnn_sized_backward(maps.data_ptr(), cells.data_ptr(), pcells.data_ptr(), A, 1, S, M, seq[3].weight.data_ptr(),
                                             da2.data_ptr(), mask.data_ptr(), p1.data_ptr(), amax.data_ptr(), slab.data_ptr(), rows, st))
        slabs.append(slab)
    assert torch.isfinite(slabs[0]).all() and torch.equal(slabs[0], slabs[1])
    # the inference entry point writes the training forward's a2
    a2i = torch.empty_like(a2)
    _lib.check(lib.rs_cnn_sized_infer(maps.data_ptr(), cells.data_ptr(), pcells.data_ptr(), A, 1, S, M, seq[0].weight.data_ptr(),
                                      seq[0].bias.data_ptr(), seq[3].weight.data_ptr(), seq[3].bias.data_ptr(), a2i.data_ptr(), st))
    assert torch.equal(a2i, a2)
    # a slab with fewer rows than workgroups is refused at the entry
    assert lib.rs_cnn_sized_backward(maps.data_ptr(), cells.data_ptr(), pcells.data_ptr(), A, 1, S, M, seq[3].weight.data_ptr(),
                                     da2.data_ptr(), mask.data_ptr(), p1.data_ptr(), amax.data_ptr(), slabs[0].data_ptr(), rows - 1, st) == 1


def _walls_off_collector(N, A, T, L, heads=True, team=True, seed=8):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic, heat_map_geometry
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    torch.manual_seed(seed)
    env = RadSearchVec(N, number_agents=A, obstruction_count=2, enforce_grid_boundaries=False, seed=SEED, env_id_base=32)
    dims = heat_map_geometry(env, L, False)[2]
    gc = CNNCritic(map_dim=dims).cuda() if team else None
    agents = {i: CNNAgentPPO(id=i, map_dim=dims, GlobalCritic=gc, steps_per_epoch=T, steps_per_episode=L, train_pi_iters=2,
                             train_v_iters=2, GlobalCriticOptimizer=torch.optim.Adam(gc.parameters(), lr=1e-3) if team else None)
              for i in range(A)}
    with torch.no_grad():
        for ag in agents.values():
            for p in list(ag.pi.actor[6:].parameters()):
                p.mul_(3.0)                                   # visibly non-uniform policies
    col = CNNCollector(env, agents, T, L, global_critic_flag=team, use_graph=False)
    col.heads = heads
    return col, agents


def test_walls_off_path_never_builds_the_dense_stack(monkeypatch):
    """At 31 x 31 (4-step episodes without walls) the actor / critic, one collect() and one update run without the dense stack and
    without a library convolution."""
    from radiation_ppo_amd import maps as maps_mod
    col, agents = _walls_off_collector(N=16, A=2, T=8, L=4)
    assert col.maps.map_dimensions == (31, 31) and col.use_heads

    def refuse(*a, **k):
        raise AssertionError("dense stack / library convolution on the walls-off path")
    monkeypatch.setattr(maps_mod, "actor_stack_from", refuse)
    monkeypatch.setattr(torch.nn.functional, "conv2d", refuse)
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    m = torch.rand(5, 4, 31, 31, device="cuda", generator=g)
    cells = torch.randint(0, 961, (5, 2), device="cuda", generator=g)
    assert agents[0].pi.logits_from_maps(m, cells, cells, 1).shape == (5, 8)
    assert agents[0].critic.value_from_maps(m).shape == (5,)
    col.collect()
    res = col.update()
    assert all(torch.isfinite(torch.tensor(r.loss_policy)) for r in res.values())


def test_walls_off_update_equals_the_library_path():
    """One update_agent on 31 x 31 maps through the HIP trunk and through the dense stack + library convolutions (the same modules
    called directly), identical inputs and draws: the parameters agree to fp32 tolerance.  Plain SGD in place of Adam, so that the
    comparison measures the gradients (Adam's first step is lr * sign(g): fp32 noise in a near-zero gradient becomes a full step)."""
    from radiation_ppo_amd.maps import actor_stack_from
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO
    M, S, A = 31, 3000, 2
    torch.manual_seed(4)
    ag = CNNAgentPPO(id=0, map_dim=(M, M), train_pi_iters=2, train_v_iters=2, chunk=1024)
    maps, cells, pcells = _random_inputs(S, A, M, seed=4)
    g = torch.Generator(device="cuda"); g.manual_seed(9)
    act = torch.randint(0, 8, (S,), device="cuda", generator=g)
    adv = torch.randn(S, device="cuda", generator=g)
    ret = torch.randn(S, device="cuda", generator=g)
    w = torch.full((S,), 1.0 / S, device="cuda")
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        logp_old = torch.log_softmax(ag.pi.logits(actor_stack_from(maps, cells, pcells, 0)), -1).gather(-1, act.unsqueeze(-1)).squeeze(-1)
    twin = copy.deepcopy(ag)
    params = []
    for a, dense in ((ag, False), (twin, True)):
        a.pi_optimizer = torch.optim.SGD(a.pi.parameters(), lr=0.05)
        a.critic_optimizer = torch.optim.SGD(a.critic.parameters(), lr=0.05)
        if dense:
            actor_in = lambda lo, hi: actor_stack_from(maps[lo:hi], cells[lo:hi], pcells[lo:hi], 0)
            critic_in = lambda lo, hi: maps[lo:hi]
        else:
            actor_in = lambda lo, hi: (maps[lo:hi], cells[lo:hi], pcells[lo:hi], 0)
            critic_in = lambda lo, hi: (maps[lo:hi],)
        with torch.backends.cudnn.flags(enabled=False):         # the native library convolution, no MIOpen solver search
            r = a.update_agent(actor_in, critic_in, act, adv, ret, logp_old, w, update_critic=True)
        assert r.stop_iteration == 2
        params.append([p.detach().clone() for p in list(a.pi.parameters()) + list(a.critic.parameters())])
    for x, y in zip(*params):
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-6), float((x - y).abs().max())


def test_walls_off_fused_select_action_round_equals_the_module_path():
    """rs_cnn_sized_infer + BLAS Linear(16 P P, 32) + rs_cnn_head + rs_store_rows against the module path (heads off) on walls-off maps
    (31 x 31): on the first lock-step, log-probabilities and values agree to float32 summation order; after the epoch every stored row
    of the fused collector equals the library modules (dense stack, nn.Sequential) evaluated on the stored maps."""
    from radiation_ppo_amd.maps import actor_stack_from
    N, A, T, L = 64, 3, 12, 4
    cf, af = _walls_off_collector(N, A, T, L, heads=True)
    cf.collect()
    cm, _ = _walls_off_collector(N, A, T, L, heads=False)
    assert cf.use_heads and not cm.use_heads and cf.maps.map_dimensions == (31, 31)
    cm.collect()
    same = cf.buf.act[0] == cm.buf.act[0]
    assert float(same.float().mean()) > 0.99
    assert torch.allclose(cf.buf.logp[0][same], cm.buf.logp[0][same], rtol=1e-4, atol=2e-5)
    assert torch.allclose(cf.buf.val[0], cm.buf.val[0], rtol=1e-4, atol=2e-5)
    assert torch.equal(cf.buf.obs[0], cm.buf.obs[0]) and torch.equal(cf.shared[0], cm.shared[0])
    assert int(cf.buf.act.min()) >= 0 and int(cf.buf.act.max()) <= 7
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        for t in range(T):
            for a, ag in af.items():
                logits = ag.pi.logits(actor_stack_from(cf.shared[t], cf.cells[t], cf.pcells[t], a))
                lp = torch.log_softmax(logits, dim=-1).gather(-1, cf.buf.act[t, :, a].unsqueeze(-1)).squeeze(-1)
                assert torch.allclose(cf.buf.logp[t, :, a], lp, rtol=1e-4, atol=2e-5), (t, a)
                v = ag.critic(cf.shared[t])
                assert torch.allclose(cf.buf.val[t, :, a], v, rtol=1e-4, atol=2e-5), (t, a)
    boot = cf.buf.last_val != 0
    assert int(boot.sum()) > 0 and bool((cf.buf.cut[boot.any(dim=2)] == 1).all())
