"""The small RAD-TEAM kernels behind the 27 x 27 trunk against float64 at their wave, block and stride edges: rs_actor_loss (through
ppo_cnn.ActorLoss), rs_cnn_head (OUT = 8 and OUT = 1, through the C ABI with the collector's arguments) and the collector's split of
the trunk, rs_cnn_trunk_prepare + rs_cnn_trunk_infer.  References, cases and the rule are in tests/_f64_ref.py (its CPU self-checks,
the float32 torch path under the same rule and the mutations the rule must see: test_f64_references.py).

rs_actor_loss runs one sample per lane in blocks of 256, writes one row of stats per 64-lane wave whose lane 0 is live and clamps dead
lanes to the last sample with w = 0.  Sizes (R.AL_SIZES): 1, 63, 64, 65 (one wave short, full, one sample into a second), 255, 256, 257
(the same at the block) and 577 = 2 x 256 + 64 + 1; clip 0.2 and 0.1.  Half of the weight lies on the last wave (R.wave_weights), so a
lost or mis-indexed last wave is wrong by tens of percent (proved on the CPU at >= 100 x the allowance).

The rule, per element of dlogits and per statistic:  |got - ref| <= R.FF_RTOL |ref| + k U mag + R.FF_TINY,  U = 2^-24, mag the sum of the
absolute per-sample terms (R.actor_loss_f64).  The constants are R.actor_error_model's, the lines of R.ff_error_model behind the logits
(units of U, SAFETY = 2 on everything):
  softmax     eight expf, their sum, one logf, two subtractions: E_lp = 2 E_out + 9.8 with E_out = 0, the logits being inputs;  plus the
              rounding of lg_j - mx, 0.5 ulp of up to the largest logit spread D of the cases (randn x 1.5 over eight logits: D = 9.51,
              R.al_spread; the feed-forward cases keep it near 1 and count it as 1): E_lp = 9.8 + D = 19.3
  p_j         expf(lp_j): E_p = E_lp + 21 (argument scaling at lp ~ -20)                                       = 40.3
  ratio       expf(logp - lpo): E_lp + 3;  g_lp = -w (adv ratio): two products: E_glp = E_lp + 5                = 24.3
  dlogits     d_j = g_lp (1[a = j] - p_j): E_dz = E_glp + E_p + 1 = 65.6 -> k_dl = 131 (k U = 7.8e-6) on |g_lp| (1[a = j] + p_j)
  statistics  the same per-sample term (kl: logp's E_lp on |lpo| + |logp|; entropy: p_j's and lp_j's on p_j (1 + |lp_j|); loss: the
              ratio's on |surr| (1 + |logp|)) plus the 64-lane butterfly, depth 6, one rounding of the partial sum per level:
              k_stat = 2 (65.6 + 6) = 143 (8.5e-6).  The host adds the rows of stats in float64: nothing.
Float32 torch on the CPU sits at <= 0.13 of the dlogits bound and <= 0.015 of the statistics', rs_actor_loss at <= 0.13 and <= 0.012.

rs_cnn_head: ReLU -> Linear(32, 16) -> ReLU -> Linear(16, OUT) as two sequential fmaf chains behind the bias, depth 32 and depth 16:
  h2          (sqrt(33) + 1) U mag2, mag2 = |W2| relu(y1) + |b2|, passed on by the ReLU (slope <= 1) and carried through |W3|
  output      (sqrt(17) + 1) U mag3, mag3 = |W3| h2 + |b3|
so |got - ref| <= R.FF_RTOL |ref| + U (R.HEAD_K2 |W3| mag2 + R.HEAD_K3 mag3) + R.FF_TINY with HEAD_K2 = 2 (sqrt(33) + 1) = 13.5 and HEAD_K3 =
2 (sqrt(17) + 1) = 10.2 (R.head_ratio); the values of OUT = 1 are held to it.  OUT = 8 hands out no logits: actions and log-probabilities
are held to R.check_draw against R.draw_f64 of the float64 head (a differing draw only within 1e-5 of a CDF step, at most two per
agent; logp at rtol 1e-5 / 5e-6), the constants of every collector kernel here, inside which float32 torch stays.

rs_cnn_trunk_infer launches the kernel of rs_cnn_trunk_forward's no-grad form, which test_cnn_trunk_gpu.py holds to float64: equal bits.

Every worst ratio is printed; profiles/cnn_heads_float64_ratios.txt keeps a copy."""
import copy
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678
from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG  # noqa: E402
TRUNK_SIZES = (1, 2, 3, 4, 64, 65, 193)            # three images make one workgroup round


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, device="cuda")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _actor_loss(batch, clip):
    """ActorLoss on a batch (tensors on any device, moved to the GPU): (stats [4] float64, dlogits [S, 8]) on the CPU."""
    from radiation_ppo_amd.ppo_cnn import ActorLoss
    logits, act, adv, lpo, w = (t.cuda() for t in batch)
    lg = logits.clone().requires_grad_(True)
    loss, st = ActorLoss.apply(lg, act, adv, lpo, w, clip)
    loss.backward()
    assert st.dtype == torch.float64 and float(loss.detach()) == float(st[3].float())
    return st.cpu(), lg.grad.cpu()


# ------------------------------------------------------------------------------------------------ rs_actor_loss
@pytest.mark.parametrize("case", R.AL_CASES, ids=R.al_case_id)
def test_actor_loss_matches_float64(case):
    c = R.al_case(*case)
    st, dl = _actor_loss(c.batch, c.clip)
    rep = []
    try:
        R.check_actor(st, dl, c.ref, "rs_actor_loss " + R.al_case_id(case), report=rep)
    finally:
        print(rep[0])


def test_actor_loss_chunks_add_up():
    """S = 257 as chunks of 100, 100 and 57 (update_agent's ragged chunks): a sample's derivative does not depend on its position, so
    the concatenated dlogits equal the one launch's bit for bit; the summed statistics stay under the rule."""
    c = R.al_case(257, 0.2)
    st, dl = _actor_loss(c.batch, c.clip)
    parts = [_actor_loss(tuple(t[lo:hi] for t in c.batch), c.clip) for lo, hi in ((0, 100), (100, 200), (200, 257))]
    assert torch.equal(_bits(torch.cat([d for _, d in parts])), _bits(dl))
    rep = []
    try:
        R.check_actor(torch.stack([s for s, _ in parts]).sum(dim=0), dl, c.ref, "rs_actor_loss S257 in chunks of 100, 100, 57", report=rep)
    finally:
        print(rep[0])


def test_actor_loss_takes_strided_columns():
    """The inputs as column a of [S, 3, 8] / [S, 3] tensors (a column of the collector's [T, N, A] buffers): the same bits as the dense
    copies, and no gradient in the other columns."""
    from radiation_ppo_amd.ppo_cnn import ActorLoss
    c = R.al_case(257, 0.2)
    st, dl = _actor_loss(c.batch, c.clip)
    g = torch.Generator().manual_seed(3)
    a = 1

    def wide(t, fill):
        big = fill((t.shape[0], 3) + tuple(t.shape[1:]))
        big[:, a] = t
        return big.cuda()
    logits3 = wide(c.logits, lambda s: torch.randn(s, generator=g)).requires_grad_(True)
    act3 = wide(c.act, lambda s: torch.randint(0, 8, s, generator=g))
    adv3, lpo3, w3 = (wide(t, lambda s: torch.randn(s, generator=g)) for t in (c.adv, c.lpo, c.w))
    col = logits3[:, a]
    assert not col.is_contiguous() and not act3[:, a].is_contiguous()
    loss, st3 = ActorLoss.apply(col, act3[:, a], adv3[:, a], lpo3[:, a], w3[:, a], c.clip)
    loss.backward()
    assert torch.equal(st3.cpu().view(torch.int64), st.view(torch.int64))
    assert torch.equal(_bits(logits3.grad[:, a]), _bits(dl))
    assert not bool(logits3.grad[:, 0].any()) and not bool(logits3.grad[:, 2].any())


def test_actor_loss_zero_weight_rows_contribute_nothing():
    """S = 257 with w = 0 and adv x 1e6 (finite) on 40 scattered rows, as a minibatch draw leaves most rows: their rows of dlogits are
    all zero, and statistics and the other rows match the reference computed with those rows deleted."""
    S, clip, rows = R.AL_ZERO
    c = R.al_case(S, clip, zero_rows=rows)
    assert int((c.w == 0).sum()) == rows
    st, dl = _actor_loss(c.batch, c.clip)
    assert not bool(dl[~c.keep].any())
    rep = []
    try:
        R.check_actor(st, dl[c.keep], c.ref, f"rs_actor_loss S{S}-clip{clip:g}-{rows}-zero-rows", report=rep)
    finally:
        print(rep[0])


# ------------------------------------------------------------------------------------------------ rs_cnn_head
def _head(seq, y1, out_dim, N, u=None, us=1, act=None, logp=None, act8=None, a8s=1, value=None, copies=1, vstride=0, mask=None):
    """rs_cnn_head with layers [8] and [10] of seq; pointers are data_ptr() integers or None.  Returns the status code."""
    from radiation_ppo_amd import _lib
    return _lib.load().rs_cnn_head(y1, seq[8].weight.data_ptr(), seq[8].bias.data_ptr(), seq[10].weight.data_ptr(), seq[10].bias.data_ptr(),
                                   out_dim, u, us, act, logp, act8, a8s, value, copies, vstride, mask, N, _stream())


def _ok(code):
    from radiation_ppo_amd import _lib
    _lib.check(code, "rs_cnn_head")
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", R.HEAD_SIZES)
def test_head_actions_and_log_probabilities_match_float64(N):
    """OUT = 8, once per agent with the collector's arguments (u + 4 a and act8 + a at stride A, act = _k_act[a], logp = _k_f[a, 0]):
    every agent has its own layers, y1 and column of u, so a wrong base or stride draws another agent's action."""
    c = R.head_case(N)
    A = c.A
    seqs = [copy.deepcopy(ac.actor).cuda() for ac in c.actors]
    y1, u = c.y1a.cuda(), c.u.cuda()
    k_act = torch.full((A, N), -1, dtype=torch.int64, device="cuda")
    k_f = _sentinel(A, 3, N)
    act8 = torch.full((N, A), -1, dtype=torch.int8, device="cuda")
    for a in range(A):
        before = (k_act.clone(), k_f.clone(), act8.clone())
        _ok(_head(seqs[a], y1[a].data_ptr(), 8, N, u=u.data_ptr() + 4 * a, us=A, act=k_act[a].data_ptr(), logp=k_f[a, 0].data_ptr(),
                  act8=act8.data_ptr() + a, a8s=A))
        for b in range(A):
            if b != a:                                              # the other agents' rows and columns: as they were, bit for bit
                assert torch.equal(k_act[b], before[0][b]) and torch.equal(_bits(k_f[b]), _bits(before[1][b])), (a, b)
                assert torch.equal(act8[:, b], before[2][:, b]), (a, b)
        assert torch.equal(_bits(k_f[:, 1:]), _bits(_sentinel(A, 2, N))), a
    worst = dict(edge=0.0, logp=0.0)
    differ = 0
    for a in range(A):
        e, lp, d = R.draw_ratios(k_act[a], k_f[a, 0], *c.actor_ref[a][3:], c.u[:, a])
        worst["edge"], worst["logp"], differ = max(worst["edge"], e), max(worst["logp"], lp), differ + d
    print(f"rs_cnn_head OUT8 N{N} A{A} | " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()) + f" draws differing {differ}")
    for a in range(A):
        R.check_draw(k_act[a], k_f[a, 0], *c.actor_ref[a][3:], c.u[:, a], f"N{N} agent {a}")
    assert bool((k_act >= 0).all()) and bool((k_act <= 7).all())
    assert torch.equal(act8.long(), k_act.t())                      # act8[n][a] == act[a][n]
    # act = logp = NULL: act8 only
    only8 = torch.full((N, A), -1, dtype=torch.int8, device="cuda")
    _ok(_head(seqs[1], y1[1].data_ptr(), 8, N, u=u.data_ptr() + 4, us=A, act8=only8.data_ptr() + 1, a8s=A))
    assert torch.equal(only8[:, 1].long(), k_act[1]) and bool((only8[:, 0] == -1).all()) and bool((only8[:, 2] == -1).all())


@pytest.mark.parametrize("N", R.HEAD_SIZES)
def test_head_values_match_float64_in_both_layouts_and_under_a_mask(N):
    """OUT = 1.  One critic per agent (copies = 1, written at _k_f[a, slot]) and a global critic (copies = A at value_stride = 3 N from
    _k_f[0, slot]: bit-identical copies); with the bootstrap mask the masked envs get the bits of the unmasked launch and the others
    keep the sentinel (N = 130: envs 64..127 are one whole wave without a masked env, and the last env is set)."""
    c = R.head_case(N)
    A = c.A
    seqs = [copy.deepcopy(cr.critic).cuda() for cr in c.critics]
    y1 = c.y1c.cuda()
    mask = c.mask.cuda()
    m = c.mask.bool()
    assert bool(m[0]) and (N <= 128 or (bool(m[N - 1]) and not bool(m[64:128].any())))
    sent = _bits(_sentinel(A, N))
    worst = {}
    # one critic per agent, the step's slot
    own, own_m = _sentinel(A, 3, N), _sentinel(A, 3, N)
    for a in range(A):
        _ok(_head(seqs[a], y1[a].data_ptr(), 1, N, value=own[a, 1].data_ptr(), copies=1, vstride=3 * N))
        _ok(_head(seqs[a], y1[a].data_ptr(), 1, N, value=own_m[a, 1].data_ptr(), copies=1, vstride=3 * N, mask=mask.data_ptr()))
    worst["own critics"] = max(R.head_ratio(own[a, 1], *c.critic_ref[a]) for a in range(A))
    for k_f in (own, own_m):
        assert torch.equal(_bits(k_f[:, 0]), sent) and torch.equal(_bits(k_f[:, 2]), sent)
    # a global critic (agent 0's network and rows), the bootstrap slot
    glob, glob_m = _sentinel(A, 3, N), _sentinel(A, 3, N)
    _ok(_head(seqs[0], y1[0].data_ptr(), 1, N, value=glob[0, 2].data_ptr(), copies=A, vstride=3 * N))
    _ok(_head(seqs[0], y1[0].data_ptr(), 1, N, value=glob_m[0, 2].data_ptr(), copies=A, vstride=3 * N, mask=mask.data_ptr()))
    worst["global critic"] = max(R.head_ratio(glob[k, 2], *c.critic_ref[0]) for k in range(A))
    for k_f in (glob, glob_m):
        assert torch.equal(_bits(k_f[:, 0]), sent) and torch.equal(_bits(k_f[:, 1]), sent)
        for k in range(1, A):
            assert torch.equal(_bits(k_f[k, 2]), _bits(k_f[0, 2])), k                  # bit-identical copies
    print(f"rs_cnn_head OUT1 N{N} A{A} | " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()) + f" ({int(m.sum())} of {N} masked)")
    assert all(v <= 1.0 for v in worst.values()), worst
    for full, part, slot in ((own, own_m, 1), (glob, glob_m, 2)):
        f, p = _bits(full[:, slot]), _bits(part[:, slot])
        assert torch.equal(p[:, m], f[:, m])                        # masked envs: the unmasked launch's bits
        assert torch.equal(p[:, ~m], sent[:, ~m])                   # unmasked envs: untouched


def test_head_and_actor_loss_reject_bad_arguments():
    """RS_ERR_INVALID_ARG before anything is launched (the outputs keep their sentinel): out_dim = 3, num_envs = 0, u = NULL at out_dim =
    8, value = NULL at out_dim = 1; samples = 0 for rs_actor_loss."""
    from radiation_ppo_amd import _lib
    c = R.head_case(65)
    N, A = c.N, c.A
    seq, crit = copy.deepcopy(c.actors[0].actor).cuda(), copy.deepcopy(c.critics[0].critic).cuda()
    y1, u = c.y1a[0].cuda(), c.u.cuda()
    act = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    logp, value = _sentinel(N), _sentinel(N)
    act8 = torch.full((N, A), -1, dtype=torch.int8, device="cuda")
    step = dict(u=u.data_ptr(), us=A, act=act.data_ptr(), logp=logp.data_ptr(), act8=act8.data_ptr(), a8s=A)
    assert _head(seq, y1.data_ptr(), 3, N, value=value.data_ptr(), **step) == RS_ERR_INVALID_ARG
    assert _head(seq, y1.data_ptr(), 8, 0, **step) == RS_ERR_INVALID_ARG
    assert _head(crit, y1.data_ptr(), 1, 0, value=value.data_ptr()) == RS_ERR_INVALID_ARG
    assert _head(seq, y1.data_ptr(), 8, N, **dict(step, u=None)) == RS_ERR_INVALID_ARG
    assert _head(crit, y1.data_ptr(), 1, N, value=None) == RS_ERR_INVALID_ARG
    k = R.al_case(65, 0.2)
    logits, a, adv, lpo, w = (t.cuda() for t in k.batch)
    dl, stats = _sentinel(65, 8), _sentinel(2, 4)
    code = _lib.load().rs_actor_loss(logits.data_ptr(), a.data_ptr(), adv.data_ptr(), lpo.data_ptr(), w.data_ptr(), dl.data_ptr(),
                                     stats.data_ptr(), 0, 0.2, _stream())
    assert code == RS_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((act == -1).all()) and bool((act8 == -1).all())
    for t in (logp, value, dl, stats):
        assert torch.equal(_bits(t), _bits(torch.full_like(t, SENTINEL)))


# ------------------------------------------------------------------------------------------------ rs_cnn_trunk_prepare + rs_cnn_trunk_infer
@pytest.mark.parametrize("N", TRUNK_SIZES)
def test_trunk_infer_equals_the_no_grad_forward(N):
    """The collector's split of the 27 x 27 trunk for the actor of agents 0 and A - 1 and for the critic (agent = -1, num_agents = 0,
    NULL cells): a2 equals rs_cnn_trunk_forward's no-grad result (ConvTrunk under torch.no_grad(), held to float64 by
    test_cnn_trunk_gpu.py) bit for bit, on two sets of maps from ONE prepare, and the row behind a2[N - 1] keeps its sentinel."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import CNNActor, CNNCritic, ConvTrunk
    from test_cnn_trunk_gpu import _random_inputs
    lib = _lib.load()
    torch.manual_seed(N)
    A = 3
    actor, critic = CNNActor().cuda(), CNNCritic().cuda()
    with torch.no_grad():                                  # make biases matter (pool ties on empty regions, ReLU gates)
        for s in (actor.actor, critic.critic):
            s[0].bias.uniform_(-0.05, 0.15)
            s[3].bias.uniform_(-0.1, 0.1)
    rounds = [_random_inputs(N, A, seed=N), _random_inputs(N, A, seed=N + 1000)]
    assert not torch.equal(rounds[0][0], rounds[1][0])
    sent = _bits(_sentinel(2704))
    for seq, agent in ((actor.actor, 0), (actor.actor, A - 1), (critic.critic, -1)):
        cin = 6 if agent >= 0 else 4
        conv = [t.detach().contiguous() for t in (seq[0].weight, seq[0].bias, seq[3].weight, seq[3].bias)]
        wt = torch.empty(lib.rs_cnn_trunk_scratch_floats(cin), dtype=torch.float32, device="cuda")
        _lib.check(lib.rs_cnn_trunk_prepare(cin, *(t.data_ptr() for t in conv), wt.data_ptr(), _stream()), "rs_cnn_trunk_prepare")
        for maps, cells, pcells in rounds:
            a2 = _sentinel(N + 1, 2704)
            ce, pc = (cells, pcells) if agent >= 0 else (None, None)
            _lib.check(lib.rs_cnn_trunk_infer(maps.data_ptr(), None if ce is None else ce.data_ptr(), None if pc is None else pc.data_ptr(),
                                              A if agent >= 0 else 0, agent, N, wt.data_ptr(), a2.data_ptr(), _stream()), "rs_cnn_trunk_infer")
            torch.cuda.synchronize()
            with torch.no_grad():
                want = ConvTrunk.apply(maps, ce, pc, agent, *conv, False)
            assert float(want.abs().max()) > 0 and bool(torch.isfinite(want).all())
            assert torch.equal(_bits(a2[:N]), _bits(want)), (agent, N)
            assert torch.equal(_bits(a2[N]), sent), (agent, N)
