"""rs_ff_team_step through the C ABI against the float64 twin of every agent's own network (tests/_f64_ref.py).

Cases (N, A): (1, 2), (63, 1), (65, 3), (64, 4), (130, 8) -- the edges of a 64-sample wave (one env, one short of a group, exactly one,
one into a second, two groups and two envs) and of the agent count (1, 2, RS_MAX_AGENTS).  Every agent has its OWN weights
(R.ff_agent("x3", seed=a)) and its own rows of x and u: a kernel that reads another agent's network, rows or uniforms fails.

Nothing new is fixed here.  Values: R.close at R.fwd_tolerance("x3")'s output constants; actions and log-probabilities: R.check_draw
(the 1e-5 CDF-edge rule, at most two differing draws per case, logp at rtol 1e-5 / 5e-6) -- the constants rs_policy_forward and K14 are
held to, inside which float32 torch stays (tests/test_f64_references.py).  The worst ratios are printed; profiles/
ff_team_float64_ratios.txt keeps a copy."""
import copy
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(1, 2), (63, 1), (65, 3), (64, 4), (130, 8)]
SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def _case(N, A):
    """Inputs and float64 references of a case, computed once and left unchanged."""
    g = torch.Generator().manual_seed(100 * N + A)
    x = torch.randn(N, A, 11, generator=g)
    u = torch.rand(N, A, generator=g)
    agents = [R.ff_agent("x3", seed=a) for a in range(A)]
    ref = []
    for a, ac in enumerate(agents):
        lg64, v64 = R.ff_forward_f64(R.f64(ac), x[:, a])
        act64, lp64, cdf64 = R.draw_f64(lg64, u[:, a])
        ref.append((v64, act64, lp64, cdf64))
    mask = R.bootstrap_mask(N, g)                                   # past 128 envs: one whole 64-group without a masked env
    return x, u, agents, ref, mask


def _call(agents_gpu, x, u, act, f, act8, mask):
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.ppo import mlp_params
    lib = _lib.load()
    A, N = len(agents_gpu), x.shape[0]
    arr = _lib.RsMlpParams * A
    pa, pc = arr(*[mlp_params(ac.actor) for ac in agents_gpu]), arr(*[mlp_params(ac.critic) for ac in agents_gpu])
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.rs_ff_team_step(pa, pc, A, p(x), p(u), p(act), p(f), p(act8), p(mask), N,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rs_ff_team_step")
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,A", CASES, ids=[f"N{n}-A{a}" for n, a in CASES])
def test_step_round_matches_float64(N, A):
    x, u, agents, ref, _ = _case(N, A)
    gpu = [copy.deepcopy(ac).cuda() for ac in agents]
    xg, ug = x.cuda(), u.cuda()
    act = torch.full((A, N), -1, dtype=torch.int64, device="cuda")
    f = torch.full((A, 3, N), SENTINEL, device="cuda")
    act8 = torch.full((N, A), -1, dtype=torch.int8, device="cuda")
    _call(gpu, xg, ug, act, f, act8, None)
    t_out, _ = R.fwd_tolerance("x3")
    worst_v = worst_lp = 0.0
    differ = 0
    for a in range(A):
        v64, act64, lp64, cdf64 = ref[a]
        same = act[a].cpu() == act64
        differ += int((~same).sum())
        worst_v = max(worst_v, R.close_ratio(f[a, 1], v64, **t_out))
        worst_lp = max(worst_lp, R.close_ratio(f[a, 0].cpu()[same], lp64.gather(-1, act64.unsqueeze(-1)).squeeze(-1)[same],
                                               rtol=1e-5, noise=0.0, tiny=5e-6))
    print(f"rs_ff_team_step step round N{N} A{A} | value {worst_v:.4f} logp {worst_lp:.4f} draws differing {differ}")
    for a in range(A):
        v64, act64, lp64, cdf64 = ref[a]
        R.close(f[a, 1], v64, f"value N{N} A{A} agent {a}", **t_out)
        R.check_draw(act[a], f[a, 0], act64, lp64, cdf64, u[:, a], f"N{N} A{A} agent {a}")
    assert bool((act >= 0).all()) and bool((act <= 7).all())
    assert torch.equal(act8.long(), act.t())                       # act8[n][a] == act[a][n]
    sent = torch.full((A, N), SENTINEL, device="cuda")
    assert torch.equal(f[:, 2].view(torch.int32), sent.view(torch.int32))      # the step round leaves the bootstrap slot alone


@pytest.mark.parametrize("N,A", CASES, ids=[f"N{n}-A{a}" for n, a in CASES])
def test_bootstrap_round_writes_the_masked_values_only(N, A):
    x, _, agents, ref, mask = _case(N, A)
    gpu = [copy.deepcopy(ac).cuda() for ac in agents]
    xg, mg = x.cuda(), mask.cuda()
    f = torch.full((A, 3, N), SENTINEL, device="cuda")
    _call(gpu, xg, None, None, f, None, mg)                         # act = act8 = NULL is accepted
    t_out, _ = R.fwd_tolerance("x3")
    m = mask.bool()
    sent = torch.full((N,), SENTINEL).view(torch.int32)
    worst = 0.0
    for a in range(A):
        got = f[a].cpu()
        worst = max(worst, R.close_ratio(got[2][m], ref[a][0][m], **t_out))
    print(f"rs_ff_team_step bootstrap round N{N} A{A} | value ({int(m.sum())} of {N} masked) {worst:.4f}")
    for a in range(A):
        got = f[a].cpu()
        R.close(got[2][m], ref[a][0][m], f"bootstrap value N{N} A{A} agent {a}", **t_out)
        assert torch.equal(got[2][~m].view(torch.int32), sent[~m]), a              # unmasked envs: untouched, bit for bit
        assert torch.equal(got[0].view(torch.int32), sent) and torch.equal(got[1].view(torch.int32), sent), a
    # mask = NULL: every env
    f2 = torch.full((A, 3, N), SENTINEL, device="cuda")
    _call(gpu, xg, None, None, f2, None, None)
    for a in range(A):
        R.close(f2[a, 2], ref[a][0], f"bootstrap value, no mask N{N} A{A} agent {a}", **t_out)
        assert torch.equal(f2[a, 2].cpu()[m], f[a, 2].cpu()[m])                    # and the same bits as the masked launch
