"""The float64 reference, the cases and the tolerance rule of the RAD-TEAM (CNN) team heads, in its one copy: reference() for the actor
rows of rs_cnn_team_eval_head / rs_cnn_team_step_head and, with k1 at the case's depth (tests/_cnn_sized_team_ref.py: k1()), of their
any-side twins; value_ratios() for the step heads' critic rows; both on first_layer().  The GPU suites reach the kernels through
tests/_cnn_team_drive.py; the CPU self-checks are tests/test_cnn_team_eval_cpu.py and tests/test_cnn_team_drive_cpu.py.  The head behind
the first layer and its rule are tests/_f64_ref.py's (cnn_head_f64, HEAD_K2, HEAD_K3, draw_f64); this module puts a float64 first layer
in front of them.

The rule.  a2 is the trunk's float32 output (an input here: exact, non-negative, sparse), U = 2^-24:
  y1        Linear(2704, 32): a dot product of depth 2704 behind the bias, whatever the order (one fmaf chain, four chains of 676 and
            three adds, a BLAS blocking):  |got - ref| <= FF_RTOL |ref| + K1 U mag1 + FF_TINY,  mag1 = |W1| a2 + |b1|,
            K1 = 2 (sqrt(2705) + 1) = 106: sqrt(n) U of the sum of the absolute terms in expectation, + 1 for the result's own rounding,
            SAFETY 2 -- the line HEAD_K2 / HEAD_K3 are built by, at depth 2704.
  logits    the head's own two chains (HEAD_K2 on carried = |W3| mag2, HEAD_K3 on mag3) plus y1's allowance passed on by the ReLUs
            (slope <= 1) through |W2| and |W3|:  E_lg = FF_RTOL |lg| + U (K1 |W3| |W2| mag1 + HEAD_K2 carried + HEAD_K3 mag3) + FF_TINY
  logp      lp_a = (lg_a - mx) - lse: log-sum-exp moves by at most the largest logit error, so two of them, plus the softmax's own
            rounding, actor_error_model's E_lp line with the lane's own logit spread D_n = max lg - min lg:
            E_lp = FF_RTOL |lp| + 2 max_j E_lg_j + 2 U (9.8 + D_n)
  draws     p_j = exp(lp_j) is off by E_lp relative, so is every CDF value: the action may differ from the float64 draw only on a lane
            whose uniform lies within E_lp x cdf_j of a float64 CDF step j, and on at most DRAW_CAP = 2 lanes per agent and case.  The cap
            is a condition, not a measurement: a draw differs when the float32 CDF's ACTUAL error (a few 1e-6 at these depths) carries a
            step across u, which at N = 130 happens on 7 x 2 x 1e-5 x 130 = 0.02 lanes per agent at most.  (The allowance itself is far
            wider here, ~1e-2: K1 U mag1 is a bound on sums of absolute terms, carried through two more layers of absolute weights.)
  act8      where(alive, act, 8), exactly."""
import copy

import torch

import _f64_ref as R

FLAT = 2704                                      # 16 x 13 x 13: the trunk's output on a 27 x 27 map
K1 = 2.0 * (2705 ** 0.5 + 1)
DRAW_CAP = 2
SIZES = (1, 31, 32, 33, 63, 64, 65, 130)         # a 32-image MFMA tile, the 64-image workgroup and ragged tiles
CASES = [(N, 3) for N in SIZES] + [(64, 8)]
MASTER = 130                                     # every case's lanes are the first N of these
SCALE = 3.0                                      # on the actor's three Linear layers: visibly non-uniform policies (>= 3 actions per agent)


def random_maps(N, A, seed):
    """Heat maps as a run produces them, on the CPU: (maps [N, 4, 27, 27], cells [N, A] int64, pcells [N, A] int64).  Sparse planes,
    z-scored readings of both signs, every owner somewhere; lanes 3 mod 7 are fresh maps (both cells -1), agents 0 and A - 1 share a
    cell on the lanes 5 mod 7."""
    g = torch.Generator().manual_seed(seed)
    maps = torch.rand(N, 4, 27, 27, generator=g) * (torch.rand(N, 4, 27, 27, generator=g) < 0.1)
    maps[:, 1] = maps[:, 1] * 6 - 3
    cells = torch.randint(0, 729, (N, A), generator=g)
    pcells = torch.where(torch.rand(N, A, generator=g) < 0.6, torch.randint(0, 729, (N, A), generator=g), torch.full((N, A), -1))
    lane = torch.arange(N)
    cells[lane % 7 == 5, A - 1] = cells[lane % 7 == 5, 0]
    maps[:, 0] = torch.round(maps[:, 0] * 3)
    maps[:, 0].view(N, 729).scatter_add_(1, cells, torch.ones(N, A))
    fresh = lane % 7 == 3
    cells[fresh], pcells[fresh] = -1, -1
    cells[0, 0] = 0                                                 # a corner: the zero padding
    if N > 2:
        cells[1, 0], cells[2, 0] = 728, 26
    return maps.contiguous(), cells.contiguous(), pcells.contiguous()


class Team:
    pass


_TEAMS = {}


def team(A):
    """A actors (CNNActor, the three Linear layers x SCALE), the master maps and u / alive of MASTER lanes; built once per A on the
    CPU.  alive is mixed with lane 0 alive; a case of N lanes takes the first N and marks lane N - 1 finished (alive_for)."""
    if A in _TEAMS:
        return _TEAMS[A]
    from radiation_ppo_amd.maps import CNNActor
    t = Team()
    t.A, t.M, t.flat, t.N = A, 27, FLAT, MASTER
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7100 + A)
        t.actors = [CNNActor() for _ in range(A)]
    with torch.no_grad():
        for ac in t.actors:
            ac.actor[0].bias.uniform_(-0.05, 0.15)
            ac.actor[3].bias.uniform_(-0.1, 0.1)
            for i in (6, 8, 10):
                for p in ac.actor[i].parameters():
                    p.mul_(SCALE)
    t.maps, t.cells, t.pcells = random_maps(MASTER, A, seed=4200 + A)
    g = torch.Generator().manual_seed(99 + A)
    t.u = torch.rand(MASTER, A, generator=g)
    t.alive = (torch.rand(MASTER, generator=g) < 0.6).to(torch.uint8)
    t.alive[0] = 1
    _TEAMS[A] = t
    return t


def alive_for(t, N):
    al = t.alive[:N].clone()
    al[N - 1] = 0
    if N > 1:
        al[0] = 1
    return al


def trunk_cpu(t):
    """a2 [A, MASTER, 2704] by torch's convolutions on the CPU (the CPU self-check's stand-in for the trunk kernel)."""
    from radiation_ppo_amd.maps import actor_stack_from
    with torch.no_grad():
        return torch.stack([t.actors[a].actor[:6](actor_stack_from(t.maps, t.cells, t.pcells, a)) for a in range(t.A)]).contiguous()


class Ref:
    pass


def first_layer(s64, a2, k1):
    """The float64 first layer of the module s64 on a float32 a2 [N, flat] (widened), and what its error may be and become:
    (y1, mag1, y1_allow, through), through = |W3| |W2| mag1, the factor of k1 U in the allowance of an output of the last layer."""
    x = a2.detach().double().cpu()
    W1, b1, W2, W3 = s64[6].weight, s64[6].bias, s64[8].weight, s64[10].weight
    y1 = x @ W1.t() + b1
    mag1 = x.abs() @ W1.abs().t() + b1.abs()
    y1_allow = R.FF_RTOL * y1.abs() + k1 * R.U * mag1 + R.FF_TINY
    return y1, mag1, y1_allow, (mag1 @ W2.abs().t()) @ W3.abs().t()


def output_allow(out, through, carried, mag3, k1):
    """the allowance of the last layer's outputs (logits, or a critic's value): the module docstring's E_lg"""
    return R.FF_RTOL * out.abs() + R.U * (k1 * through + R.HEAD_K2 * carried + R.HEAD_K3 * mag3) + R.FF_TINY


def reference(seq, a2, u, k1=K1):
    """The float64 policy round of one agent on a float32 a2 [N, flat] (widened) and its uniforms u [N]: y1, logits, the draw, and
    the allowances of the module docstring, the first layer's constant k1 that of a2's depth (K1: 2704)."""
    s64 = R.f64(seq)
    r = Ref()
    with torch.no_grad():
        r.y1, _, r.y1_allow, through = first_layer(s64, a2, k1)
        r.lg, mag3, carried = R.cnn_head_f64(s64, r.y1)
        e_lg = output_allow(r.lg, through, carried, mag3, k1)
        spread = r.lg.amax(dim=1) - r.lg.amin(dim=1)
        r.act, r.lp, r.cdf = R.draw_f64(r.lg, u.cpu())
        r.lp_allow = 2 * e_lg.amax(dim=1) + 2 * R.U * (9.8 + spread)         # + FF_RTOL |lp| where it is applied
    return r


def value_ratios(seq_cpu, a2, got_v, got_y1, k1):
    """A critic row of the step heads under the same lines: (worst |y1 - ref| / allowance, worst |value - ref| / allowance), the one
    output held to the allowance reference() gives a logit."""
    s64 = R.f64(seq_cpu)
    with torch.no_grad():
        y1, _, y1_allow, through = first_layer(s64, a2, k1)
        val, mag3, carried = R.cnn_head_f64(s64, y1)
        allow = output_allow(val, through, carried, mag3, k1)
        gv, gy = got_v.detach().double().cpu().reshape(val.shape), got_y1.detach().double().cpu()
        assert bool(torch.isfinite(gv).all()) and bool(torch.isfinite(gy).all())
        return float(((gy - y1).abs() / y1_allow).max()), float(((gv - val).abs() / allow).max())


def value_passes(q_y1, q_value):
    return q_y1 <= 1.0 and q_value <= 1.0


def ratios(r, u, alive, act, logp, act8, y1=None):
    """The rule as numbers, for one agent: dict(y1, logp: worst error / allowance; differing: lanes whose action is not the float64
    draw; unexcused: those of them whose uniform is NOT within the allowance of a CDF step; act8: entries != where(alive, act, 8))."""
    act, logp, u = act.cpu().long(), logp.detach().double().cpu(), u.double().cpu()
    out = dict(y1=0.0)
    if y1 is not None:
        q = (y1.detach().double().cpu() - r.y1).abs() / r.y1_allow
        out["y1"] = float(torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf"))).max())
    same = act == r.act
    near = ((r.cdf[:, :-1] - u.unsqueeze(-1)).abs() <= r.lp_allow.unsqueeze(-1) * r.cdf[:, :-1]).any(dim=1)
    out["differing"] = int((~same).sum())
    out["unexcused"] = int((~same & ~near).sum())
    ref_lp = r.lp.gather(-1, r.act.unsqueeze(-1)).squeeze(-1)
    q = (logp - ref_lp).abs() / (R.FF_RTOL * ref_lp.abs() + r.lp_allow)
    q = torch.where(torch.isfinite(logp), q, torch.full_like(q, float("inf")))
    out["logp"] = float(q[same].max()) if bool(same.any()) else 0.0
    want8 = torch.where(alive.cpu() != 0, act, torch.full_like(act, 8))
    out["act8"] = int((act8.cpu().long() != want8).sum())
    return out


def passes(q):
    return q["y1"] <= 1.0 and q["logp"] <= 1.0 and q["unexcused"] == 0 and q["differing"] <= DRAW_CAP and q["act8"] == 0


def torch32(seq, a2, u, alive):
    """The float32 torch composition of the round, as the composed runner has it: (y1, act, logp, act8)."""
    with torch.no_grad():
        y1 = torch.nn.functional.linear(a2, seq[6].weight, seq[6].bias)
        lp = torch.log_softmax(seq[7:11](y1), dim=-1)
        cdf = torch.cumsum(lp.exp(), dim=-1)
        act = (cdf[:, :-1] <= u.unsqueeze(-1)).sum(dim=-1)
        logp = lp.gather(-1, act.unsqueeze(-1)).squeeze(-1)
        return y1, act, logp, torch.where(alive != 0, act, torch.full_like(act, 8)).to(torch.int8)


def distinct_actions(r):
    return int(torch.unique(r.act).numel())


def clone_seq(seq, device):
    return copy.deepcopy(seq).to(device)
