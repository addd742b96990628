"""What the two GPU suites of the RAD-A2C evaluation share (tests/test_rnn_eval_gpu.py: one agent, through the rs_rnn_eval_* entries
and run_test_environments_rnn; tests/test_rnn_team_eval_gpu.py: teams): the seeded agents and the state of the two bookkeeping kernels
with their torch composition.  (The comparisons of records and of a carried-hidden log against the oracle: tests/_eval_runs.py.)  One
agent is the team of one throughout: [N][1] rows.  torch and the package are imported inside the functions that run on the device."""
import ctypes as C

DEV = "cuda:0"


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _args(hid, pol, val, rec):
    return dict(hidden=((hid,),), hidden_sizes_pol=((pol,),), hidden_sizes_val=((val,),), hidden_sizes_rec=(rec,))


# K11 + K14's arithmetic (rs_rnn_team_eval_step / rs_rnn_policy_step_rows); rs_pfgru_sized_step + rs_rnn_sized_step
WIDTHS = {"default": None, "sized": _args(32, 64, 64, 16)}


def team(A, widths="default", L=30, scale=4.0, seed=9):
    """A agents with their own weights (one torch seed per agent) and decisive policies (policy-head weights x scale, as
    tests/test_evaluate_gpu.py): sources are found within 30 steps sometimes"""
    import torch
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    out = {}
    for a in range(A):
        torch.manual_seed(seed + 101 * a)
        out[a] = RNNAgentPPO(id=a, steps_per_episode=L, actor_critic_args=WIDTHS[widths])
        with torch.no_grad():
            for p in out[a].agent.pi.parameters():
                p.mul_(scale)
    return out


def agent(widths="default", L=30, scale=4.0, seed=9):
    return team(1, widths, L, scale, seed)[0]


class Lanes:
    """The state rs_rnn_team_eval_state points at, [N][A] rows; with A = 1 also what rs_rnn_eval_state points at.  impl "hip": the
    kernels' side; "torch": the composition's side (same dtypes)."""

    def __init__(self, N, A, Rl, impl):
        import torch
        from radiation_ppo_amd.ppo import DeviceWelford
        n = torch.arange(N, device=DEV)
        self.N, self.A, self.Rl = N, A, Rl
        self.stat = DeviceWelford((N, A), DEV, impl=impl)
        started = (n % 3 != 1).view(N, 1).expand(N, A)              # lanes with n % 3 == 1 enter with Welford count 0
        first = torch.floor(torch.rand(N, A, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) * 900.0).double()
        self.stat.count.copy_(started.double())
        self.stat.mean.copy_(torch.where(started, first, torch.zeros_like(first)))
        self.done_before = n % 5 == 3                               # lanes that enter with every run behind them
        self.late = (n % 7 == 5) & ~self.done_before                # lanes the caller starts late (see the tests' docstrings)
        self.active = (~(self.done_before | self.late)).to(torch.uint8)
        self.again = torch.full((N,), 3, dtype=torch.uint8, device=DEV)      # overwritten on every lane by the first step
        self.run = torch.where(self.done_before, torch.full_like(n, Rl), torch.zeros_like(n)).int()
        self.steps = torch.zeros(N, dtype=torch.int32, device=DEV)
        self.ret = torch.zeros(N, dtype=torch.float32, device=DEV)
        self.rec_len = torch.full((N, Rl), -5, dtype=torch.int32, device=DEV)
        self.rec_ret = torch.full((N, Rl), -7.5, dtype=torch.float32, device=DEV)
        self.rec_suc = torch.full((N, Rl), 9, dtype=torch.uint8, device=DEV)
        self.calls = (n * 3).long()
        self.idle = ((n.view(N, 1) + torch.arange(A, device=DEV).view(1, A)) % 8).to(torch.int8).contiguous()
        self.finished = torch.tensor([int(self.done_before.sum())], dtype=torch.int32, device=DEV)   # monotonic from the caller's start value
        self.cur = torch.full((N, A, 11), -1.0, device=DEV)
        self.x = torch.full((N, A, 11), -2.0, device=DEV)

    def arrays(self):
        return dict(active=self.active, again=self.again, run=self.run, steps=self.steps, ret=self.ret, rec_len=self.rec_len,
                    rec_ret=self.rec_ret, rec_suc=self.rec_suc, pf_calls=self.calls, idle_act8=self.idle, finished=self.finished,
                    cur_obs=self.cur, x=self.x, count=self.stat.count, mean=self.stat.mean, sq=self.stat.sq, std=self.stat.std)

    def struct(self, L, env_obs, env_rew, env_done, optional=True, single=False):
        """rs_rnn_team_eval_state; single: rs_rnn_eval_state, the same fields without A"""
        from radiation_ppo_amd import _lib
        p = lambda t: t.data_ptr()
        s = self.stat
        assert self.A == 1 or not single
        cls, dims = (_lib.RsRnnEvalState, (self.N,)) if single else (_lib.RsRnnTeamEvalState, (self.N, self.A))
        return cls(*dims, self.Rl, L, p(env_obs), p(env_rew), p(env_done), p(self.cur), p(self.x), p(s.count), p(s.mean), p(s.sq), p(s.std),
                   p(self.active), p(self.again), p(self.run), p(self.steps), p(self.ret), p(self.rec_len), p(self.rec_ret),
                   p(self.rec_suc), p(self.calls) if optional else None, p(self.idle) if optional else None, p(self.finished))

    # the torch composition, in the order include/radsearch.h lists; obs [N, A, 11], rew and done [N, A] (or [N] with one agent)
    def post_step(self, L, obs, rew, done):
        import torch
        N, Rl = self.N, self.Rl
        a = self.active.bool()
        self.ret.copy_(torch.where(a, self.ret + rew.view(N, self.A)[:, 0], self.ret))
        self.steps += a.int()
        self.calls += a.long()
        found = a & done.view(N, self.A).bool().any(dim=1)
        over = found | (a & (self.steps == L))
        self.stat.update(obs[..., 0], mask=a)
        lane, slot = torch.arange(N, device=DEV), self.run.long().clamp(max=Rl - 1)
        self.rec_len[lane, slot] = torch.where(over, self.steps, self.rec_len[lane, slot])
        self.rec_ret[lane, slot] = torch.where(over, self.ret, self.rec_ret[lane, slot])
        self.rec_suc[lane, slot] = torch.where(over, found.to(torch.uint8), self.rec_suc[lane, slot])
        self.run += over.int()
        self.steps.masked_fill_(over, 0)
        self.ret.masked_fill_(over, 0.0)
        self.again.copy_((over & (self.run < Rl)).to(torch.uint8))
        last = over & (self.run == Rl)
        self.active.masked_fill_(last, 0)
        self.idle.masked_fill_(last.view(N, 1), 8)
        self.finished += last.sum().int()
        self.cur.copy_(obs)
        self.x.copy_(obs)
        self.stat.standardize(obs[..., 0], out=self.x[..., 0])
        return found, over, last

    def post_refresh(self, obs):
        import torch
        m = self.again.bool()
        self.stat.reset(m)
        self.stat.update(obs[..., 0], mask=m)
        z = obs.clone()
        self.stat.standardize(obs[..., 0], out=z[..., 0])
        self.cur.copy_(torch.where(m.view(-1, 1, 1), obs, self.cur))
        self.x.copy_(torch.where(m.view(-1, 1, 1), z, self.x))


def same(k, t, what=""):
    import torch
    for (name, a), b in zip(k.arrays().items(), t.arrays().values()):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, name, (a != b).nonzero()[:6].tolist())
