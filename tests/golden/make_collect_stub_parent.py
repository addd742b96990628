"""Fixture of RNNCollector's lock-step on the CPU over a scripted env: what the torch composition of the bookkeeping (returns, counters,
cut / boot flags, Welford update / reset / restart, observation copies, buffer rows, draw counters) computed at commit d42dfd2 ("C
binding: derive the ctypes signatures and structs from the header"), the commit BEFORE the composition moved into CollectGlue's torch
form.  On the CPU there is no kernel: the policy step is the torch modules, the predictor bank its torch form, the env the stub below,
which draws every row from a seeded torch.Generator (always for all envs, so the stream of draws does not depend on the masks) and logs
what it was given.  The recorder runs on that commit's tree and on every later one; tests/test_collect_stub_parent_cpu.py replays it.

N = 5, A = 2, T = 6, L = 3, two epochs: main() asserts that terminal, timeout and epoch cuts and non-zero bootstrap values occur.

    python tests/golden/make_collect_stub_parent.py [OUT.npz]   # no GPU; on a later tree it must reproduce the committed file
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "collect_stub_parent.npz")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, A, T, L, EPOCHS = 5, 2, 6, 3, 2
BUFFER = ("obs", "act", "rew", "val", "logp", "last_val", "cut", "source_tar")


class StubEnv:
    """What RNNCollector asks of RadSearchVec: fixed-address obs / reward / team / done / oob, state("src_x" / "src_y") [1, N],
    reset(mask), step, action_uniforms, set_epoch_end and cfg.seed / cfg.env_id_base."""

    def __init__(self, seed: int = 77):
        self.num_envs, self.number_agents, self.device = N, A, torch.device("cpu")
        self.cfg = SimpleNamespace(seed=11, env_id_base=5)
        self.gen = torch.Generator().manual_seed(seed)
        self.obs = torch.zeros(N, A, 11)
        self.reward, self.team = torch.zeros(N, A), torch.zeros(N)
        self.done, self.oob = torch.zeros(N, A, dtype=torch.uint8), torch.zeros(N, A, dtype=torch.uint8)
        self._src = {"src_x": torch.zeros(1, N, dtype=torch.int32), "src_y": torch.zeros(1, N, dtype=torch.int32)}
        self.log = dict(reset=[], act=[], epoch_end=[])

    def state(self, name: str) -> torch.Tensor:
        return self._src[name]

    def _rows(self) -> torch.Tensor:
        o = torch.rand(N, A, 11, generator=self.gen)
        o[..., 0] = torch.rand(N, A, generator=self.gen) * 400.0             # readings wide enough for a standard deviation above 1
        return o

    def _outs(self):
        return self.obs, self.reward, self.team, self.done, {"out_of_bounds": self.oob}

    def reset(self, mask=None):
        m = torch.ones(N, dtype=torch.bool) if mask is None else mask.bool().clone()
        self.log["reset"].append(m)
        rows, sx, sy = self._rows(), torch.randint(0, 2700, (N,), generator=self.gen), torch.randint(0, 2700, (N,), generator=self.gen)
        self.obs.copy_(torch.where(m.view(N, 1, 1), rows, self.obs))
        self._src["src_x"][0].copy_(torch.where(m, sx.int(), self._src["src_x"][0]))
        self._src["src_y"][0].copy_(torch.where(m, sy.int(), self._src["src_y"][0]))
        self.reward.masked_fill_(m.view(N, 1), 0.0); self.team.masked_fill_(m, 0.0)
        self.done.masked_fill_(m.view(N, 1), 0); self.oob.masked_fill_(m.view(N, 1), 0)
        return self._outs()

    def step(self, act8: torch.Tensor):
        assert act8.dtype == torch.int8 and tuple(act8.shape) == (N, A)
        self.log["act"].append(act8.clone())
        self.obs.copy_(self._rows())
        self.reward.copy_(torch.randn(N, A, generator=self.gen))
        self.team.copy_(self.reward.sum(dim=1))
        self.done.copy_((torch.rand(N, A, generator=self.gen) < 0.1).to(torch.uint8))   # the latch as each agent id saw it
        self.oob.copy_((torch.rand(N, A, generator=self.gen) < 0.3).to(torch.uint8))
        return self._outs()

    def action_uniforms(self, out: torch.Tensor) -> torch.Tensor:
        return out.copy_(torch.rand(N, A, generator=self.gen))

    def set_epoch_end(self) -> None:
        self.log["epoch_end"].append(len(self.log["act"]))


def collector():
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector
    torch.manual_seed(4)
    env = StubEnv()
    agents = {a: RNNAgentPPO(id=a, steps_per_epoch=T, steps_per_episode=L, seed=3 + a, device="cpu") for a in range(A)}
    with torch.no_grad():
        for ag in agents.values():
            for p in ag.agent.pi.parameters():
                p.mul_(2.0)
    col = RNNCollector(env, agents, T, L, use_graph=False)
    assert not col.use_glue and not col.use_k14 and col.bank.impl == "torch"
    return col


def drive(col, steps: int = T, epochs: int = EPOCHS):
    """{member: array}: after each epoch every buffer column, the statistics and the carried state; at the end the env's log"""
    out = {}
    col.start()
    for ep in range(epochs):
        col._cg.acc.zero_()
        col._cg.t.zero_()
        col._reset_hidden(None)
        with torch.no_grad():
            for t in range(steps):
                col._step(t == steps - 1)
        got = {**{k: getattr(col.buf, k) for k in BUFFER}, **{"stat_" + k: v for k, v in col._cg.acc.result().items()},
               "c_obs": col.obs, "c_ret": col.ep_ret, "c_steps": col.steps_in_ep, "c_h": col.h, "w_count": col.stat.count, "w_mean": col.stat.mean,
               "w_sq": col.stat.sq, "w_std": col.stat.std, "pf_h": col.bank.h, "pf_p": col.bank.p, "pf_episode": col.bank.episode,
               "pf_calls": col.bank.calls, "begun": col.episodes_begun, "t": col._t}
        out.update({f"ep{ep}.{k}": v.detach().clone().numpy() for k, v in got.items()})
    log = col.env.log
    out["log.reset"] = torch.stack(log["reset"]).numpy()
    out["log.act"] = torch.stack(log["act"]).numpy()
    out["log.epoch_end"] = np.asarray(log["epoch_end"], dtype=np.int64)
    return out


def covers(out) -> None:
    """terminal-only, timeout and epoch cuts, and bootstrap values that are not zero"""
    cut, last = out["ep0.cut"][:, :, 0], out["ep0.last_val"]
    assert cut[-1].all() and cut[:-1].any() and not cut[:-1].all()
    assert (last != 0).any() and ((last == 0).all(axis=2) & (cut == 1))[:-1].any()          # a cut without bootstrap: a pure terminal
    assert ((last != 0).any(axis=2) & (cut == 1))[:-1].any()                                # a cut with bootstrap before the epoch's end: a timeout
    assert out["log.epoch_end"].tolist() == [T, 2 * T]


def main():
    out = drive(collector())
    covers(out)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "members")


if __name__ == "__main__":
    main()
