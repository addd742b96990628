"""What the four GPU suites of the RAD-TEAM (CNN) team kernels share (tests/test_cnn_team_eval_gpu.py, test_cnn_team_step_gpu.py and their
any-side twins test_cnn_sized_team_eval_gpu.py, test_cnn_sized_team_step_gpu.py): the small pieces (bits, stream, ptr, the sentinel, the
parameter arrays, the network builders), a record per kernel family that says how its five entry points are called (FAMILY27, SIZED), the
guarded calls of the two heads, the team-trunk check, the existing path, the once-per-team master, and the bodies of the tests the two
families have in common.  The float64 rule itself is tests/_cnn_team_ref.py's; tests/test_cnn_team_drive_cpu.py holds the pure parts of
this module to planted faults without a GPU."""
import ctypes as C
import types

import numpy as np
import torch

import _cnn_sized_team_ref as S
import _cnn_team_ref as T
from radiation_ppo_amd import _lib

SENTINEL = -12345.678
GUARD = 4096                                                # floats of NaN on both sides of the sized step head's scratch
SEED = 1234
KEYS = ("obs", "act", "rew", "val", "logp", "last_val", "cut", "adv", "ret")


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def is_sentinel(t):
    return torch.equal(bits(t), bits(torch.full_like(t, SENTINEL)))


def guards_intact(buf, lo, hi):
    """buf[:lo] and buf[hi:] still hold the sentinel, bit for bit"""
    return is_sentinel(buf[:lo]) and is_sentinel(buf[hi:])


def fmt(d):
    return " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in d.items())


def call(name, *args):
    """The library's `name` on torch's current stream, tensors as their addresses (None: NULL), then a synchronize: the return code.
    Pass tensors, not addresses: the argument list keeps a temporary such as cells.int().cuda() alive until the kernel is done (the
    step suites once passed the data_ptr()s of two such temporaries, freed and handed out again before the launch)."""
    rc = getattr(_lib.load(), name)(*[ptr(a) if torch.is_tensor(a) else a for a in args], stream())
    torch.cuda.synchronize()
    return rc


def run(name, *args):
    _lib.check(call(name, *args), name)


def _param_array(cls, seqs, layers):
    return (cls * len(seqs))(*[cls(*[ptr(q) for i in layers for q in (s[i].weight, s[i].bias)]) for s in seqs])


def head_params(seqs):
    return _param_array(_lib.RsCnnHeadParams, seqs, (6, 8, 10))


def conv_params(seqs):
    return _param_array(_lib.RsCnnConvParams, seqs, (0, 3))


def trunk_prepare(seqs, cin):
    """every network's convolution weights in K9's layout: wt [n, scratch]"""
    wt = torch.empty(len(seqs), _lib.load().rs_cnn_trunk_scratch_floats(cin), dtype=torch.float32, device="cuda")
    for i, s in enumerate(seqs):
        run("rs_cnn_trunk_prepare", cin, s[0].weight, s[0].bias, s[3].weight, s[3].bias, wt[i])
    return wt


def critics(n, seed, M=27):
    """n critic networks for M x M maps with biases that matter and visibly different values"""
    from radiation_ppo_amd.maps import CNNCritic
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        mods = [CNNCritic(map_dim=(M, M)) for _ in range(n)]
    with torch.no_grad():
        for m in mods:
            m.critic[0].bias.uniform_(-0.05, 0.15)
            m.critic[3].bias.uniform_(-0.1, 0.1)
            for i in (6, 8, 10):
                for p in m.critic[i].parameters():
                    p.mul_(T.SCALE)
    return mods


def actors(A, M, seed):
    from radiation_ppo_amd.maps import CNNActor
    torch.manual_seed(seed)
    seqs = [CNNActor(map_dim=(M, M)).cuda().actor for _ in range(A)]
    with torch.no_grad():                                  # make biases matter (the shortcut's max(0 + b1, 0), pool ties, ReLU gates)
        for s in seqs:
            s[0].bias.uniform_(-0.05, 0.15)
            s[3].bias.uniform_(-0.1, 0.1)
    return seqs


def onehot_rows(A, flat, ks):
    """(a2 [A, len(ks), flat] whose row n is 1.0 at ks[n] and 0 elsewhere, uniforms u [len(ks), A])"""
    N = len(ks)
    a2 = torch.zeros(A, N, flat, device="cuda")
    a2[:, torch.arange(N), torch.tensor(ks)] = 1.0
    return a2, torch.rand(N, A, device="cuda")


def check_onehot_y1(y1, seqs, ks, tag):
    """on onehot_rows, y1[row][n][j] is a single term plus exact zeros, then the bias: float32(W1[j][ks[n]] + b1[j]) of seqs[row],
    bit for bit"""
    for row, s in enumerate(seqs):
        with torch.no_grad():
            want = s[6].weight[:, ks].t().contiguous() + s[6].bias                    # [N, 32], one float32 add each
        bad = (bits(y1[row]) != bits(want)).nonzero()
        assert bad.numel() == 0, (tag, row, [(ks[n], j) for n, j in bad[:6].tolist()])
        assert float(want.abs().min()) > 0


# ------------------------------------------------------------------------------------------------ the two families
# w is what a family's trunks read the convolutions from: trunk_prepare's wt [n, scratch] (27 x 27) or the networks themselves (any side)
def _sized_one_trunk(w, i, maps, cells, pcells, A, a, out):
    s = w[i]
    run("rs_cnn_sized_infer", maps, cells, pcells, A, a, maps.shape[0], maps.shape[2], s[0].weight, s[0].bias, s[3].weight, s[3].bias, out)


def _sized_step_head(ap, A, cp, nc, flat, io, N, rows):
    """through a NaN-filled scratch of exactly the size the size function gives for `rows`, guarded on both sides"""
    need = _lib.load().rs_cnn_sized_team_head_scratch_floats(flat, rows, N)
    assert need > 0
    scr = torch.full((need + 2 * GUARD,), float("nan"), device="cuda")
    rc = call("rs_cnn_sized_team_step_head", ap, A, cp, nc, flat, *io, scr[GUARD:], need, N)
    assert bool(torch.isnan(scr[:GUARD]).all()) and bool(torch.isnan(scr[GUARD + need:]).all())       # nothing written beside the scratch
    return rc


FAMILY27 = types.SimpleNamespace(
    label="cnn team", team=T.team, case=lambda t, N: f"N{N} A{t.A}", k1=lambda flat: T.K1, critic_seed=lambda t: 7300 + t.A,
    names=dict(team_trunk="rs_cnn_team_trunk_infer", critic_trunk="rs_cnn_team_critic_trunk_infer", one_trunk="rs_cnn_trunk_infer",
               eval_head="rs_cnn_team_eval_head", step_head="rs_cnn_team_step_head"),
    weights=trunk_prepare,
    team_trunk=lambda w, maps, c32, p32, out: run("rs_cnn_team_trunk_infer", maps, c32, p32, len(w), maps.shape[0], w, out),
    critic_trunk=lambda w, maps, out: run("rs_cnn_team_critic_trunk_infer", maps, len(w), maps.shape[0], w, out),
    one_trunk=lambda w, i, maps, cells, pcells, A, a, out: run("rs_cnn_trunk_infer", maps, cells, pcells, A, a, maps.shape[0], w[i], out),
    eval_head=lambda hp, A, flat, io, N: call("rs_cnn_team_eval_head", hp, A, *io, N),
    step_head=lambda ap, A, cp, nc, flat, io, N, rows: call("rs_cnn_team_step_head", ap, A, cp, nc, *io, N))
SIZED = types.SimpleNamespace(
    label="cnn sized team", team=lambda key: S.team(*key), case=lambda t, N: f"P{t.P} flat {t.flat} N{N} A{t.A}", k1=S.k1,
    critic_seed=lambda t: 7400 + 10 * t.P + t.A,
    names=dict(team_trunk="rs_cnn_sized_team_infer", critic_trunk="rs_cnn_sized_team_critic_infer", one_trunk="rs_cnn_sized_infer",
               eval_head="rs_cnn_sized_team_eval_head", step_head="rs_cnn_sized_team_step_head"),
    weights=lambda seqs, cin: seqs,
    team_trunk=lambda w, maps, c32, p32, out: run("rs_cnn_sized_team_infer", maps, c32, p32, len(w), maps.shape[0], maps.shape[2],
                                                  conv_params(w), out),
    critic_trunk=lambda w, maps, out: run("rs_cnn_sized_team_critic_infer", maps, len(w), maps.shape[0], maps.shape[2], conv_params(w), out),
    one_trunk=_sized_one_trunk,
    eval_head=lambda hp, A, flat, io, N: call("rs_cnn_sized_team_eval_head", hp, A, flat, *io, N),
    step_head=_sized_step_head)


# ------------------------------------------------------------------------------------------------ guarded calls
def eval_head(fam, seqs, flat, a2, u, alive, N, outputs=True):
    """The family's evaluation head into sentinel-guarded buffers: dict(act8 [N, A], act [A, N], logp [A, N], y1 [A, N, 32]);
    outputs=False: the three optional outputs NULL."""
    A = len(seqs)
    act8 = torch.full((N + 2, A), -1, dtype=torch.int8, device="cuda")
    act = torch.full((A * N + 2,), -1, dtype=torch.int64, device="cuda")
    logp = torch.full((A * N + 2,), SENTINEL, device="cuda")
    y1 = torch.full((A * N + 2, 32), SENTINEL, device="cuda")
    o = (act[1:], logp[1:], y1[1:]) if outputs else (None, None, None)
    _lib.check(fam.eval_head(head_params(seqs), A, flat, (a2, u, alive, act8[1:], *o), N), fam.names["eval_head"])
    assert bool((act8[0] == -1).all()) and bool((act8[N + 1] == -1).all())          # the guards on both sides
    assert int(act[0]) == -1 and int(act[-1]) == -1
    assert guards_intact(logp, 1, -1) and guards_intact(y1, 1, -1)
    if not outputs:
        assert bool((act == -1).all()) and is_sentinel(logp)
    return dict(act8=act8[1:N + 1], act=act[1:A * N + 1].view(A, N), logp=logp[1:A * N + 1].view(A, N), y1=y1[1:A * N + 1].view(A, N, 32))


def step_head(fam, actor_seqs, critic_seqs, flat, a2a, a2c, u, N, A, mask=None, boot=False, rows_of_scratch=None):
    """The family's step head into sentinel-filled, guarded buffers (the any-side one through its NaN-filled, guarded scratch, sized for
    the launched rows unless rows_of_scratch says otherwise): dict(rc, act [A, N], f [A, 3, N], act8 [N, A], y1 [A + C, N, 32]).
    boot=True: the bootstrap round, the actors' arguments NULL."""
    nc = len(critic_seqs)
    act = torch.full((A * N + 2,), -1, dtype=torch.int64, device="cuda")
    f = torch.full((A * 3 * N + 2,), SENTINEL, device="cuda")
    act8 = torch.full((N + 2, A), -1, dtype=torch.int8, device="cuda")
    y1 = torch.full(((A + nc) * N + 2, 32), SENTINEL, device="cuda")
    io = (None, a2c, None, None, f[1:], None, mask, y1[1:]) if boot else (a2a, a2c, u, act[1:], f[1:], act8[1:], mask, y1[1:])
    rc = fam.step_head(None if boot else head_params(actor_seqs), A, head_params(critic_seqs), nc, flat, io, N,
                       rows_of_scratch or (nc if boot else A + nc))
    assert int(act[0]) == -1 and int(act[-1]) == -1 and bool((act8[0] == -1).all()) and bool((act8[N + 1] == -1).all())
    assert guards_intact(f, 1, -1) and guards_intact(y1, 1, -1)
    out = dict(rc=rc, act=act[1:A * N + 1].view(A, N), f=f[1:A * 3 * N + 1].view(A, 3, N), act8=act8[1:N + 1],
               y1=y1[1:(A + nc) * N + 1].view(A + nc, N, 32))
    assert bool(torch.isfinite(out["f"]).all()) and bool(torch.isfinite(out["y1"]).all())             # no NaN of a scratch reached an output
    return out


# ------------------------------------------------------------------------------------------------ trunks, the existing path, the master
def check_team_trunk(fam, role, seqs, maps, cells=None, pcells=None):
    """The family's team trunk of `role` ("actor": maps, cells, pcells; "critic": maps alone) for the networks seqs: a2 [n, N, flat]
    between sentinel guard rows, every element written, and each network's rows equal to one single-network launch bit for bit."""
    actor = role == "actor"
    n, N, M = len(seqs), maps.shape[0], maps.shape[2]
    flat = 16 * (M // 2) ** 2
    w = fam.weights(seqs, 6 if actor else 4)
    maps = maps.cuda()
    G = 2 * flat                                           # guard rows on both sides of [n][N][flat]
    buf = torch.full((G + n * N * flat + G,), SENTINEL, device="cuda")
    if actor:
        cells, pcells = cells.cuda(), pcells.cuda()
        fam.team_trunk(w, maps, cells.int().contiguous(), pcells.int().contiguous(), buf[G:])
    else:
        fam.critic_trunk(w, maps, buf[G:])
    assert guards_intact(buf, G, G + n * N * flat), (M, N, n)
    got = buf[G:G + n * N * flat].view(n, N, flat)
    assert not bool((got == SENTINEL).any()), (M, N, n)    # every element written
    for i in range(n):
        want = torch.full((N, flat), SENTINEL, device="cuda")
        fam.one_trunk(w, i, maps, cells, pcells, n if actor else 0, i if actor else -1, want)
        assert float(want.abs().max()) > 0 and bool(torch.isfinite(want).all())
        bad = (bits(got[i]) != bits(want)).nonzero()
        assert bad.numel() == 0, (M, N, n, i, bad[:4].tolist())
    if n > 1:
        assert not torch.equal(got[0], got[n - 1])         # the networks are told apart: their own weights (and cell columns)
    return got


def existing_path(fam, m, a, N, u, alive):
    """The composed path for agent a on the case's lanes: one single-agent trunk launch + BLAS linear + rs_cnn_head + the idle rule."""
    t, s = m["t"], m["seqs"][a]
    a2 = torch.empty(N, t.flat, device="cuda")
    fam.one_trunk(m["w"], a, t.maps[:N].cuda().contiguous(), t.cells[:N].cuda().contiguous(), t.pcells[:N].cuda().contiguous(), t.A, a, a2)
    with torch.no_grad():
        y1 = torch.nn.functional.linear(a2, s[6].weight, s[6].bias)
    act = torch.empty(N, dtype=torch.int64, device="cuda")
    logp = torch.empty(N, device="cuda")
    run("rs_cnn_head", y1, s[8].weight, s[8].bias, s[10].weight, s[10].bias, 8, u.data_ptr() + 4 * a, t.A, act, logp, None, 1, None, 1, 0, None, N)
    return a2, y1, act, logp, torch.where(alive != 0, act, torch.full_like(act, 8)).to(torch.int8)


_MASTER = {}


def master(fam, key, critics_too=False, head_too=False):
    """Once per family and team (key: A, or (P, A) for any side): the ref module's actors on the GPU, a2a [A, master lanes, flat] from the
    team trunk on the master maps and u.  critics_too: A critics and their team trunk's a2c.  head_too: the float64 references and the
    evaluation head's outputs on all master lanes (what a case's lanes must equal bit for bit: grid independence)."""
    m = _MASTER.get((fam.label, key))
    if m is None:
        t = fam.team(key)
        seqs = [T.clone_seq(ac.actor, "cuda") for ac in t.actors]
        w = fam.weights(seqs, 6)
        a2a = torch.empty(t.A, t.N, t.flat, device="cuda")
        fam.team_trunk(w, t.maps.cuda(), t.cells.int().cuda(), t.pcells.int().cuda(), a2a)
        assert float(a2a.min()) >= 0.0 and float((a2a == 0).float().mean()) > 0.2      # non-negative and sparse, as in a run
        m = _MASTER[fam.label, key] = dict(t=t, seqs=seqs, w=w, a2a=a2a, u=t.u.cuda())
    t = m["t"]
    if critics_too and "crit" not in m:
        m["cpu_critics"] = critics(t.A, fam.critic_seed(t), t.M)
        m["crit"] = [T.clone_seq(c.critic, "cuda") for c in m["cpu_critics"]]
        m["a2c"] = torch.empty(t.A, t.N, t.flat, device="cuda")
        fam.critic_trunk(fam.weights(m["crit"], 4), t.maps.cuda(), m["a2c"])
        assert float(m["a2c"].min()) >= 0.0 and float(m["a2c"].max()) > 0.0
    if head_too and "out" not in m:
        m["refs"] = [T.reference(t.actors[a].actor, m["a2a"][a], t.u[:, a], fam.k1(t.flat)) for a in range(t.A)]
        m["out"] = eval_head(fam, m["seqs"], t.flat, m["a2a"], m["u"], T.alive_for(t, t.N).cuda(), t.N)
    return m


# ------------------------------------------------------------------------------------------------ shared bodies: the heads
def head_matches_float64_and_so_does_the_existing_path(fam, key, N):
    m = master(fam, key, head_too=True)
    t, seqs = m["t"], m["seqs"]
    A = t.A
    a2 = m["a2a"][:, :N].contiguous()
    u, alive = t.u[:N].cuda().contiguous(), T.alive_for(t, N).cuda()
    assert int(alive[N - 1]) == 0 and (N == 1 or (int(alive[0]) == 1 and 0 < int(alive.sum()) < N))
    got = eval_head(fam, seqs, t.flat, a2, u, alive, N)
    refs = m["refs"] if N == t.N else [T.reference(t.actors[a].actor, a2[a], u[:, a], fam.k1(t.flat)) for a in range(A)]
    worst = {k: dict(y1=0.0, logp=0.0, differing=0, unexcused=0, act8=0) for k in ("kernel", "existing")}
    fails = []
    for a in range(A):
        assert T.distinct_actions(m["refs"][a]) >= 3, a                 # a visibly non-uniform policy that still draws several actions
        if N >= 31:
            assert T.distinct_actions(refs[a]) >= 3, (N, a)
        q = T.ratios(refs[a], u[:, a], alive, got["act"][a], got["logp"][a], got["act8"][:, a], y1=got["y1"][a])
        xa2, y1, act, logp, a8 = existing_path(fam, m, a, N, u, alive)
        assert torch.equal(bits(xa2), bits(a2[a])), a                # both paths start from the same trunk bits
        qe = T.ratios(refs[a], u[:, a], alive, act, logp, a8, y1=y1)
        for name, r in (("kernel", q), ("existing", qe)):
            for k in r:
                worst[name][k] = max(worst[name][k], r[k])
            if not T.passes(r):
                fails.append((name, a, r))
    for name in worst:
        print(f"{fam.label} head {fam.case(t, N)} {name:8s} | " + fmt(worst[name]))
    assert not [f for f in fails if f[0] == "existing"], fails       # the existing path past 1.0 would mean the MODEL is wrong
    assert not fails, fails
    assert bool((got["act"] >= 0).all()) and bool((got["act"] <= 7).all())
    want8 = torch.where(alive.view(N, 1) != 0, got["act"].t(), torch.full_like(got["act"].t(), 8)).to(torch.int8)
    assert torch.equal(got["act8"], want8)                           # act8[n][a] = alive[n] ? act[a][n] : 8, exactly
    # the optional outputs NULL: act8 alone, the same rows; a second call: the same bits
    only8 = eval_head(fam, seqs, t.flat, a2, u, alive, N, outputs=False)
    assert torch.equal(only8["act8"], got["act8"])
    again = eval_head(fam, seqs, t.flat, a2, u, alive, N)
    for k in got:
        assert torch.equal(bits(again[k]), bits(got[k])) if got[k].dtype == torch.float32 else torch.equal(again[k], got[k]), k
    # the same lanes inside the master call: equal bits, no dependence on N or the grid
    big = m["out"]
    assert torch.equal(bits(big["y1"][:, :N]), bits(got["y1"])) and torch.equal(bits(big["logp"][:, :N]), bits(got["logp"]))
    assert torch.equal(big["act"][:, :N], got["act"])


def bootstrap_round(fam, key, boot_y1, masked_y1=None):
    """The bootstrap round writes slot 2 under the mask and nothing else, a step round under a mask writes the masked-in envs alone, an
    empty mask writes nothing.  What y1 holds under a mask is the family's (the 27 x 27 kernel skips whole tiles, the k-split one masks
    per lane): boot_y1(got, the step round of that critic mode, on, A) and masked_y1(got, on).  Returns (m, the step rounds of both
    critic modes) for the family's refusals."""
    A, N = 3, 130
    m = master(fam, key, critics_too=True)
    flat, a2a, a2c, u = m["t"].flat, m["a2a"], m["a2c"], m["u"]
    step = {nc: step_head(fam, m["seqs"], m["crit"][:nc], flat, a2a, a2c[:nc].contiguous(), u, N, A) for nc in (1, A)}
    mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
    mask[[64, 70, 127, 128, 129]] = 1                                       # lanes 0..63 all zero: the first tile returns early
    mask[100] = 7                                                           # any non-zero byte counts
    on = mask != 0
    for nc in (1, A):
        got = step_head(fam, None, m["crit"][:nc], flat, None, a2c[:nc].contiguous(), None, N, A, mask=mask, boot=True)
        assert got["rc"] == 0
        assert bool((got["act"] == -1).all()) and bool((got["act8"] == -1).all())
        assert is_sentinel(got["f"][:, 0]) and is_sentinel(got["f"][:, 1]) and is_sentinel(got["y1"][:A])
        assert is_sentinel(got["f"][:, 2][:, ~on])
        boot_y1(got, step[nc], on, A)
        # the masked envs: the step round's value bits (the same critic on the same a2), in slot 2
        assert torch.equal(bits(got["f"][:, 2][:, on]), bits(step[nc]["f"][:, 1][:, on])), nc
    # a step round under a mask: the masked-out envs write nothing, the others what the unmasked round wrote
    got = step_head(fam, m["seqs"], m["crit"], flat, a2a, a2c, u, N, A, mask=mask)
    assert got["rc"] == 0
    assert bool((got["act"][:, ~on] == -1).all()) and bool((got["act8"][~on] == -1).all()) and is_sentinel(got["f"][:, :, ~on])
    if masked_y1 is not None:
        masked_y1(got, on)
    assert torch.equal(got["act"][:, on], step[A]["act"][:, on]) and torch.equal(bits(got["f"][:, :2][:, :, on]), bits(step[A]["f"][:, :2][:, :, on]))
    assert torch.equal(got["act8"][on].long(), got["act"][:, on].t())
    # an empty mask: nothing written, RS_OK
    got = step_head(fam, None, m["crit"], flat, None, a2c, None, N, A, mask=torch.zeros(N, dtype=torch.uint8, device="cuda"), boot=True)
    assert got["rc"] == 0 and is_sentinel(got["f"]) and is_sentinel(got["y1"])
    return m, step


def sharding(fam, key):
    """N = 130 in one call against the same lanes as two calls of 65: equal bits in every output.  Returns (m, the whole call)."""
    A, N = 3, 130
    m = master(fam, key, critics_too=True)
    flat = m["t"].flat
    whole = step_head(fam, m["seqs"], m["crit"], flat, m["a2a"], m["a2c"], m["u"], N, A)
    for lo in (0, 65):
        sl = slice(lo, lo + 65)
        part = step_head(fam, m["seqs"], m["crit"], flat, m["a2a"][:, sl].contiguous(), m["a2c"][:, sl].contiguous(), m["u"][sl].contiguous(), 65, A)
        assert torch.equal(part["act"], whole["act"][:, sl]) and torch.equal(part["act8"], whole["act8"][sl])
        assert torch.equal(bits(part["f"][:, :2]), bits(whole["f"][:, :2, sl])) and torch.equal(bits(part["y1"]), bits(whole["y1"][:, sl]))
    return m, whole


# ------------------------------------------------------------------------------------------------ shared bodies: the collector
def collector(team, flag, walls, T_, L, N=64, CA=3, base=32, use_graph=False, on=None, record=None, ids=None, mixed=False):
    """(CNNCollector, agents) of CA agents on N envs, T_ steps an epoch and L an episode, walls on (27 x 27 maps) or off.  flag: the
    collector's switch of the family's team round ("team_round" / "sized_team_round"), set to `on` when given; "_" + flag is the round
    itself, spied on with `record` (the bootstrap rounds' step, maps and masks, as the round receives them).  mixed: the last agent has a
    critic of its own beside the others' global one; ids: the agents' ids."""
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic, heat_map_geometry
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    torch.manual_seed(8)
    env = RadSearchVec(N, number_agents=CA, obstruction_count=2, enforce_grid_boundaries=walls, seed=SEED, env_id_base=base)
    kw = {} if walls else dict(map_dim=tuple(heat_map_geometry(env, L, False)[2]))
    gc = CNNCritic(**kw).cuda() if team else None
    shares = lambda i: team and not (mixed and i == CA - 1)
    agents = {i: CNNAgentPPO(id=i, GlobalCritic=gc if shares(i) else None,
                             GlobalCriticOptimizer=torch.optim.Adam(gc.parameters(), lr=1e-3) if shares(i) else None, **kw)
              for i in (ids if ids is not None else range(CA))}
    with torch.no_grad():
        for ag in agents.values():
            for p in list(ag.pi.actor[6:].parameters()):
                p.mul_(3.0)                                   # visibly non-uniform policies
    col = CNNCollector(env, agents, T_, L, global_critic_flag=team, use_graph=use_graph)
    if on is not None:
        setattr(col, flag, on)
    if record is not None:
        inner = getattr(col, "_" + flag)

        def spy(maps, mask8=None):
            if mask8 is not None:
                record.append((int(col._t), maps.clone(), mask8.clone()))
            return inner(maps, mask8=mask8)
        setattr(col, "_" + flag, spy)
    return col, agents


def stored(col):
    return {**{k: getattr(col.buf, k).clone() for k in KEYS}, "shared": col.shared.clone(), "cells": col.cells.clone(),
            "pcells": col.pcells.clone(), "complete_len": col.complete_len.clone()}


def collector_round_against_the_per_agent_round_and_the_modules(make, flag, team, CT, CA):
    """make(team, **kw) is the suite's collector (kw: collector()'s).  Returns (the collector with the round on, the one with it off),
    both after their epoch, for the family's own post-conditions."""
    boots = []
    cf, af = make(team, record=boots)
    assert getattr(cf, "use_" + flag)
    cf.collect()
    cm, _ = make(team, on=False)
    assert not getattr(cm, "use_" + flag) and cm.use_heads
    cm.collect()
    # ---- the first lock-step, where both collectors see the same state
    same = cf.buf.act[0] == cm.buf.act[0]
    assert float(same.float().mean()) > 0.99
    assert torch.allclose(cf.buf.logp[0][same], cm.buf.logp[0][same], rtol=1e-4, atol=2e-5)
    assert torch.allclose(cf.buf.val[0], cm.buf.val[0], rtol=1e-4, atol=2e-5)
    assert torch.equal(cf.buf.obs[0], cm.buf.obs[0]) and torch.equal(cf.shared[0], cm.shared[0])
    assert torch.equal(cf.cells[0], cm.cells[0]) and torch.equal(cf.pcells[0], cm.pcells[0])
    # ---- the whole epoch: every stored row against the modules on the stored maps
    assert int(cf.buf.act.min()) >= 0 and int(cf.buf.act.max()) <= 7 and int(torch.unique(cf.buf.act).numel()) >= 3
    for t in range(CT):
        for a, ag in af.items():
            logits = ag.pi.logits_from_maps(cf.shared[t], cf.cells[t], cf.pcells[t], a)
            lp = torch.log_softmax(logits, dim=-1).gather(-1, cf.buf.act[t, :, a].unsqueeze(-1)).squeeze(-1)
            assert torch.allclose(cf.buf.logp[t, :, a], lp, rtol=1e-4, atol=2e-5), (t, a)
            assert torch.allclose(cf.buf.val[t, :, a], ag.critic.value_from_maps(cf.shared[t]), rtol=1e-4, atol=2e-5), (t, a)
    if not team:
        assert not torch.equal(cf.buf.val[:, :, 0], cf.buf.val[:, :, CA - 1])
    # ---- last_val: non-zero on cut rows only, and there the critic on the bootstrap round's maps
    nz = cf.buf.last_val != 0
    assert int(nz.sum()) > 0 and bool((cf.buf.cut[nz.any(dim=2)] == 1).all())
    assert len(boots) == CT
    timeouts = 0
    for t, maps, mask in boots:
        on = mask != 0
        assert not bool(nz[t][~on].any()), t
        if t < CT - 1:
            timeouts += int(on.sum())                                   # before the epoch's end only time-outs are bootstrapped
        for a, ag in af.items():
            v = ag.critic.value_from_maps(maps)
            assert torch.allclose(cf.buf.last_val[t, :, a][on], v[on], rtol=1e-4, atol=2e-5), (t, a)
    assert timeouts > 0 and bool((boots[-1][2] != 0).all())
    return cf, cm


def collector_graph_equals_eager_and_two_halves_equal_the_whole(make, flag, team, CN):
    runs = {}
    for name, kw in (("eager", dict()), ("graph", dict(use_graph=True)), ("lo", dict(N=CN // 2, base=32)), ("hi", dict(N=CN // 2, base=32 + CN // 2))):
        col, _ = make(team, **kw)
        assert getattr(col, "use_" + flag)
        col.collect()
        assert (col._graph is not None) == (name == "graph") and col.env.error_flags() == 0
        runs[name] = stored(col)
    for k in runs["eager"]:
        assert torch.equal(runs["graph"][k], runs["eager"][k]), k
        halves = torch.cat([runs["lo"][k], runs["hi"][k]], dim=0 if k == "complete_len" else 1)
        if k in ("adv", "ret"):
            continue                                                    # (GAE over the rows checked here)
        assert torch.equal(halves, runs["eager"][k]), k


def train_ppo_cnn_one_epoch(walls):
    """one train_PPO('cnn') epoch of 2 agents with a global critic on 16 envs: finite losses and a finite buffer; returns the trainer"""
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.train import train_PPO
    A = 2
    env = RadSearchVec(16, number_agents=A, obstruction_count=1, enforce_grid_boundaries=walls, seed=6)
    sim = train_PPO(env=env, logger_kwargs={}, ppo_kwargs=dict(steps_per_epoch=16, steps_per_episode=8, number_of_agents=A, train_pi_iters=2,
                                                               train_v_iters=2),
                    seed=6, number_of_agents=A, actor_critic_architecture="cnn", global_critic_flag=True, steps_per_epoch=16,
                    steps_per_episode=8, total_epochs=1)
    sim.train()
    for i in range(A):
        rows = sim.loggers[i].rows
        assert len(rows) == 1 and np.isfinite(rows[0]["loss_policy"]), i
    assert np.isfinite(sim.loggers[0].rows[0]["loss_critic"])         # only agent 0 updates the global critic (ppo.py:858)
    buf = sim.collector.buf
    assert bool(torch.isfinite(buf.logp).all()) and bool(torch.isfinite(buf.val).all()) and int(buf.act.max()) <= 7
    return sim
