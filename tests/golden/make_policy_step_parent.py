"""Fixture of the policy kernels' step outputs -- what no recorded file held before: log-probabilities, values, GRU states, y1_out and
the collectors' [A][3][N] rows -- recorded from commit cec4a92 ("Collectors: one lock-step glue under the three training collectors"),
the commit BEFORE kernels began to share the action draw (csrc/rs_action.hpp) and the RAD-TEAM head tail (csrc/rs_cnn_head.hpp).  At
that commit every kernel carried its own copy; what the copies computed is what a kernel must go on computing, on a shared piece or on
its own text.  Only C entry points are called (radiation_ppo_amd._lib), so the recorder runs on the parent's
tree and on every later one.

Every case has N = 130 lanes (two full 64-lane groups and a ragged one of 2) and runs in two forms
  <case>.nomask.*   every lane live (mask NULL, or a mask of ones where the entry point requires one)
  <case>.mask.*     lanes 64..127 (a whole group) and the single lanes 3, 17 and 129 switched off
Every output starts from a sentinel and is stored whole, but for two that equal a stored member bit for bit, which run() asserts: the
states rs_rnn_team_eval_step leaves (rs_rnn_team_step's h) and the y1_out of the CNN bootstrap rounds (the step round's critic rows).
The uniforms are seeded draws with the lanes 5 and 70 set to 0.0 and the lanes 9, 80 and 128 to the largest float32 below 1.  rs_rnn_policy_step has no mask argument: it is in the nomask form only.  rs_ff_team_step
ignores the mask in its step round (include/radsearch.h): the recorder asserts that its masked step round equals the unmasked one.

Two conditions keep the fixture from proving nothing, asserted by main() and by the test:
  - per entry point that draws, every action 0..7 occurs (DRAWS: the entry point's members that hold actions).  The seeds and the
    scales below were chosen on the CPU so that this holds for the float64 references of tests/_f64_ref.py alone:
        python tests/golden/make_policy_step_parent.py --reference
  - every masked form leaves the sentinel in the masked-out lanes of every output the mask governs.

    python tests/golden/make_policy_step_parent.py [OUT.npz]   # on the MI355X; on a later tree it must reproduce the committed file
"""
import copy
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
OUT = os.path.join(HERE, "policy_step_parent.npz")
for _d in (ROOT, TESTS):
    if _d not in sys.path:
        sys.path.insert(0, _d)

N = 130
OFF_GROUP, OFF_LANES = (64, 128), (3, 17, 129)
F_MARK, ACT_MARK, ACT8_MARK = -12345.678, -7, -3
ONE_BELOW = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
RNN_SCALE = 1.5          # on every policy parameter of the recurrent agents (GRU and heads)
HEAD_Y1_SCALE = 0.5      # rs_cnn_head: on _f64_ref.head_case's y1 rows
A2_DENSITY, A2_SCALE = 0.25, 0.3    # the CNN team heads' a2 rows: non-negative and sparse, as a trunk's output
FF_X_SCALE = 0.5         # rs_ff_team_step: on the standard-normal observations
SIZED = [(1, 2, 2), (20, 9, 33), (40, 64, 7), (64, 64, 64)]       # one per GRU tier 16 / 32 / 48 / 64, odd and partial head blocks

# case: (family, parameters)
CASES = {
    "rnn-default": ("rnn", dict(widths=None, A=3)),
    **{"rnn-sized-" + "x".join(map(str, w)): ("rnn", dict(widths=w, A=2)) for w in SIZED},
    "cnn-head": ("cnn_head", dict(A=3, a=1)),
    "cnn27-A2-C1": ("cnn_team", dict(P=None, A=2, C=1)),
    "cnn27-A2-C2": ("cnn_team", dict(P=None, A=2, C=2)),
    "cnn-sized-p4": ("cnn_team", dict(P=4, A=1, C=1)),
    "cnn-sized-p5": ("cnn_team", dict(P=5, A=1, C=1)),
    "cnn-sized-p6": ("cnn_team", dict(P=6, A=1, C=1)),
    "ff-A3": ("ff", dict(A=3)),
}
FORMS = ("nomask", "mask")
# entry point that draws: the suffixes of its action members (any case, any form)
DRAWS = {
    "rs_rnn_policy_step": (".rs_rnn_policy_step.act",),
    "rs_rnn_policy_step_rows": (".rs_rnn_policy_step_rows.act",),
    "rs_rnn_team_step": (".rs_rnn_team_step.act",),
    "rs_rnn_team_eval_step": (".rs_rnn_team_eval_step.act8",),
    "rs_rnn_sized_step": (".rs_rnn_sized_step.act",),
    "rs_rnn_sized_team_step": (".rs_rnn_sized_team_step.act",),
    "rs_cnn_head": (".rs_cnn_head.act",),
    "rs_cnn_team_step_head": (".rs_cnn_team_step_head.act",),
    "rs_cnn_sized_team_step_head": (".rs_cnn_sized_team_step_head.act",),
    "rs_ff_team_step": (".rs_ff_team_step.act",),
}


def _torch():
    import torch
    return torch


def mask_cpu():
    torch = _torch()
    m = torch.ones(N, dtype=torch.uint8)
    m[OFF_GROUP[0]:OFF_GROUP[1]] = 0
    m[list(OFF_LANES)] = 0
    return m


def uniforms(A, g):
    torch = _torch()
    u = torch.rand(N, A, generator=g)
    u[[5, 70]] = 0.0
    u[[9, 80, 128]] = ONE_BELOW
    return u


# ------------------------------------------------------------------------------------------------ inputs, built on the CPU
def rnn_inputs(widths, A):
    """A recurrent agents as tests/test_rnn_team_step_gpu.py's `packed` seeds them (policy parameters x RNN_SCALE), rows and states"""
    torch = _torch()
    import _rnn_eval as H
    from radiation_ppo_amd.rada2c import RNNModelActorCritic
    hid = 24 if widths is None else widths[0]
    acs = []
    for a in range(A):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(50 + 7 * a)
            ac = RNNModelActorCritic(**(H._args(*widths, 16) if widths else {}))
        assert ac.fused_policy == (widths is None) and ac.sized_policy == (widths is not None)
        with torch.no_grad():
            for q in ac.pi.parameters():
                q.mul_(RNN_SCALE)
        acs.append(ac)
    g = torch.Generator().manual_seed(2000 + 10 * hid + A)
    x, loc = torch.rand(N, A, 11, generator=g) * 2.0 - 1.0, torch.rand(N, A, 2, generator=g)
    h0 = (torch.rand(A, N, hid, generator=g) * 2.0 - 1.0) / hid ** 0.5
    return dict(acs=acs, x=x, loc=loc, h0=h0, u=uniforms(A, g), hid=hid)


def _sized_actors(P, A, M):
    """CNNActor for M x M maps as tests/_cnn_sized_team_ref.team scales them (that helper knows no P = 6)"""
    torch = _torch()
    import _cnn_sized_team_ref as S
    from radiation_ppo_amd.maps import CNNActor
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7300 + 10 * P + A)
        actors = [CNNActor(map_dim=(M, M)) for _ in range(A)]
    with torch.no_grad():
        for ac in actors:
            for i in (6, 8, 10):
                for p in ac.actor[i].parameters():
                    p.mul_(S.SCALE)
    return actors


def cnn_team_inputs(P, A, C_):
    """actors' and critics' Sequentials on the CPU and a2 rows [A][N][flat], [C][N][flat]"""
    torch = _torch()
    import _cnn_team_drive as D
    if P is None:
        import _cnn_team_ref as T
        flat = 2704
        actors = [ac.actor for ac in T.team(A).actors]
        critics = [m.critic for m in D.critics(C_, 7300 + A)]
    else:
        import test_cnn_sized_team_step_gpu as G
        flat, M = 16 * P * P, G._side(P)
        actors = [ac.actor for ac in _sized_actors(P, A, M)]
        critics = [m.critic for m in D.critics(C_, 7400 + P, M)]
    g = torch.Generator().manual_seed(3000 + flat + 10 * A + C_)
    sparse = lambda rows: (torch.rand(rows, N, flat, generator=g) * A2_SCALE * (torch.rand(rows, N, flat, generator=g) < A2_DENSITY)).contiguous()
    return dict(actors=actors, critics=critics, a2a=sparse(A), a2c=sparse(C_), u=uniforms(A, g), flat=flat)


def cnn_head_inputs(A, a):
    torch = _torch()
    import _f64_ref as R
    c = R.head_case(N, A)
    g = torch.Generator().manual_seed(4000 + A)
    return dict(actor=c.actors[a].actor, critic=c.critics[a].critic, y1a=(c.y1a[a] * HEAD_Y1_SCALE).contiguous(),
                y1c=(c.y1c[a] * HEAD_Y1_SCALE).contiguous(), u=uniforms(A, g))


def ff_inputs(A):
    torch = _torch()
    import _f64_ref as R
    g = torch.Generator().manual_seed(5000 + A)
    return dict(agents=[R.ff_agent("x3", seed=a) for a in range(A)], x=torch.randn(N, A, 11, generator=g) * FF_X_SCALE, u=uniforms(A, g))


# ------------------------------------------------------------------------------------------------ the float64 draws, on the CPU
def reference_actions(case):
    """{entry point: float64 actions of the case's unmasked form} by the references of tests/_f64_ref.py"""
    torch = _torch()
    import _f64_ref as R
    family, c = CASES[case]
    with torch.no_grad():
        if family == "rnn":
            i = rnn_inputs(c["widths"], c["A"])
            acts = [R.draw_f64(R.f64(ac).policy_step(i["x"][:, a].double(), i["loc"][:, a].double(), i["h0"][a].double())[0], i["u"][:, a])[0]
                    for a, ac in enumerate(i["acs"])]
            team = torch.stack(acts)
            if c["widths"] is None:
                return {"rs_rnn_policy_step": acts[1], "rs_rnn_policy_step_rows": acts[1], "rs_rnn_team_step": team, "rs_rnn_team_eval_step": team}
            return {"rs_rnn_sized_step": acts[1], "rs_rnn_sized_team_step": team}
        if family == "cnn_head":
            i = cnn_head_inputs(c["A"], c["a"])
            return {"rs_cnn_head": R.draw_f64(R.cnn_head_f64(R.f64(i["actor"]), i["y1a"])[0], i["u"][:, c["a"]])[0]}
        if family == "cnn_team":
            i = cnn_team_inputs(c["P"], c["A"], c["C"])
            acts = []
            for a, seq in enumerate(i["actors"]):
                s64 = R.f64(seq)
                y1 = i["a2a"][a].double() @ s64[6].weight.t() + s64[6].bias
                acts.append(R.draw_f64(R.cnn_head_f64(s64, y1)[0], i["u"][:, a])[0])
            return {"rs_cnn_team_step_head" if c["P"] is None else "rs_cnn_sized_team_step_head": torch.stack(acts)}
        i = ff_inputs(c["A"])
        return {"rs_ff_team_step": torch.stack([R.draw_f64(R.ff_forward_f64(R.f64(ac), i["x"][:, a])[0], i["u"][:, a])[0]
                                                for a, ac in enumerate(i["agents"])])}


def reference_coverage():
    """{entry point: sorted actions the float64 references draw over its cases}"""
    seen = {}
    for case in CASES:
        for entry, act in reference_actions(case).items():
            seen.setdefault(entry, set()).update(int(v) for v in act.flatten().tolist())
    return {k: sorted(v) for k, v in seen.items()}


# ------------------------------------------------------------------------------------------------ the runs, on cuda:0
def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Out:
    """sentinel-filled outputs of one launch; off: the masked-out lanes (None in the nomask form)"""

    def __init__(self, prefix, off):
        self.prefix, self.off, self.got = prefix, off, {}

    def new(self, shape, dtype=None):
        torch = _torch()
        dtype = dtype or torch.float32
        mark = {torch.float32: F_MARK, torch.int64: ACT_MARK, torch.int8: ACT8_MARK}[dtype]
        return torch.full(shape, mark, dtype=dtype, device="cuda")

    def keep(self, name, t, lane_dim=None, start=None):
        """store t; lane_dim: the dimension of t that runs over the lanes (None: the mask does not govern this output); start: what the
        masked-out lanes must still hold (the sentinel when None)"""
        torch = _torch()
        torch.cuda.synchronize()
        if self.off is not None and lane_dim is not None:
            held = t.index_select(lane_dim, self.off)
            want = torch.full_like(held, {torch.float32: F_MARK, torch.int64: ACT_MARK, torch.int8: ACT8_MARK}[t.dtype]) if start is None \
                else start.index_select(lane_dim, self.off)
            assert held.numel() > 0 and torch.equal(held, want), (self.prefix, name, "a masked-out lane was written")
        self.got[f"{self.prefix}.{name}"] = t.detach().cpu().numpy().copy()


def _run_rnn(case, form, c):
    torch = _torch()
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.rada2c import pack_policy_weights, pack_sized_policy_weights
    lib = _lib.load()
    widths, A, a = c["widths"], c["A"], 1
    i = rnn_inputs(widths, A)
    hid = i["hid"]
    W = [(pack_policy_weights(ac.cuda()) if widths is None else pack_sized_policy_weights(ac.cuda())).contiguous() for ac in i["acs"]]
    wp = (C.c_void_p * A)(*[_p(w) for w in W])
    x, loc, h0, u = i["x"].cuda(), i["loc"].cuda(), i["h0"].cuda(), i["u"].cuda()
    m8 = mask_cpu().cuda() if form == "mask" else None
    off = (m8 == 0).nonzero().flatten() if form == "mask" else None
    got = {}
    xa, la, ua = _p(x) + 44 * a, _p(loc) + 8 * a, _p(u) + 4 * a

    # ---- one agent's rows of the [N][A][.] tensors
    if widths is None and form == "nomask":                          # rs_rnn_policy_step: packed rows, no mask argument
        o = _Out(f"{case}.{form}.rs_rnn_policy_step", None)
        xc, lc, uc = x[:, a].contiguous(), loc[:, a].contiguous(), u[:, a].contiguous()
        ho, lg, v, act, lp = o.new((N, hid)), o.new((N, 8)), o.new((N,)), o.new((N,), torch.int64), o.new((N,))
        _lib.check(lib.rs_rnn_policy_step(_p(W[a]), _p(xc), _p(lc), _p(h0[a]), _p(uc), _p(ho), _p(lg), _p(v), _p(act), _p(lp), N, _stream()),
                   "rs_rnn_policy_step")
        for k, t in (("h_out", ho), ("logits", lg), ("value", v), ("act", act), ("logp", lp)):
            o.keep(k, t)
        got.update(o.got)
    entry = "rs_rnn_policy_step_rows" if widths is None else "rs_rnn_sized_step"
    o = _Out(f"{case}.{form}.{entry}", off)
    ho, lg, v, act, lp, a8 = o.new((N, hid)), o.new((N, 8)), o.new((N,)), o.new((N,), torch.int64), o.new((N,)), o.new((N, A), torch.int8)
    if widths is None:
        _lib.check(lib.rs_rnn_policy_step_rows(_p(W[a]), xa, 11 * A, la, 2 * A, _p(h0[a]), ua, A, _p(ho), _p(v), _p(act), _p(lp), _p(a8), A,
                                               _p(m8), N, _stream()), entry)
    else:
        _lib.check(lib.rs_rnn_sized_step(_p(W[a]), *widths, xa, 11 * A, la, 2 * A, _p(h0[a]), ua, A, _p(ho), _p(lg), _p(v), _p(act), _p(lp),
                                         _p(a8), A, _p(m8), N, _stream()), entry)
        o.keep("logits", lg, 0)
    for k, t in (("h_out", ho), ("value", v), ("act", act), ("logp", lp), ("act8", a8)):
        o.keep(k, t, 0)
    got.update(o.got)

    # ---- the team's step round, then its bootstrap round on the states the step round left
    entry = "rs_rnn_team_step" if widths is None else "rs_rnn_sized_team_step"
    o = _Out(f"{case}.{form}.{entry}", off)
    h, act, f, a8 = h0.clone(), o.new((A, N), torch.int64), o.new((A, 3, N)), o.new((N, A), torch.int8)

    def team(u_, act_, a8_):
        tail = (_p(x), _p(loc), _p(h), _p(u_), _p(act_), _p(f), _p(a8_), _p(m8), N, _stream())
        _lib.check(lib.rs_rnn_team_step(wp, A, *tail) if widths is None else lib.rs_rnn_sized_team_step(wp, A, *widths, *tail), entry)

    team(u, act, a8)
    o.keep("h", h, 1, start=h0)
    o.keep("act", act, 1)
    o.keep("logp_val_boot", f, 2)
    o.keep("act8", a8, 0)
    h1 = hs = h.clone()
    team(None, None, None)
    o.keep("boot.logp_val_boot", f, 2)
    torch.cuda.synchronize()
    assert torch.equal(h, h1)                                         # the bootstrap round does not write h
    got.update(o.got)

    # ---- the evaluation's round (default widths: a kernel of its own)
    if widths is None:
        o = _Out(f"{case}.{form}.rs_rnn_team_eval_step", off)
        h, a8 = h0.clone(), o.new((N, A), torch.int8)
        active = m8 if m8 is not None else torch.ones(N, dtype=torch.uint8, device="cuda")
        _lib.check(lib.rs_rnn_team_eval_step(wp, A, _p(x), _p(loc), _p(h), _p(u), _p(active), _p(a8), N, _stream()), "rs_rnn_team_eval_step")
        o.keep("act8", a8, 0)
        assert torch.equal(h, hs)                                     # the step round's states, bit for bit: held by that member
        got.update(o.got)
    return got


def _run_cnn_head(case, form, c):
    torch = _torch()
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    A, a = c["A"], c["a"]
    i = cnn_head_inputs(A, a)
    m8 = mask_cpu().cuda() if form == "mask" else None
    off = (m8 == 0).nonzero().flatten() if form == "mask" else None
    o = _Out(f"{case}.{form}.rs_cnn_head", off)
    u = i["u"].cuda()
    for out_dim, seq, y1 in ((8, i["actor"], i["y1a"]), (1, i["critic"], i["y1c"])):
        s, y1 = copy.deepcopy(seq).cuda(), y1.cuda()                  # the case's modules are shared with other tests: left on the CPU
        w = (_p(s[8].weight), _p(s[8].bias), _p(s[10].weight), _p(s[10].bias))
        if out_dim == 8:
            act, lp, a8 = o.new((N,), torch.int64), o.new((N,)), o.new((N, A), torch.int8)
            _lib.check(lib.rs_cnn_head(_p(y1), *w, 8, _p(u) + 4 * a, A, _p(act), _p(lp), _p(a8) + a, A, None, 1, 0, _p(m8), N, _stream()), "rs_cnn_head")
            for k, t in (("act", act), ("logp", lp), ("act8", a8)):
                o.keep(k, t, 0)
        else:
            v = o.new((3, N))                                         # value_copies = 3 at a stride of N floats
            _lib.check(lib.rs_cnn_head(_p(y1), *w, 1, None, 1, None, None, None, 1, _p(v), 3, N, _p(m8), N, _stream()), "rs_cnn_head")
            o.keep("value", v, 1)
    return o.got


def _run_cnn_team(case, form, c):
    torch = _torch()
    from radiation_ppo_amd import _lib
    import _cnn_team_drive as D
    lib = _lib.load()
    P, A, nc = c["P"], c["A"], c["C"]
    i = cnn_team_inputs(P, A, nc)
    flat = i["flat"]
    actors, critics = [copy.deepcopy(s).cuda() for s in i["actors"]], [copy.deepcopy(s).cuda() for s in i["critics"]]   # shared teams stay on the CPU
    pa, pc = D.head_params(actors), D.head_params(critics)
    a2a, a2c, u = i["a2a"].cuda(), i["a2c"].cuda(), i["u"].cuda()
    mask = mask_cpu().cuda() if form == "mask" else None
    off = (mask == 0).nonzero().flatten() if form == "mask" else None
    entry = "rs_cnn_team_step_head" if P is None else "rs_cnn_sized_team_step_head"
    o = _Out(f"{case}.{form}.{entry}", off)
    if P is not None:
        need = lib.rs_cnn_sized_team_head_scratch_floats(flat, A + nc, N)
        assert need > 0
        scr = torch.full((need,), float("nan"), device="cuda")

    def head(boot, act, f, a8, y1, m):
        args = (None, A, pc, nc) if boot else (pa, A, pc, nc)
        mid = (None, _p(a2c), None, None, _p(f), None, _p(m), _p(y1)) if boot else (_p(a2a), _p(a2c), _p(u), _p(act), _p(f), _p(a8), _p(m), _p(y1))
        if P is None:
            _lib.check(lib.rs_cnn_team_step_head(*args, *mid, N, _stream()), entry)
        else:
            _lib.check(lib.rs_cnn_sized_team_step_head(*args, flat, *mid, _p(scr), need, N, _stream()), entry)

    act, f, a8, y1 = o.new((A, N), torch.int64), o.new((A, 3, N)), o.new((N, A), torch.int8), o.new((A + nc, N, 32))
    head(False, act, f, a8, y1, mask)
    for k, t, d in (("act", act, 1), ("logp_val_boot", f, 2), ("act8", a8, 0), ("y1_out", y1, 1)):
        o.keep(k, t, d)
    y1b = o.new((A + nc, N, 32))                                      # the bootstrap round (row0 = A) requires a mask: ones in the nomask form
    head(True, None, f, None, y1b, mask if mask is not None else torch.ones(N, dtype=torch.uint8, device="cuda"))
    o.keep("boot.logp_val_boot", f, 2)
    torch.cuda.synchronize()                                          # its y1: the step round's critic rows (held by y1_out) where live, nothing else
    want = o.new((A + nc, N, 32))
    live = torch.ones(N, dtype=torch.bool, device="cuda") if off is None else mask != 0
    want[A:, live] = y1[A:, live]
    assert torch.equal(y1b, want)
    return o.got


def _run_ff(case, form, c):
    torch = _torch()
    import test_ff_team_step_gpu as G
    A = c["A"]
    i = ff_inputs(A)
    gpu = [copy.deepcopy(ac).cuda() for ac in i["agents"]]
    x, u = i["x"].cuda(), i["u"].cuda()
    mask = mask_cpu().cuda() if form == "mask" else None
    off = (mask == 0).nonzero().flatten() if form == "mask" else None
    o = _Out(f"{case}.{form}.rs_ff_team_step", off)
    act, f, a8 = o.new((A, N), torch.int64), o.new((A, 3, N)), o.new((N, A), torch.int8)
    G._call(gpu, x, u, act, f, a8, mask)                              # the step round ignores the mask
    for k, t in (("act", act), ("logp_val_boot", f), ("act8", a8)):
        o.keep(k, t)
    if form == "mask":
        act0, f0, a80 = o.new((A, N), torch.int64), o.new((A, 3, N)), o.new((N, A), torch.int8)
        G._call(gpu, x, u, act0, f0, a80, None)
        assert torch.equal(act, act0) and torch.equal(f, f0) and torch.equal(a8, a80)
    fb = o.new((A, 3, N))
    G._call(gpu, x, None, None, fb, None, mask)
    o.keep("boot.logp_val_boot", fb, 2)
    return o.got


RUNNERS = {"rnn": _run_rnn, "cnn_head": _run_cnn_head, "cnn_team": _run_cnn_team, "ff": _run_ff}


def run(case):
    """{member: array} of one case on cuda:0, both forms"""
    family, c = CASES[case]
    got = {}
    for form in FORMS:
        got.update(RUNNERS[family](case, form, c))
    return got


def actions_drawn(members):
    """{entry point: sorted actions in its members, sentinels left out}"""
    seen = {}
    for entry, tails in DRAWS.items():
        vals = set()
        for k, v in members.items():
            if k.endswith(tails):
                vals.update(int(x) for x in np.unique(v))
        seen[entry] = sorted(vals - {ACT_MARK, ACT8_MARK})
    return seen


def main():
    want = list(range(8))
    ref = reference_coverage()
    for entry in DRAWS:
        print("float64 reference", entry, ref.get(entry), flush=True)
        assert ref.get(entry) == want, entry
    if "--reference" in sys.argv:
        return
    out = {}
    for case in CASES:
        got = run(case)
        print(case, len(got), "members", sum(v.nbytes for v in got.values()), "bytes", flush=True)
        out.update(got)
    for entry, acts in actions_drawn(out).items():
        print("drawn", entry, acts, flush=True)
        assert acts == want, entry
    path = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = path[0] if path else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
