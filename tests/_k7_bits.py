"""What the bit-identity suites of K7 and K6 share (tests/golden/make_*_bits.py record a fixture, tests/test_k7_*_gpu.py and
tests/test_k6_chain_bits_gpu.py replay it): the seeded input generators, one run() of the library on a path, and the helpers that
store and compare raw words.  What a suite does differently is an argument of run(); its cases and inputs() stay in its recorder.

numpy only at import: test modules build their case tables from here at collection time, without a GPU.  torch and the package are
imported inside the functions that run on the device.

A new suite: a recorder with CASES, inputs() and a main() that calls run() and record(); a test that compares run() with expected()
through same_bits()."""
import contextlib
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CLIP, ALPHA, VF = 0.2, 0.01, 0.01
ACTOR_PARAMS = 5448           # the critic's 4993 gradients lie behind the actor's in the bucket
N_PARAMS = 10441
BUCKET = N_PARAMS + 16        # RS_PPO_GRAD_FLOATS: the gradients and the (hi, lo) statistics tail
STAT_VALUE_LOSS = 3
PARAM_NAMES = ("aw1", "ab1", "aw2", "ab2", "aw3", "ab3", "cw1", "cb1", "cw2", "cb2", "cw3", "cb3")
BATCH_NAMES = ("x", "act", "adv", "ret", "lpo", "w")
PATHS = ("grad", "pair", "split")
SPLIT_ENV = "RS_PPO_SPLIT_GRAD"


def params(seed: int):
    """FF_core parameters (actor then critic, nn.Linear order) as float32 numpy arrays, uniform(+-1/sqrt(fan_in)) like torch's init."""
    rng = np.random.default_rng(seed)
    out = []
    for nout in (8, 1):
        for fi, fo in ((11, 64), (64, 64), (64, nout)):
            b = 1.0 / np.sqrt(fi)
            out.append(rng.uniform(-b, b, (fo, fi)).astype(np.float32))
            out.append(rng.uniform(-b, b, (fo,)).astype(np.float32))
    return out


def batch(M: int, seed: int):
    """X, act, adv, ret, logp_old, w.  logp_old scatters around log(1/8) so that the ratios fall on both sides of the clip
    interval; the weights are non-uniform."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((M, 11)).astype(np.float32)
    act = rng.integers(0, 8, M).astype(np.int64)
    adv = rng.standard_normal(M).astype(np.float32)
    ret = rng.standard_normal(M).astype(np.float32)
    lpo = (np.log(0.125) + 0.4 * rng.standard_normal(M)).astype(np.float32)
    w = (rng.uniform(0.25, 1.75, M) / M).astype(np.float32)
    return X, act, adv, ret, lpo, w


def device_batch(bv):
    import torch
    return [torch.from_numpy(a).cuda() for a in bv]


def load(pv, begin: bool = False):
    """(ac, its parameters in the C ABI's order, f): an FFActorCritic on cuda:0 that holds the twelve arrays pv, and its FusedPPOGrad
    with bucket and statistics filled with 7.0 (the stop path must overwrite these).  begin: begin_update() before the fill."""
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from radiation_ppo_amd.ppo import FFActorCritic, FusedPPOGrad
    ac = FFActorCritic().cuda()
    ps = [ac.actor[0].weight, ac.actor[0].bias, ac.actor[2].weight, ac.actor[2].bias, ac.actor[4].weight, ac.actor[4].bias,
          ac.critic[0].weight, ac.critic[0].bias, ac.critic[2].weight, ac.critic[2].bias, ac.critic[4].weight, ac.critic[4].bias]
    with torch.no_grad():
        for p, v in zip(ps, pv):
            p.copy_(torch.from_numpy(v))
    f = FusedPPOGrad(ac)
    if begin:
        f.begin_update()
    f.bucket.fill_(7.0)
    f.stats.fill_(7.0)
    return ac, ps, f


@contextlib.contextmanager
def split_grad(path: str):
    """the launch form of rs_ppo_update_step: RS_PPO_SPLIT_GRAD is removed, set for path "split", and the caller's value put back"""
    old = os.environ.pop(SPLIT_ENV, None)
    if path == "split":
        os.environ[SPLIT_ENV] = "1"
    try:
        yield
    finally:
        os.environ.pop(SPLIT_ENV, None)
        if old is not None:
            os.environ[SPLIT_ENV] = old


def read_back(ps, f, step: bool = True):
    """{kind: float array}: g the whole bucket [10457], s the statistics float64 [5] and, after an update step, p the flat parameters,
    m and v [10441] each"""
    out = {"g": f.bucket.cpu().numpy().copy(), "s": f.stats.cpu().numpy().copy()}
    if step:
        out.update(p=np.concatenate([p.detach().cpu().numpy().ravel() for p in ps]), m=f.m.cpu().numpy().copy(),
                   v=f.v.cpu().numpy().copy())
    return out


def run(pv, b, path: str, *, lr=None, stop: bool = False, begin="step", use_stop_flag: bool = False):
    """One call of the library on cuda:0 with the parameters pv and the device batch b (device_batch), read back by read_back().
    path: "grad" = rs_ppo_grad (leaves parameters and moments alone: g and s only), "pair" = rs_ppo_update_step (learning rate lr, no
    KL threshold) as the pair launch, "split" = the same as one launch per network.
    stop: rs_update_state.stopped is set after the sentinel fill; use_stop_flag: rs_ppo_grad is told to read it.
    begin: where an update step calls begin_update(), which clears stopped: "first" = before the fill and the stop flag, "step" =
    right before the step, None = nowhere."""
    import torch
    assert path in PATHS and begin in ("first", "step", None), (path, begin)
    ac, ps, f = load(pv, begin=(begin == "first"))
    if stop:
        f.state_i32[1] = 1
    with split_grad(path):
        if path == "grad":
            f(*b, CLIP, ALPHA, VF, use_stop_flag=use_stop_flag)
        else:
            if begin == "step":
                f.begin_update()
            f.step(*b, CLIP, ALPHA, VF, lr=lr, kl_threshold=1e30)
        torch.cuda.synchronize()
    assert SPLIT_ENV not in os.environ, "the split-launch setting leaked, or the suite was started with it set"
    return read_back(ps, f, step=(path != "grad"))


def digest(a):
    """SHA-256 of a's bytes as uint8 [32]"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def same_bits(got, want, what):
    """got and want, arrays of raw words, are equal in dtype, shape and every word; else: how many differ, where, and the first as hex"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), [hex(int(v)) for v in got.ravel()[bad[:4]]],
                           [hex(int(v)) for v in want.ravel()[bad[:4]]])


def _first(kind: str):
    return "grad" if kind in ("g", "s") else "pair"


def record(out, name: str, path: str, words):
    """store {kind: words} of one case and path in out: the first path's in full, a later path's only where it differs"""
    for kind, v in words.items():
        first = f"{kind}_{name}_{_first(kind)}"
        if first not in out:
            out[first] = v
        elif not np.array_equal(out[first], v):
            out[f"{kind}_{name}_{path}"] = v
            print("   ", name, path, kind, "differs from the first path in", int((out[first] != v).sum()), "words: stored on its own")


def expected(golden, name: str, path: str, kinds):
    """{kind: words} of one case and path: a path's own entry where the recorder found it to differ from the first path's.  Of
    kinds, "grad" has g and s only."""
    def pick(kind):
        key = f"{kind}_{name}_{path}"
        return golden[key] if key in golden.files else golden[f"{kind}_{name}_{_first(kind)}"]
    return {kind: pick(kind) for kind in kinds if path != "grad" or _first(kind) == "grad"}


def maker(module_name: str):
    """the recorder tests/golden/<module_name>.py as a module"""
    spec = importlib.util.spec_from_file_location(module_name, os.path.join(HERE, "golden", module_name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden(file_name: str):
    return np.load(os.path.join(HERE, "golden", file_name))


def torch_batch(M: int, seed: int):
    """the batch of the two A-against-B tests, drawn on the device: X, act, adv, ret, logp_old, w (normalised)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(M, 11, device="cuda", generator=g)
    act = torch.randint(0, 8, (M,), device="cuda", generator=g)
    adv = torch.randn(M, device="cuda", generator=g)
    ret = torch.randn(M, device="cuda", generator=g)
    lpo = -2.0 + 0.1 * torch.randn(M, device="cuda", generator=g)
    w = torch.rand(M, device="cuda", generator=g)
    return X, act, adv, ret, lpo, w / w.sum()


def state_bytes(f):
    """{name: uint8 tensor}: everything a FusedPPOGrad and its network hold after a call"""
    import torch
    torch.cuda.synchronize()
    out = {"bucket": f.bucket, "stats": f.stats, "m": f.m, "v": f.v, "state": f.state}
    out.update({f"param{i}": p.data for i, (p, _) in enumerate(f.views)})
    return {k: t.detach().cpu().contiguous().view(torch.uint8).clone() for k, t in out.items()}
