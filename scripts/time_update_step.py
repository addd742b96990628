"""Fixed cost of one Adam step of the PPO update (K7 actor + K7 critic + what follows them) on synthetic batches.

Times, with HIP events on the launch stream, (a) the gradient pass alone (rs_ppo_grad, as scripts/time_k7.py) and (b) the whole
step as VecAgentPPO runs it (gradient pass + Adam + KL commit) at M, M/2 and M/4 samples, three runs of five rounds of 20 steps
each, medians.  Time per step is a straight line in M: the intercept of the least-squares line is what a step pays whatever the
batch (prologue and epilogue of the two K7 kernels, the launches behind them, the gaps in between).
RS_LIB_PATH selects another build; RS_PPO_SPLIT_TAIL=1 keeps the three-kernel tail in a build that has the fused one,
RS_PPO_SPLIT_GRAD=1 one gradient launch per network in a build that has the pair launch (whole step only)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from radiation_ppo_amd.ppo import FFActorCritic, FusedPPOGrad  # noqa: E402

M0 = int(sys.argv[1]) if len(sys.argv) > 1 else 4096 * 480
RUNS, ROUNDS, REPS = 3, 5, 20
LR, THR = 0.0, 1e30              # every step is taken (no KL stop), the parameters stay where they are


def batch(M):
    torch.manual_seed(0)
    X = torch.randn(M, 11, device="cuda")
    act = torch.randint(0, 8, (M,), device="cuda")
    adv, ret, lpo = torch.randn(M, device="cuda"), torch.randn(M, device="cuda"), -2.0 + 0.1 * torch.randn(M, device="cuda")
    return X, act, adv, ret, lpo, torch.full((M,), 1.0 / M, device="cuda")


def median_ms(fn):
    ts = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / REPS)
    return sorted(ts)[len(ts) // 2]


def fit(ms_by_m):
    """least-squares line through (M, ms): (intercept in us, slope in ns per sample)"""
    n = len(ms_by_m)
    xm = sum(m for m, _ in ms_by_m) / n
    ym = sum(t for _, t in ms_by_m) / n
    k = sum((m - xm) * (t - ym) for m, t in ms_by_m) / sum((m - xm) ** 2 for m, _ in ms_by_m)
    return (ym - k * xm) * 1e3, k * 1e6


torch.manual_seed(0)
ac = FFActorCritic().cuda()
f = FusedPPOGrad(ac)
fused = hasattr(f, "step") and not os.environ.get("RS_PPO_SPLIT_TAIL")
print(f"lib={os.environ.get('RS_LIB_PATH', 'default')}  grad={'one launch per network' if os.environ.get('RS_PPO_SPLIT_GRAD') else 'default'}  tail={'fused (one launch)' if fused else 'reduce + apply + commit (three launches)'}")
data = {M: batch(M) for M in (M0, M0 // 2, M0 // 4)}


def grad_only(b):
    f(*b, 0.2, 0.1)


def whole_step(b):
    if fused:
        f.step(*b, 0.2, 0.1, lr=LR, kl_threshold=THR)
    else:
        f(*b, 0.2, 0.1, use_stop_flag=True)
        f.adam_step(LR, THR)


for name, fn in (("grad pass", grad_only), ("whole step", whole_step)):
    for run in range(RUNS):
        pts = []
        for M, b in data.items():
            f.begin_update()
            for _ in range(5):
                fn(b)
            torch.cuda.synchronize()
            pts.append((M, median_ms(lambda: fn(b))))
        icpt, slope = fit(pts)
        print(f"{name:10s} run {run}: " + "  ".join(f"M={m}: {t:.4f} ms" for m, t in pts) + f"   intercept {icpt:7.1f} us  slope {slope:.4f} ns/sample")
