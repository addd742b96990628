"""Fixture of the one-agent RAD-A2C evaluation, recorded from the commit BEFORE run_test_environments_rnn and the recurrent half of
run_test_environments became fronts to the team runner (evaluate.run_test_environments_rnn_team with one agent).  At that commit the
one-agent lock-step had its own fused loop, its own kernel pair and two composed loops; what they computed is what the team runner
must go on computing with A = 1.

For the eight (widths, carried hidden states, obstructions) cases of tests/test_rnn_eval_gpu.py, on the seeded agent of that file
(torch.manual_seed(9), policy parameters x 4) and 6 sampled environments x 4 runs x 30 steps:
  rnn_fused.<case>.*       run_test_environments_rnn(fused=True): the records and the int8 action log
  rnn_composed.<case>.*    run_test_environments_rnn(fused=False): the records
and for the two default-width cases with obstructions
  plain.<case>.*           run_test_environments(carry_hidden_across_runs=...): the records
The records are every field the tests' record comparison reads, see encode(); returns are stored as float32 bits.

    python tests/golden/make_rnn_eval_parent.py [OUT.npz]   # on the MI355X; on a later tree it must reproduce the committed file
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "rnn_eval_parent.npz")

E, R, L, SET_SEED = 6, 4, 30, 77
WIDTHS = {"default": None, "sized": dict(hidden=((32,),), hidden_sizes_pol=((64,),), hidden_sizes_val=((64,),), hidden_sizes_rec=(16,))}
# (widths, carried hidden states, obstructions): seed of the run -- SEEDS of tests/test_rnn_eval_gpu.py
CASES = {("default", True, 0): 321, ("default", True, 2): 20, ("default", False, 0): 321, ("default", False, 2): 5,
         ("sized", True, 0): 123, ("sized", True, 2): 321, ("sized", False, 0): 123, ("sized", False, 2): 321}
PLAIN = (("default", True, 2), ("default", False, 2))


def name(widths, carry, obst) -> str:
    return f"{widths}-{'carried' if carry else 'lane_per_run'}-obst{obst}"


def encode(results, log=None):
    """{field: array} of a runner's List[MonteCarloResults]: the scalars per environment, every list concatenated in environment
    order with its lengths in `counts`, returns as float32 bits; with a log, that too."""
    cat = lambda get, dt: np.array([v for r in results for v in get(r)], dtype=dt)
    out = {"id": np.array([r.id for r in results], dtype=np.int32),
           "completed_runs": np.array([r.completed_runs for r in results], dtype=np.int32),
           "success_counter": np.array([r.success_counter for r in results], dtype=np.int32),
           "total_episode_length": cat(lambda r: r.total_episode_length, np.int32),
           "counts": np.array([[len(r.total_episode_length)] + [len(getattr(b, k)) for b in (r.successful, r.unsuccessful)
                                                                 for k in ("episode_length", "episode_return", "intensity", "background_intensity")]
                               for r in results], dtype=np.int32)}
    for which in ("successful", "unsuccessful"):
        for k in ("episode_length", "intensity", "background_intensity"):
            out[f"{which}.{k}"] = cat(lambda r: getattr(getattr(r, which), k), np.int32)
        out[f"{which}.episode_return"] = cat(lambda r: getattr(getattr(r, which), "episode_return"), np.float32).view(np.uint32)
    if log is not None:
        out["log"] = np.ascontiguousarray(log)
    return out


def agent(widths):
    import torch
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    torch.manual_seed(9)
    ag = RNNAgentPPO(id=0, steps_per_episode=L, actor_critic_args=WIDTHS[widths])
    with torch.no_grad():
        for p in ag.agent.pi.parameters():
            p.mul_(4.0)
    return ag


def run(case):
    """{member: array} of one case on cuda:0"""
    sys.path.insert(0, ROOT)
    from radiation_ppo_amd.evaluate import run_test_environments, run_test_environments_rnn, sample_test_environments
    widths, carry, obst = case
    sets = sample_test_environments(E, obstruction_count=obst, seed=SET_SEED)
    kw = dict(montecarlo_runs=R, steps_per_episode=L, obstruction_count=obst, seed=CASES[case], carry_hidden_across_runs=carry)
    ag = agent(widths)
    res, _, log = run_test_environments_rnn(ag, sets, return_actions=True, fused=True, **kw)
    assert log.dtype == np.int8
    got = {f"rnn_fused.{name(*case)}.{k}": v for k, v in encode(res, log).items()}
    res, _ = run_test_environments_rnn(ag, sets, fused=False, **kw)
    got.update({f"rnn_composed.{name(*case)}.{k}": v for k, v in encode(res).items()})
    if case in PLAIN:
        res, _ = run_test_environments(ag, sets, **kw)
        got.update({f"plain.{name(*case)}.{k}": v for k, v in encode(res).items()})
    return got


def main():
    out = {}
    for case in CASES:
        got = run(case)
        pre = f"rnn_fused.{name(*case)}."
        print(name(*case), "lock-steps", got[pre + "log"].shape[0], "successes", int(got[pre + "success_counter"].sum()), "of", E * R, flush=True)
        out.update(got)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
