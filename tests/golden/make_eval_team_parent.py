"""Fixture of the three lane-per-run team evaluations -- run_test_environments_team (feed-forward), run_test_environments_cnn_team
(RAD-TEAM, 27 x 27 maps) and run_test_environments_cnn_team_sized (RAD-TEAM, square maps of side 8..256) -- recorded from commit
b23b3c5 ("RAD-TEAM (CNN) teams in training: three policy launches per round"), the commit BEFORE the three became fronts to one
lock-step loop (evaluate._run_lane_per_run_team).  At that commit each runner had its own copy of the loop; what the copies computed
is what the one loop must go on computing under each of the three policy rounds.

The agents, seeds and sets are those of the runners' own whole-run tests (tests/test_ff_eval_gpu.py, tests/test_cnn_team_eval_gpu.py,
tests/test_cnn_sized_team_eval_gpu.py: imported, not copied), where the fused and the composed log are known to agree.  Per case
  <case>.fused.*       fused=True: the records and, where the case keeps one, the int8 action log
  <case>.composed.*    fused=False: the same
The records are every field of the List[MonteCarloResults], see make_rnn_eval_parent.encode(); returns are stored as float32 bits.
Only the three public runners are called, so the recorder runs on the parent's tree and on every later one.

    python tests/golden/make_eval_team_parent.py [OUT.npz]   # on the MI355X; on a later tree it must reproduce the committed file
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
OUT = os.path.join(HERE, "eval_team_parent.npz")

# case: (family, what differs from the family's base case)
CASES = {
    # feed-forward, E = 4, R = 3, L = 30: one agent without obstructions; three agents on the team reward with two
    "ff-A1-individual-obst0": ("ff", dict(A=1, team_mode="individual", obst=0, sets=77, seed=123)),
    "ff-A3-team-obst2": ("ff", dict(A=3, team_mode="team", obst=2, sets=11, seed=321)),
    "ff-A3-team-obst2-nolog": ("ff", dict(A=3, team_mode="team", obst=2, sets=11, seed=321, log=False)),     # the fixed act8 buffer
    # RAD-TEAM at 27 x 27, E = 4, R = 3, L = 30, 2 obstructions; without the predictor bank; every lane over at lock-step 1
    "cnn27-A2-individual": ("cnn27", dict(team_mode="individual")),
    "cnn27-A2-team": ("cnn27", dict(team_mode="team")),
    "cnn27-A2-nopredictor": ("cnn27", dict(variant="nopredictor")),
    "cnn27-A1-earlystop": ("cnn27", dict(variant="earlystop")),
    # RAD-TEAM sized, walls off, L = 8 (35 x 35 maps), 2 obstructions: one chunk; 132 lanes in chunks of 64, 64 and 4; 27 x 27 maps
    "sized-A2-team": ("sized", dict(team_mode="team", R=3)),
    "sized-A2-chunks": ("sized", dict(team_mode="individual", R=33, a2_bytes=1)),
    "sized-A2-side27": ("sized", dict(team_mode="individual", R=3, side=27)),
}


def _maker(module_name):
    """a sibling recorder as a module (tests/_k7_bits.maker)"""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import _k7_bits
    return _k7_bits.maker(module_name)


def _call(case):
    """(runner, agents, sets, keyword arguments) of one case"""
    for d in (ROOT, TESTS):
        if d not in sys.path:
            sys.path.insert(0, d)
    from radiation_ppo_amd import evaluate as ev
    family, c = CASES[case]
    if family == "ff":
        import test_ff_eval_gpu as T
        sets = ev.sample_test_environments(4, obstruction_count=c["obst"], seed=c["sets"])
        kw = dict(montecarlo_runs=3, steps_per_episode=30, team_mode=c["team_mode"], obstruction_count=c["obst"], seed=c["seed"],
                  return_actions=c.get("log", True))
        return ev.run_test_environments_team, T._team(c["A"]), sets, kw
    if family == "cnn27":
        import test_cnn_team_eval_gpu as T
        if c.get("variant") == "nopredictor":                      # test_the_runner_without_predictor_and_its_refusals
            sets = ev.sample_test_environments(2, obstruction_count=0, seed=8)
            kw = dict(montecarlo_runs=2, steps_per_episode=6, seed=3, use_predictor=False, return_actions=True)
            return ev.run_test_environments_cnn_team, T._agents(2, 12), sets, kw
        if c.get("variant") == "earlystop":                        # test_the_run_stops_on_the_device_side_count_at_the_next_sixteenth_step
            sets = {f"env_{i}": (np.array([1350.0, 1350.0]), np.array([1353.0, 1354.0]), 2_000_000 + 1000 * i, 20 + i) for i in range(3)}
            kw = dict(montecarlo_runs=4, steps_per_episode=40, seed=5, return_actions=True)
            return ev.run_test_environments_cnn_team, T._agents(1, 11), sets, kw
        sets = ev.sample_test_environments(4, obstruction_count=2, seed=T.RUN_SEEDS["sets"])
        kw = dict(montecarlo_runs=3, steps_per_episode=30, team_mode=c["team_mode"], obstruction_count=2, seed=T.RUN_SEEDS["run"],
                  return_actions=True)
        return ev.run_test_environments_cnn_team, T._agents(2, T.RUN_SEEDS["torch"], T.RUN_SCALE), sets, kw
    import test_cnn_sized_team_eval_gpu as T
    walls = "side" in c                                            # 27 x 27 maps: walls on, the environment's own spawn rules
    sets = ev.sample_test_environments(4, obstruction_count=2, seed=T.RUN_SEEDS["sets"]) if walls else T._sets(4, 2, T.RUN_SEEDS["sets"])
    kw = dict(montecarlo_runs=c["R"], steps_per_episode=T.L_RUN, team_mode=c["team_mode"], obstruction_count=2,
              enforce_grid_boundaries=walls, seed=T.RUN_SEEDS["run"], return_actions=True)
    if "a2_bytes" in c:
        kw["a2_bytes"] = c["a2_bytes"]
    return ev.run_test_environments_cnn_team_sized, T._agents(2, T.RUN_SEEDS["torch"], side=c.get("side", 35)), sets, kw


def run(case):
    """{member: array} of one case on cuda:0, fused and composed"""
    encode = _maker("make_rnn_eval_parent").encode
    runner, agents, sets, kw = _call(case)
    got = {}
    for form, fused in (("fused", True), ("composed", False)):
        res = runner(agents, sets, fused=fused, **kw)
        log = res[2] if kw["return_actions"] else None
        assert log is None or log.dtype == np.int8
        got.update({f"{case}.{form}.{k}": v for k, v in encode(res[0], log).items()})
    return got


def main():
    out = {}
    for case in CASES:
        got = run(case)
        log = got.get(f"{case}.fused.log")
        print(case, "lock-steps", None if log is None else log.shape[0], "successes", int(got[f"{case}.fused.success_counter"].sum()),
              "of", int(got[f"{case}.fused.completed_runs"].sum()), flush=True)
        out.update(got)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
