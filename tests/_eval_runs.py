"""What the GPU suites of the evaluation runners share (tests/test_evaluate_gpu.py, test_ff_eval_gpu.py, test_cnn_team_eval_gpu.py,
test_cnn_sized_team_eval_gpu.py, test_gs_eval_gpu.py, test_rnn_eval_gpu.py, test_rnn_team_eval_gpu.py): the replay of a run's action log
through the oracle, lane per run and with carried hidden states, the comparison of the records with the replayed runs IN RUN ORDER, of
the records of two runs with each other, and the stop rule of the lane-per-run loop.  numpy and the oracle only; its own test, with
planted faults and without a GPU: tests/test_eval_runs_cpu.py."""
import numpy as np

from oracle.radsearch_oracle import PhiloxDraws, RadSearchOracle


def rects(saved_env):
    """(min x, min y, max x, max y) of every obstruction of a saved environment; None where it has none"""
    if len(saved_env) < 5:
        return None
    return [(int(o[0][:, 0].min()), int(o[0][:, 1].min()), int(o[0][:, 0].max()), int(o[0][:, 1].max())) for o in saved_env[4]]


def near_sets(E):
    """The detector starts 5 cm from the source; a step moves at most 100 cm and the terminal radius is 110 cm, so a run ends with the
    first step in which an agent moves, whatever is drawn."""
    return {f"env_{i}": (np.array([1350.0, 1350.0]), np.array([1353.0, 1354.0]), 2_000_000 + 1000 * i, 20 + i) for i in range(E)}


def lane_oracle(saved_env, seed, lane, A, obst, walls):
    """the oracle on the draws of `lane`, and what starts a run of the saved environment on it (returns the first observation)"""
    ref = RadSearchOracle(PhiloxDraws(seed, lane), number_agents=A, obstruction_count=obst, enforce_grid_boundaries=walls)
    return ref, lambda: ref.refresh_environment(*saved_env[:4], rects(saved_env))


def replay_lane_per_run(sets, actions, A, R, L, seed, obst, team_mode="individual", enforce_grid_boundaries=True, idle_rule=True,
                        on_step=None):
    """A lane-per-run log, actions [lock-steps, E * R, A] (or [lock-steps, E * R] of one agent), replayed through the oracle: lane
    n = e * R + r is refresh_environment of env_e, then its logged rows; the run is over when any agent's flag rises or after L steps.
    The return is the float32 sum of individual_reward[0], or of team_reward.  idle_rule: the lane's rows are < 8 while it runs and 8
    (idle) from there on.  on_step(ref, obs, t, n) sees the oracle and its current observation before step t of lane n.
    Returns [(steps, found, return)] in lane order."""
    log = actions.reshape(actions.shape[0], actions.shape[1], -1)
    runs = []
    for e in range(len(sets)):
        for r in range(R):
            n = e * R + r
            ref, start = lane_oracle(sets[f"env_{e}"], seed, n, A, obst, enforce_grid_boundaries)
            obs = start()
            ret, steps, found = np.float32(0.0), 0, False
            while not found and steps < min(L, len(log)):
                if on_step is not None:
                    on_step(ref, obs, steps, n)
                obs, rew, done, _ = ref.step({a: int(log[steps, n, a]) for a in range(A)})
                ret = np.float32(ret + np.float32(rew["individual_reward"][0] if team_mode == "individual" else rew["team_reward"]))
                steps += 1
                found = any(done.values())
            if idle_rule:
                assert (log[:steps, n] < 8).all() and (log[steps:, n] == 8).all(), (e, r, steps)
            runs.append((steps, found, float(ret)))
    return runs


def replay_carried(sets, actions, seed, obst, R, L):
    """A carried-hidden log, actions [lock-steps, E, A]: lane e is refresh_environment of env_e, every agent's logged action, refresh
    again after a run ... -- R runs one after the other, returns from individual_reward[0].  An idle row (8) ends a lane's replay (the
    policy draws 0..7) and the lane idles from there to the end of the log.  Returns [(steps, found, return)] in (environment, run)
    order, as replay_lane_per_run."""
    A = actions.shape[2]
    runs = []
    for e in range(len(sets)):
        ref, start = lane_oracle(sets[f"env_{e}"], seed, e, A, obst, True)
        start()
        own, ret, steps, t = [], np.float32(0.0), 0, 0
        while t < len(actions) and actions[t, e, 0] != 8:
            _, rew, done, _ = ref.step({a: int(actions[t, e, a]) for a in range(A)})
            ret = np.float32(ret + np.float32(rew["individual_reward"][0]))
            steps, t = steps + 1, t + 1
            found = any(done.values())
            if found or steps == L:
                own.append((steps, found, float(ret)))
                ret, steps = np.float32(0.0), 0
                start()
        assert (actions[t:, e] == 8).all() and len(own) == R, (e, t, own)
        runs += own
    return runs


def check_records(results, runs, R):
    """The records against the replayed runs of either replay, per environment and in run order: id, completed_runs, every length,
    the success count, each bucket's lengths and its returns within 1e-4.  Returns the number of successful runs."""
    assert len(runs) == len(results) * R
    for e, res in enumerate(results):
        own = runs[e * R:(e + 1) * R]
        assert res.id == e and res.completed_runs == R, (e, res.id, res.completed_runs)
        assert res.total_episode_length == [steps for steps, _, _ in own], (e, own, res.total_episode_length)
        assert res.success_counter == sum(found for _, found, _ in own), (e, own, res.success_counter)
        for bucket, kind in ((res.successful, True), (res.unsuccessful, False)):
            lens, rets = [s for s, f, _ in own if f == kind], [r for _, f, r in own if f == kind]
            assert bucket.episode_length == lens, (e, kind, lens, bucket.episode_length)
            assert len(bucket.episode_return) == len(rets) and all(abs(v - r) < 1e-4 for v, r in zip(bucket.episode_return, rets)), \
                (e, kind, rets, bucket.episode_return)
    return sum(found for _, found, _ in runs)


def same_records(res_a, res_b, runs):
    """the records of two runs (fused and composed): every field equal"""
    assert len(res_a) == len(res_b)
    for a, b in zip(res_a, res_b):
        assert a.id == b.id and a.completed_runs == b.completed_runs == runs and a.success_counter == b.success_counter
        assert a.total_episode_length == b.total_episode_length
        for x, y in ((a.successful, b.successful), (a.unsuccessful, b.unsuccessful)):
            assert x.episode_length == y.episode_length and x.episode_return == y.episode_return
            assert x.intensity == y.intensity and x.background_intensity == y.background_intensity


def check_stops_at_the_sixteenth(run, E, R, A):
    """The stop rule of the lane-per-run loop on near_sets, for one agent (two agents on one spot that draw the same direction collide
    and neither moves): every lane ends at lock-step 1; the host reads the finished-lane count every 16 lock-steps, so the log has 16
    rows and rows 1..15 are idle, in both forms.  run(sets, fused) returns (results, summary, actions)."""
    sets = near_sets(E)
    for fused in (True, False):
        results, summary, actions = run(sets, fused)
        assert actions.shape == (16, E * R, A), (fused, actions.shape)
        assert (actions[0] < 8).all() and (actions[1:] == 8).all()
        assert summary["completed_runs"] == E * R and summary["success_rate"] == 1.0
        for res in results:
            assert res.success_counter == R and res.total_episode_length == [1] * R and res.successful.episode_length == [1] * R
            assert res.unsuccessful.episode_length == []
