"""tests/_eval_runs.py, what the GPU suites of the evaluation runners trust, held to planted faults without a GPU.  Two hand-made
environments with two obstructions and two agents: env_0's detector starts 5 cm from its source (every run ends at step 1), env_1's
1343 cm away (no run can end within 12 steps of at most 100 cm against a terminal radius of 110 cm).  A log is made by walking the oracle
with seeded actions, lane per run and with the runs of an environment one after the other, and padded with 8; the records come from
radiation_ppo_amd.evaluate._collect_results on CPU tensors, the function that builds every runner's records.  The clean log and records
pass; each fault, planted alone, must raise AssertionError."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _eval_runs as V  # noqa: E402

A, R, L, SEED, OBST = 2, 3, 12, 5, 2
E, FAR = 2, 1 * R                                                   # FAR: the first lane (lane per run) of env_1
_box = lambda x0, y0, x1, y1: [np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]], dtype=np.float64)]
SETS = {"env_0": (np.array([1350.0, 1350.0]), np.array([1353.0, 1354.0]), 2_000_000, 20, [_box(2000, 2000, 2300, 2400), _box(600, 1900, 900, 2200)]),
        "env_1": (np.array([1350.0, 1350.0]), np.array([400.0, 400.0]), 2_001_000, 21, [_box(2000, 300, 2200, 700), _box(300, 1500, 700, 1700)])}


def _walk(carried):
    """(log [T, lanes, A] int8, ep_len [E * R], ep_ret [E * R], success [E * R]) of a walk of the oracle: agent a takes (d + 3 a) % 8
    for a seeded d in 0..7, so two agents on one spot never propose the same cell.  A lane is an (environment, run) pair, or with
    `carried` an environment whose R runs follow each other."""
    rng = np.random.default_rng(SEED)
    rows, ep_len, ep_ret, suc = [], [], [], []
    for lane in range(E if carried else E * R):
        ref, start = V.lane_oracle(SETS[f"env_{lane if carried else lane // R}"], SEED, lane, A, OBST, True)
        rows.append([])
        for _ in range(R if carried else 1):
            start()
            ret, steps, found = np.float32(0.0), 0, False
            while not found and steps < L:
                act = [(int(rng.integers(0, 8)) + 3 * a) % 8 for a in range(A)]
                rows[-1].append(act)
                _, rew, done, _ = ref.step(dict(enumerate(act)))
                ret, steps, found = np.float32(ret + np.float32(rew["individual_reward"][0])), steps + 1, any(done.values())
            ep_len.append(steps); ep_ret.append(ret); suc.append(found)
    log = np.full((max(len(r) for r in rows) + 2, len(rows), A), 8, dtype=np.int8)
    for n, r in enumerate(rows):
        log[:len(r), n] = r
    return log, np.array(ep_len, dtype=np.int32), np.array(ep_ret, dtype=np.float32), np.array(suc)


def _records(ep_len, ep_ret, suc):
    from radiation_ppo_amd.evaluate import _collect_results
    inten = torch.tensor([SETS[f"env_{n // R}"][2] for n in range(E * R)])
    bkg = torch.tensor([SETS[f"env_{n // R}"][3] for n in range(E * R)])
    return _collect_results(sorted(SETS), E, R, torch.from_numpy(ep_len), torch.from_numpy(ep_ret), torch.from_numpy(suc), inten, bkg)


def _replay(carried, log):
    return V.replay_carried(SETS, log, SEED, OBST, R, L) if carried else V.replay_lane_per_run(SETS, log, A, R, L, SEED, OBST)


def _membership_form(results, runs):
    """what the lane-per-run suites asserted before: a run's length and return are SOMEWHERE in its bucket"""
    for e, res in enumerate(results):
        for r in range(R):
            steps, found, ret = runs[e * R + r]
            assert res.total_episode_length[r] == steps
            bucket = res.successful if found else res.unsuccessful
            assert steps in bucket.episode_length
            assert any(abs(v - ret) < 1e-4 for v in bucket.episode_return)
    assert sum(r.success_counter for r in results) == sum(f for _, f, _ in runs)


@pytest.fixture(scope="module", params=[False, True], ids=["lane_per_run", "carried"])
def walk(request):
    return (request.param, *_walk(request.param))


def test_a_clean_log_and_its_records_pass(walk):
    carried, log, ep_len, ep_ret, suc = walk
    assert ep_len.tolist() == [1] * R + [L] * R and suc.tolist() == [True] * R + [False] * R       # both outcomes
    assert log.shape[1:] == ((E if carried else E * R), A) and (log[-2:] == 8).all()
    runs = _replay(carried, log)
    assert [(s, f) for s, f, _ in runs] == list(zip(ep_len.tolist(), suc.tolist()))
    assert V.check_records(_records(ep_len, ep_ret, suc), runs, R) == R
    if not carried:                                                  # a [lock-steps, lanes] log of one agent, without the idle rule
        one = np.where(log[:, :, 0] == 8, 3, log[:, :, 0]).astype(np.int64)
        assert len(V.replay_lane_per_run(SETS, one, 1, R, L, SEED, OBST, idle_rule=False)) == E * R
        with pytest.raises(AssertionError):
            V.replay_lane_per_run(SETS, one, 1, R, L, SEED, OBST)


def _return_moved(ep_len, ep_ret, suc):
    ep_ret[FAR + 1] += np.float32(1e-3)


def _runs_swapped(ep_len, ep_ret, suc):
    assert abs(ep_ret[FAR] - ep_ret[FAR + 2]) > 1e-3                 # the two runs are told apart by their returns
    for a in (ep_len, ep_ret, suc):
        a[[FAR, FAR + 2]] = a[[FAR + 2, FAR]]


def _flag_flipped(ep_len, ep_ret, suc):
    suc[1] = not suc[1]                                              # _collect_results then files the run in the other bucket


def _length_off_by_one(ep_len, ep_ret, suc):
    ep_len[FAR + 1] -= 1


RECORD_FAULTS = [_return_moved, _runs_swapped, _flag_flipped, _length_off_by_one]


@pytest.mark.parametrize("fault", RECORD_FAULTS, ids=[f.__name__[1:] for f in RECORD_FAULTS])
def test_a_fault_in_the_records_is_caught(walk, fault):
    carried, log, *arrays = walk
    runs = _replay(carried, log)
    arrays = [a.copy() for a in arrays]
    fault(*arrays)
    results = _records(*arrays)
    if fault is _runs_swapped:
        _membership_form(results, runs)                              # the old form lets swapped runs pass
    else:
        with pytest.raises(AssertionError):
            _membership_form(results, runs)                          # (the other faults it did see)
    with pytest.raises(AssertionError):
        V.check_records(results, runs, R)


def test_a_wrong_run_count_is_caught(walk):
    carried, log, *arrays = walk
    results = _records(*arrays)
    results[1].completed_runs = R + 1
    with pytest.raises(AssertionError):
        V.check_records(results, _replay(carried, log), R)
    with pytest.raises(AssertionError):
        V.check_records(_records(*arrays)[:1], _replay(carried, log), R)


@pytest.mark.parametrize("fault", ["action_after_the_end", "idle_before_the_end"])
def test_a_fault_in_the_idle_rows_is_caught(walk, fault):
    carried, log = walk[:2]
    log = log.copy()
    if fault == "action_after_the_end":
        log[(R if carried else 1) + 1, 0, 0] = 3                     # lane 0 (env_0) is over after R steps, or after 1
    else:
        log[5, -1] = 8                                               # the last lane (env_1) runs at least 12 steps
    with pytest.raises(AssertionError):
        _replay(carried, log)


def test_same_records_sees_every_field(walk):
    results = _records(*walk[2:])
    other = copy.deepcopy(results)
    V.same_records(results, other, R)
    other[1].unsuccessful.intensity[0] += 1
    old = lambda res: [(r.id, r.success_counter, r.total_episode_length, r.successful.episode_return, r.unsuccessful.episode_return) for r in res]
    assert old(results) == old(other)                                # the tuple form two suites used did not see it
    with pytest.raises(AssertionError):
        V.same_records(results, other, R)
    with pytest.raises(AssertionError):
        V.same_records(results, copy.deepcopy(results), R + 1)


def test_the_stop_rule_helper_holds_both_forms_to_sixteen_rows():
    """a stand-in runner whose every lane ends at lock-step 1; one that stops a row late in either form is caught"""
    from radiation_ppo_amd.evaluate import _collect_results
    Es, Rs = 3, 2
    n = Es * Rs

    def runner(late_form=None):
        def run(sets, fused):
            assert sorted(sets) == [f"env_{i}" for i in range(Es)] and sets["env_2"][2:] == (2_002_000, 22)
            log = np.full((17 if fused == late_form else 16, n, 1), 8, dtype=np.int8)
            log[0] = 4
            zero = torch.zeros(n, dtype=torch.int32)
            results = _collect_results(sorted(sets), Es, Rs, zero + 1, torch.zeros(n), torch.ones(n, dtype=torch.bool), zero, zero)
            return results, dict(completed_runs=n, success_rate=1.0), log
        return run

    V.check_stops_at_the_sixteenth(runner(), Es, Rs, 1)
    for late_form in (True, False):
        with pytest.raises(AssertionError):
            V.check_stops_at_the_sixteenth(runner(late_form), Es, Rs, 1)
