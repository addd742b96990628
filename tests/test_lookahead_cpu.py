"""The look-ahead (rs_peek) and the gradient-search controller (rs_gs_eval_step) without a GPU: the plain-Python reference the GPU
tests rely on (tests/_lookahead_ref.py) is held to the pinned oracle's own step and to the reference controller's recorded
arithmetic (tests/golden/grad_search.npz, written by tests/golden/make_grad_search.py from the reference's GradSearch), the header
and the derived binding carry the two entries, and evaluate_PPO takes 'gs' without a model_path."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle.radsearch_oracle import PhiloxDraws, RadSearchOracle

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as F  # noqa: E402
import _lookahead_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("A", [1, 2, 8])
@pytest.mark.parametrize("enforce", [True, False])
@pytest.mark.parametrize("obst", [0, 3, 7])
def test_reference_lookahead_is_the_oracle_s_own_step(obst, enforce, A):
    """For every move k the oracle, deep-copied, takes its int form step(k) (no collision rule): each agent's position, whether it
    moved and, where it moved, the rate of its measurement equal the look-ahead's values exactly -- on sampled layouts, after random
    joint moves, and from saved starts beside a wall, on an obstruction's edge and corner and one step from the source."""
    rng = np.random.default_rng(100 * obst + 10 * A + int(enforce))
    moved_seen = blocked_seen = 0
    for env_id in range(3):
        env = RadSearchOracle(PhiloxDraws(77, env_id), number_agents=A, obstruction_count=obst, enforce_grid_boundaries=enforce)
        starts = [None, None, None]
        r0 = env.rects[0] if env.rects else None
        if r0 is not None:                                         # on the first rectangle's left edge, and on its corner
            starts += [(r0[0], (r0[1] + r0[3]) // 2), (r0[0], r0[1])]
        starts += [(0, 0) if enforce else (2699, 2699), (env.src[0] + 100, env.src[1])]
        for start in starts:
            if start is None:
                env.step({a: int(rng.integers(0, 8)) for a in range(A)})
            else:
                env.refresh_environment(env.src, start, env.intensity, env.bkg_intensity)
            xy, moved, lam, _ = R.peek(env)
            for k in range(8):
                for a, (pos, mv, last_lam) in enumerate(R.step_candidate(env, k)):
                    assert tuple(xy[a, k]) == tuple(pos) and bool(moved[a, k]) == mv, (env_id, start, k, a)
                    if mv:
                        assert lam[a, k] == last_lam, (env_id, start, k, a)
                    moved_seen += int(mv)
                    blocked_seen += int(not mv)
    assert moved_seen > 0 and (blocked_seen > 0 or not (enforce or obst))


def test_reference_lookahead_leaves_the_oracle_alone():
    import copy
    env = RadSearchOracle(PhiloxDraws(5, 3), number_agents=2, obstruction_count=3, enforce_grid_boundaries=True)
    env.refresh_environment(env.src, (env.src[0] + 100, env.src[1]), env.intensity, env.bkg_intensity)      # move 0 lands on the source
    before = copy.deepcopy(env)
    R.peek(env)
    assert env.err == before.err and env.t == before.t and env.iter_count == before.iter_count
    for a in range(2):
        assert vars(env.agents[a]) == vars(before.agents[a])


# softmax of 8 float32 terms against float64, relative to each probability: expf 2 ulp, the 8-term sum up to 8 u, the division and the
# store 1 u each, and the rounding of the exponent's argument, u |x - max|, with |x - max| <= 104 (beyond it float32's exp is 0): 120 u.
# tiny: a probability in float32's subnormal range (or flushed to 0) is off by up to 2^-126.
SOFTMAX_RTOL, SOFTMAX_TINY = 120 * F.U, 2.0 ** -126


def test_controller_arithmetic_is_the_reference_s():
    """GradSearch.step's float32 `grad` tensor, bit for bit, and softmax(grad) under the float64 tolerance rule, on the rows the
    reference's own class produced: plain rows, rows with blocked moves, q in {0.5, 1, 4}, saturated rows (1e4 counts)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "grad_search.npz"))
    q, cur, cand, grad, probs = (g[k] for k in ("q", "cur", "cand", "grad", "probs"))
    assert grad.dtype == np.float32 and probs.dtype == np.float32 and set(q.tolist()) == {0.5, 1.0, 4.0}
    moved = (cand[:, :, 1:3] != cur[:, None, 1:3]).any(axis=2)                 # core.py:641
    assert (~moved).any() and (~moved).all(axis=1).any() and np.abs(cand[:, :, 0] - cur[:, None, 0]).max() == 10000.0
    for i in range(len(q)):
        mine = R.gradient(cur[i, 0], cand[i, :, 0], moved[i], float(q[i]))
        assert mine.dtype == np.float32 and np.array_equal(mine.view(np.uint32), grad[i].view(np.uint32)), (i, mine, grad[i])
        _, p64, cdf = R.draw(mine, np.float32(0.5))
        F.close(torch.from_numpy(probs[i]), torch.from_numpy(p64), f"softmax row {i}", rtol=SOFTMAX_RTOL, noise=0.0, tiny=SOFTMAX_TINY)
        assert abs(cdf[-1] - 1.0) < 1e-12
    assert np.abs(grad).max() >= 100.0                                         # the saturated rows are there


def test_reference_draw_is_the_inverse_cdf():
    g = np.array([[0.0] * 8, [5.0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.float32)
    act, p, cdf = R.draw(g, np.array([0.55, 0.999999], dtype=np.float32))
    assert act.tolist() == [4, 7] and abs(p[0, 0] - 0.125) < 1e-15
    assert R.near_edge(cdf, np.array([0.5, 0.3], dtype=np.float32)).tolist() == [True, False]


def test_header_and_binding_carry_the_lookahead():
    import ctypes as C
    from radiation_ppo_amd import _lib
    sym = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert sym["rs_peek"] == (C.c_int, [C.c_void_p] * 7)
    assert sym["rs_gs_eval_step"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    assert [a for _, a in _lib._functions["rs_peek"][1]] == ["h", "from_xy", "xy", "moved", "lam", "meas", "stream"]
    assert _lib.RS_ABI_VERSION == 4
    assert list(sym)[-2:] == ["rs_peek", "rs_gs_eval_step"]                    # appended: what was declared before keeps its place


def test_refusals_come_before_any_launch():
    from radiation_ppo_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    w = 4096                                                                   # non-NULL stand-ins: every refusal comes before anything is touched
    assert lib.rs_peek(None, None, w, w, w, w, None) == _lib.RS_ERR_INVALID_ARG
    assert lib.rs_gs_eval_step(None, w, 1.0, w, w, w, None, None) == _lib.RS_ERR_INVALID_ARG


def test_evaluate_ppo_takes_gs_without_a_model(monkeypatch):
    from radiation_ppo_amd import evaluate, testsets
    seen = {}
    sets = {f"env_{i}": (np.array([500.0, 500.0]), np.array([1500.0, 1500.0]), 1000000, 20) for i in range(5)}
    monkeypatch.setattr(testsets, "load_test_environments", lambda path: sets)

    def runner(env_sets, **kw):
        seen.update(kw, n=len(env_sets))
        return [], {"success_rate": 0.0}
    monkeypatch.setattr(evaluate, "run_test_environments_gradient_search", runner)
    ev = evaluate.evaluate_PPO(dict(test_env_path="nowhere", obstruction_count=0, episodes=3, montecarlo_runs=2,
                                    actor_critic_architecture="gs", number_of_agents=2, steps_per_episode=7, q=4.0, seed=3))
    assert ev.evaluate() == ([], {"success_rate": 0.0})                         # no model_path among the eval_kwargs
    assert seen["n"] == 3 and seen["q"] == 4.0 and seen["number_of_agents"] == 2 and seen["montecarlo_runs"] == 2
    assert seen["steps_per_episode"] == 7 and seen["team_mode"] == "individual" and "model_path" not in seen
    seen.clear()
    evaluate.evaluate_PPO(dict(test_env_path="nowhere", obstruction_count=0, actor_critic_architecture="gs")).evaluate()
    assert seen["q"] == 1.0 and seen["number_of_agents"] == 1
    with pytest.raises(ValueError):
        evaluate.evaluate_PPO(dict(test_env_path="nowhere", obstruction_count=-1, actor_critic_architecture="gs"))
