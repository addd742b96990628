"""The bootstrap particle filter and the RID-FIM controller without a GPU: the numpy restatement the GPU tests rely on
(tests/_bpf_ref.py) is held to what the reference's own classes computed on recorded draws (tests/golden/bpf_fic.npz, written by
tests/golden/make_bpf_fic.py from ParticleFilter, FIC and ssp of algos/test_environment/eval/core.py), the header and the derived
binding carry the new entries, and the runner refuses bad arguments before the library is loaded.

Every step of a recorded case is checked on its own, from the recorded state before it.  Exact: the resampling decision, ssp's
indices, the particles after the step (bit for bit), nEff, the action and the latch.  Under a bound: weights, estimates, J_fish and
J.  The bound is the first-order one for float64 sums taken in another order, computed here: a sum of n terms moves by at most
n * 2^-52 relative to the sum of its terms' magnitudes; for the Renyi sum that is e = (NP + 3 Z) * 2^-52 relative on each p_z and
p_za (NP particles, Z readings, the two logs and the product), carried through J = c sum_z p_z (log p_za - alpha log p_z) as
|dJ| <= |c| sum_z p_z (e |log p_za - alpha log p_z| + e + alpha e) (tests/_bpf_ref.py: renyi).  The restatement and the recording
share one math library, so the evaluation term of _bpf_ref (EVAL) is off here.

One difference from the reference is by rule: a reading z whose p_z underflows to 0 contributes 0 to J where the reference computes
0 * (-inf + inf) = nan.  The recording has such rows (J is nan there and np.argmax returns the first nan); on them the restatement
must be finite, and action and latch are not compared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _bpf_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "bpf_fic.npz"))
CASES = sorted({int(k[1:].split("_")[0]) for k in G.files if k.startswith("c")})
_p = G["params"]
P0 = dict(sigma_xy=_p[0], sigma_I=_p[1], alpha=_p[2], fim_thresh=_p[3], interval=(int(_p[4]), int(_p[5])), intensity=(_p[6], _p[7]),
          coord=(_p[8], _p[9]))


def _case(c):
    g = {k.split("_", 1)[1]: G[k] for k in G.files if k.startswith(f"c{c}_")}
    NP, thresh, bkg = g["meta"]
    return g, int(NP), dict(P0, thresh=thresh), bkg


def test_the_recording_has_the_cases():
    metas = {tuple(G[f"c{c}_meta"][:2]) for c in CASES}
    assert metas == {(64.0, 1.0), (64.0, 0.1), (100.0, 1.0), (100.0, 0.1)}
    readings = np.concatenate([G[f"c{c}_reading"] for c in CASES])
    assert (readings < 76).any() and (readings > 76).any()                                         # a short z window, and a full one
    assert any(((G[f"c{c}_cand"] == G[f"c{c}_det"][:, None, :]).all(axis=2)).any() for c in CASES)    # a move that stays where it is
    assert any(((G[f"c{c}_latch_before"] == 1) & (G[f"c{c}_latch_after"] == 0)).any() for c in CASES)  # a row that trips the latch
    res = np.concatenate([G[f"c{c}_resampled"] for c in CASES])
    assert res.any() and not res.all()
    assert all(len(G[f"c{c}_reading"]) == 6 for c in CASES)


@pytest.mark.parametrize("c", CASES)
def test_ssp_is_the_reference_s(c):
    g, NP, P, bkg = _case(c)
    for t in np.flatnonzero(g["resampled"]):
        idx, children = R.ssp(g["ssp_w"][t], g["resample_u"][t])
        assert idx is not None and children.sum() == NP and np.array_equal(idx, g["ssp_idx"][t]), (c, t)


@pytest.mark.parametrize("c", CASES)
def test_track_is_the_reference_s(c):
    g, NP, P, bkg = _case(c)
    for t in range(6):
        first = t == 0
        with np.errstate(divide="ignore"):
            xp0, lw0 = (None, np.zeros(NP)) if first else (g["xp"][t - 1], np.log(g["w"][t - 1]))
        o = R.track(xp0, lw0, g["reading"][t], g["det"][t], bkg, first, P, g["prior_u"][t], g["normals"][t], g["resample_u"][t])
        assert o["resampled"] == bool(g["resampled"][t]) and o["ok"], (c, t)
        if o["resampled"]:
            assert np.array_equal(o["idx"], g["ssp_idx"][t]), (c, t)
        assert np.array_equal(o["xp"].view(np.uint64), g["xp"][t].view(np.uint64)), (c, t)           # gathered particles, bit for bit
        assert o["neff"] == g["neff"][t], (c, t)
        e = R.eps_sum(NP)
        assert (np.abs(o["w"] - g["w"][t]) <= e * g["w"][t]).all(), (c, t, np.abs(o["w"] / g["w"][t] - 1).max())
        assert (np.abs(o["est"] - g["est"][t]) <= 2 * e * (g["w"][t][:, None] * np.abs(g["xp"][t])).sum(axis=0)).all(), (c, t)
        assert np.array_equal(np.isneginf(o["logw"]), g["w"][t] == 0)


@pytest.mark.parametrize("c", CASES)
def test_controller_is_the_reference_s(c):
    g, NP, P, bkg = _case(c)
    nan_rows = 0
    for t in range(6):
        latch = int(g["latch_before"][t])
        o = R.controller(g["xp"][t], g["w"][t], g["cand"][t], g["reading"][t], bkg, latch, P, eval_term=False)
        assert (np.abs(o["J_fish"] - g["J_fish"][t]) <= o["tolF"]).all(), (c, t)
        assert np.isfinite(o["J"]).all() and np.isfinite(o["tolJ"]).all()
        want = g["J_renyi"][t] if latch else g["J_fish"][t]
        ok = np.isfinite(want)
        print(f"case {c} step {t}: latch {latch}, max |dJ| {np.abs(o['J'] - want)[ok].max() if ok.any() else 0:.3e}, allowance {o['tolJ'].max():.3e}")
        assert (np.abs(o["J"] - want)[ok] <= o["tolJ"][ok]).all(), (c, t, o["J"] - want, o["tolJ"])
        same = (g["cand"][t][:, None, :] == g["cand"][t][None, :, :]).all(axis=2)
        assert all(o["J"][a].tobytes() == o["J"][b].tobytes() for a in range(8) for b in range(8) if same[a, b])     # same position, same bits
        if ok.all():
            assert o["act"] == g["act"][t] and o["latch"] == g["latch_after"][t], (c, t)
            assert o["act"] == min(a for a in range(8) if o["J"][a] == o["J"].max())                                 # ties: the lowest index
            assert abs(o["J_fish"][o["act"]] - g["score"][t]) <= o["tolF"][o["act"]]
        else:
            nan_rows += 1
    if c == 3:                                                     # latch still up where p_z underflows
        assert nan_rows > 0                                        # the rule about p_z == 0 is exercised by the recording


def test_an_empty_window_and_a_zero_weight():
    P = dict(P0, thresh=1.0)
    rng = np.random.default_rng(0)
    xp = np.column_stack([rng.uniform(100, 1000, 32), rng.uniform(0, 2500, (32, 2))])
    w = rng.dirichlet(np.ones(32))
    w[3] = 0.0
    o = R.controller(xp, w, np.array([1000.0, 1000.0]) + make_moves(), 0.0, 20.0, 1, dict(P, interval=(75, 1)))
    assert len(R.window(0.0, (75, 1))) == 0 and (o["J"] == 0).all() and o["act"] == 0 and o["latch"] == 1
    assert len(R.window(40.0, (75, 75))) == 114 and R.window(40.0, (75, 75))[0] == 1.0 and len(R.window(5000.0, (75, 75))) == 150


def make_moves():
    return np.array([(-100, 0), (-71, 71), (0, 100), (71, 71), (100, 0), (71, -71), (0, -100), (-71, -71)], dtype=np.float64)


def test_header_and_binding_carry_the_filter():
    from radiation_ppo_amd import _lib
    sym = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    v, pp, d = C.c_void_p, C.POINTER(C.c_void_p), C.c_double
    assert sym["rs_bpf_scratch_bytes"] == (C.c_size_t, [C.c_int32, C.c_int32])
    assert sym["rs_bpf_params_create"] == (C.c_int, [C.c_int32, d, d, d, v, v, d, d, v, pp])
    assert [a for _, a in _lib._functions["rs_bpf_params_create"][1]] == ["num_particles", "sigma_xy", "sigma_I", "thresh", "intensity", "coord",
                                                                          "alpha", "fim_thresh", "interval", "out"]
    assert sym["rs_bpf_state_create"] == (C.c_int, [C.c_int32] + [v] * 8 + [C.c_size_t, pp])
    assert sym["rs_bpf_params_destroy"] == (None, [v]) and sym["rs_bpf_state_destroy"] == (None, [v])
    assert sym["rs_bpf_track"] == (C.c_int, [v, v, v, v, v, C.c_int32, v])
    assert sym["rs_ridfim_eval_step"] == (C.c_int, [v] * 9)
    assert sym["rs_bpf_draws"] == (C.c_int, [v, C.c_int32, v, v, v, v])
    assert _lib._structs["rs_bpf_params"] is None and _lib._structs["rs_bpf_state"] is None          # opaque, like rs_handle
    assert _lib.RS_BPF_RESAMPLED == 1 and _lib.RS_BPF_ERR_SSP == 2 and _lib.RS_BPF_MAX_WINDOW == 1024
    text = open(_lib.HEADER_PATH).read()
    assert "core.py:554-591" in text and "core.py:703-764" in text and "contributes 0" in text and "bit-equal" in text
    dev = open(os.path.join(ROOT, "radiation_ppo_amd", "csrc", "rs_device.hpp")).read()
    assert "#define RS_STREAM_BPF 192u" in dev
    from radiation_ppo_amd import build
    assert "rs_bpf.hip" in build.SOURCES


def test_refusals_come_before_any_launch():
    from radiation_ppo_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    w = 4096                                                       # non-NULL stand-ins: every refusal comes before anything is touched
    bad = _lib.RS_ERR_INVALID_ARG
    assert lib.rs_bpf_scratch_bytes(0, 100) == 0 and lib.rs_bpf_scratch_bytes(3, 1) == 0
    assert lib.rs_bpf_scratch_bytes(3, 100) == 3 * 100 * (3 * 8 + 4)
    box, win = lambda a, b: (C.c_double * 2)(a, b), lambda a, b: (C.c_int32 * 2)(a, b)
    good = dict(NP=64, sxy=15.0, sI=1.0, thresh=1.0, inten=box(1e2, 1e3), coord=box(0.0, 25e2), alpha=0.6, fim=0.36, win=win(75, 75))

    def create(**kw):
        a, out = dict(good, **kw), C.c_void_p()
        rc = lib.rs_bpf_params_create(a["NP"], a["sxy"], a["sI"], a["thresh"], a["inten"], a["coord"], a["alpha"], a["fim"], a["win"], C.byref(out))
        return rc, out
    rc, prm = create()
    assert rc == 0 and prm.value
    for kw in (dict(NP=1), dict(sxy=-1.0), dict(sI=-1.0), dict(thresh=-0.5), dict(inten=box(2.0, 1.0)), dict(coord=box(5.0, 1.0)), dict(alpha=1.0),
               dict(alpha=float("nan")), dict(win=win(600, 600)), dict(win=win(-1, 5)), dict(inten=None), dict(win=None)):
        rc, out = create(**kw)
        assert rc == bad and not out.value, kw
    st = C.c_void_p()
    assert lib.rs_bpf_state_create(0, w, w, w, w, w, w, w, w, 1 << 20, C.byref(st)) == bad
    assert lib.rs_bpf_state_create(1, w, w, None, w, w, w, w, w, 1 << 20, C.byref(st)) == bad and not st.value
    assert lib.rs_bpf_state_create(1, w, w, w, w, w, w, w, w, 1 << 20, C.byref(st)) == 0 and st.value
    assert lib.rs_bpf_track(None, prm, st, w, w, 1, None) == bad
    assert lib.rs_bpf_track(w, None, st, w, w, 1, None) == bad and lib.rs_bpf_track(w, prm, None, w, w, 1, None) == bad
    assert lib.rs_ridfim_eval_step(None, prm, st, w, w, w, None, None, None) == bad
    assert lib.rs_bpf_draws(None, 64, w, w, w, None) == bad
    lib.rs_bpf_params_destroy(prm)
    lib.rs_bpf_state_destroy(st)
    lib.rs_bpf_params_destroy(None)
    lib.rs_bpf_state_destroy(None)


def test_the_runner_refuses_before_the_library_loads(monkeypatch):
    from radiation_ppo_amd import _lib, evaluate

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    sets = {"env_0": (np.array([500.0, 500.0]), np.array([1500.0, 1500.0]), 1000000, 20)}
    for kw in (dict(number_of_agents=0), dict(number_of_agents=9), dict(device="cpu"), dict(nParticles=1), dict(lanes_per_pass=0),
               dict(lanes_per_pass=99, montecarlo_runs=100)):          # a pass runs whole environments
        with pytest.raises(ValueError):
            evaluate.run_test_environments_rid_fim(sets, **kw)


def test_evaluate_ppo_takes_rid_fim_without_a_model(monkeypatch):
    from radiation_ppo_amd import evaluate, testsets
    seen = {}
    sets = {f"env_{i}": (np.array([500.0, 500.0]), np.array([1500.0, 1500.0]), 1000000, 20) for i in range(5)}
    monkeypatch.setattr(testsets, "load_test_environments", lambda path: sets)

    def runner(env_sets, **kw):
        seen.update(kw, n=len(env_sets))
        return [], {"success_rate": 0.0}
    monkeypatch.setattr(evaluate, "run_test_environments_rid_fim", runner)
    ev = evaluate.evaluate_PPO(dict(test_env_path="nowhere", obstruction_count=0, episodes=3, montecarlo_runs=2, nParticles=500,
                                    actor_critic_architecture="rid-fim", number_of_agents=2, steps_per_episode=7, seed=3))
    assert ev.evaluate() == ([], {"success_rate": 0.0})
    assert seen["n"] == 3 and seen["nParticles"] == 500 and seen["number_of_agents"] == 2 and seen["montecarlo_runs"] == 2
    assert seen["steps_per_episode"] == 7 and seen["team_mode"] == "individual" and "model_path" not in seen and "alpha" not in seen


def test_the_filter_s_defaults_are_the_reference_s():
    import inspect
    from radiation_ppo_amd.bpf import BootstrapParticleFilter
    d = {k: v.default for k, v in inspect.signature(BootstrapParticleFilter.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(nParticles=6000, noise_params=(15.0, 1.0, 1.0), thresh=1.0, intensity=(1e2, 1e3), coord=(0.0, 25e2), alpha=0.6,
                     fim_thresh=0.36, interval=(75, 75))
