"""BPF-A2C and the Fisher analysis without a GPU: the numpy restatement the GPU tests rely on (tests/_bpf_a2c_ref.py), the host
recursion of the posterior Cramer-Rao bound (radiation_ppo_amd.bpf.pcrb) and the package's actor are held to what the reference's own
classes computed (tests/golden/bpf_a2c.npz, written by tests/golden/make_bpf_a2c.py from RNNModelActorCritic, ParticleFilter,
FIC.particle_FIM and StatBuff of algos/test_environment/eval/core.py); the header and the derived binding carry the two new entries,
and the runner refuses bad arguments before the library is loaded.

The restatement and the recording share numpy and one math library, so every entry of every matrix, its trace, the initial bound and
the recursion's B_t are held to 1e-12 relative, entry by entry.  The actor's normalised logits and hidden state are float32 torch
against float32 torch: rtol 1e-5, atol 1e-6, as tests/test_pfgru_golden.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _bpf_a2c_ref as R2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "bpf_a2c.npz"))
CASES = sorted({int(k[1:].split("_")[0]) for k in G.files if k.startswith("c")})
SIGMA_XY, SIGMA_I, I_LO, I_HI, C_LO, C_HI, AREA_MAX = G["params"]
NOISE = (SIGMA_XY, SIGMA_I, SIGMA_I)
REL = 1e-12


def _case(c):
    g = {k.split("_", 1)[1]: G[k] for k in G.files if k.startswith(f"c{c}_")}
    NP, thresh, bkg = g["meta"]
    return g, int(NP), bkg


def _close(got, want):
    return np.allclose(got, want, rtol=REL, atol=0.0)


def test_the_recording_has_the_cases():
    assert {tuple(G[f"c{c}_meta"][:2]) for c in CASES} == {(64.0, 1.0), (64.0, 0.1), (100.0, 1.0), (100.0, 0.1)}
    assert all(len(G[f"c{c}_reading"]) == 6 and G[f"c{c}_F_sim"].shape == (6, 8, 3, 3) for c in CASES)
    acts = np.concatenate([G[f"c{c}_act"] for c in CASES])
    assert len(set(acts.tolist())) >= 4                            # the walks turn
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "bpf_a2c.npz")) < 400 * 1024


@pytest.mark.parametrize("c", CASES)
def test_the_matrix_is_the_reference_s(c):
    g, NP, bkg = _case(c)
    for t in range(6):
        F, mag = R2.fim(g["xp"][t], g["w"][t], g["det"][t], bkg)
        assert _close(F, g["F_det"][t]) and _close(R2.trace(F), np.trace(g["F_det"][t])), (c, t, F - g["F_det"][t])
        assert (np.abs(F) <= mag).all() and not np.allclose(F, F.T)               # J @ scale scales columns
        for k in range(8):
            Fk, _ = R2.fim(g["xp"][t], g["w"][t], g["det"][t] + R2.ACTION[k], bkg)
            assert _close(Fk, g["F_sim"][t, k]) and _close(R2.trace(Fk), np.trace(g["F_sim"][t, k])), (c, t, k)


@pytest.mark.parametrize("c", CASES)
def test_the_initial_bound_and_the_recursion_are_the_reference_s(c):
    from radiation_ppo_amd.bpf import pcrb
    g, NP, bkg = _case(c)
    F0, _ = R2.fim_prior(g["xp_init"], g["det"][0], bkg, (I_LO, I_HI), (C_LO, C_HI))
    assert _close(F0, g["bound"][0]), (c, F0 / g["bound"][0] - 1)
    assert (g["xp_init"][:, 0] >= I_LO).all() and (g["xp_init"][:, 0] < I_HI).all() and (g["xp_init"][:, 1:] < C_HI).all()
    B = pcrb(g["bound"][0], g["F_det"][1:], NOISE)
    assert B.shape == (6, 3, 3) and _close(B, g["bound"]), (c, B / g["bound"] - 1)
    assert _close(R2.pcrb(g["bound"][0], g["F_det"][1:], NOISE), g["bound"])
    # batched over lanes, and nan from a lane's end on
    R = np.stack([g["F_det"][1:], g["F_det"][1:]], axis=1)
    R[3:, 1] = np.nan
    Bb = pcrb(np.stack([g["bound"][0]] * 2), R, NOISE)
    assert Bb.shape == (6, 2, 3, 3) and _close(Bb[:, 0], g["bound"]) and _close(Bb[:4, 1], g["bound"][:4]) and np.isnan(Bb[4:, 1]).all()


def _actor():
    from radiation_ppo_amd.rada2c import RNNModelActorCritic
    ac = RNNModelActorCritic()
    sd = ac.state_dict()
    sd.update({k[2:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("w_")})
    ac.load_state_dict(sd)
    assert ac.fused_policy
    return ac.eval()


@pytest.mark.parametrize("c", CASES)
def test_the_actor_on_the_filter_s_estimate_is_the_reference_s(c):
    g, NP, bkg = _case(c)
    ac = _actor()
    with torch.no_grad():
        for t in range(6):
            x0 = R2.standardise(g["reading"][t], g["mu"][t], g["sig"][t])
            assert x0 == np.float32(g["obs_std"][t, 0]), (c, t)                    # the standardised, clipped reading as the actor sees it: bit for bit
            loc = (g["est"][t, 1:] / AREA_MAX).astype(np.float32)
            logits, _, h1 = ac.policy_step(torch.from_numpy(g["obs_std"][t].astype(np.float32)).view(1, 11), torch.from_numpy(loc).view(1, 2),
                                           torch.from_numpy(g["h_before"][t]).view(1, 24))
            logp = torch.log_softmax(logits, dim=-1)[0].numpy()
            assert np.allclose(logp, g["logp"][t], rtol=1e-5, atol=1e-6), (c, t, logp - g["logp"][t])
            assert np.allclose(h1[0].numpy(), g["h_after"][t], rtol=1e-5, atol=1e-6), (c, t)
            if t:
                assert np.array_equal(g["h_before"][t], g["h_after"][t - 1])
                assert np.array_equal(g["det"][t], g["det"][t - 1] + R2.ACTION[g["act"][t - 1]])     # sim_step's table moves the walk


def test_header_and_binding_carry_the_new_entries():
    from radiation_ppo_amd import _lib, evaluate
    from radiation_ppo_amd.bpf import BootstrapParticleFilter
    sym = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    v, pp, d, i = C.c_void_p, C.POINTER(C.c_void_p), C.c_double, C.c_int32
    assert sym["rs_bpf_fim"] == (C.c_int, [v, v, v, v, v, i, v, v, v])
    assert [a for _, a in _lib._functions["rs_bpf_fim"][1]] == ["h", "p", "s", "alive", "pos", "prior", "F", "trace", "stream"]
    assert sym["rs_bpf_a2c_eval_step"] == (C.c_int, [v, pp, i, v, v, v, v, d, v, v, v, v, v, v, v, v])
    names = list(_lib._functions)
    assert names.index("rs_bpf_draws") < names.index("rs_bpf_fim") < names.index("rs_bpf_a2c_eval_step") < names.index("rs_peek")
    text = open(_lib.HEADER_PATH).read()
    assert "core.py:686-694" in text and "test_policy.py:136-154" in text and "broadcasts y" in text
    assert "broadcasts y" in BootstrapParticleFilter.fim.__doc__ and "mis-specified" in evaluate.run_test_environments_bpf_a2c.__doc__
    assert tuple(map(tuple, R2.ACTION)) == evaluate.BPF_A2C_ACTION


def test_refusals_come_before_any_launch():
    from radiation_ppo_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    w = 4096                                                       # non-NULL stand-ins: every refusal comes before anything is touched
    bad = _lib.RS_ERR_INVALID_ARG
    prm, st = C.c_void_p(), C.c_void_p()
    assert lib.rs_bpf_params_create(64, 15.0, 1.0, 1.0, (C.c_double * 2)(1e2, 1e3), (C.c_double * 2)(0.0, 25e2), 0.6, 0.36,
                                    (C.c_int32 * 2)(75, 75), C.byref(prm)) == 0
    assert lib.rs_bpf_state_create(1, w, w, w, w, w, w, w, w, 1 << 20, C.byref(st)) == 0
    assert lib.rs_bpf_fim(None, prm, st, w, None, 0, w, None, None) == bad
    assert lib.rs_bpf_fim(w, None, st, w, None, 0, w, None, None) == bad and lib.rs_bpf_fim(w, prm, None, w, None, 1, w, None, None) == bad
    wts = (C.c_void_p * 8)(*([w] * 8))
    step = lambda h, ws, A, *rest: lib.rs_bpf_a2c_eval_step(h, ws, A, *rest, None, None, None)
    assert step(None, wts, 1, w, w, w, w, 2200.0, w, w, w, w, w) == bad       # the rest needs a handle: tests/test_bpf_a2c_step_gpu.py
    lib.rs_bpf_params_destroy(prm)
    lib.rs_bpf_state_destroy(st)


def test_the_runners_refuse_before_the_library_loads(monkeypatch):
    from radiation_ppo_amd import _lib, evaluate
    from radiation_ppo_amd.rada2c import RNNAgentPPO

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    sets = {"env_0": (np.array([500.0, 500.0]), np.array([1500.0, 1500.0]), 1000000, 20)}
    ag = RNNAgentPPO(id=0, device="cpu")
    wide = RNNAgentPPO(id=1, device="cpu", actor_critic_args=dict(hidden=((16,),), hidden_sizes_pol=((8,),), hidden_sizes_val=((8,),)))
    for agents, kw in (({}, {}), ({1: ag}, {}), ({i: ag for i in range(9)}, {}), ({0: ag}, dict(device="cpu")), ({0: ag}, dict(nParticles=1)),
                       ({0: ag}, dict(lanes_per_pass=0)), ({0: ag}, dict(lanes_per_pass=99, montecarlo_runs=100)), ({0: object()}, {}),
                       ({0: ag, 1: wide}, {}), ({0: wide}, dict(fused=True))):
        with pytest.raises(ValueError):
            evaluate.run_test_environments_bpf_a2c(agents, sets, **kw)
    with pytest.raises(ValueError):
        evaluate.run_test_environments_rid_fim(sets, fisher=True, device="cpu")


def test_evaluate_ppo_takes_bpf_a2c(monkeypatch, tmp_path):
    from radiation_ppo_amd import evaluate, testsets
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    seen = {}
    sets = {f"env_{i}": (np.array([500.0, 500.0]), np.array([1500.0, 1500.0]), 1000000, 20) for i in range(5)}
    monkeypatch.setattr(testsets, "load_test_environments", lambda path: sets)
    for i in range(2):
        RNNAgentPPO(id=i, device="cpu", seed=i).save(str(tmp_path / f"{i}_agent"))

    def runner(agents, env_sets, **kw):
        seen.update(kw, n=len(env_sets), agents=agents)
        return [], {"success_rate": 0.0}, {"bounds": np.zeros((6, 2, 7, 3, 3))}
    monkeypatch.setattr(evaluate, "run_test_environments_bpf_a2c", runner)
    ev = evaluate.evaluate_PPO(dict(test_env_path="nowhere", obstruction_count=0, episodes=3, montecarlo_runs=2, nParticles=500, fisher=True,
                                    actor_critic_architecture="bpf-a2c", number_of_agents=2, steps_per_episode=7, seed=3,
                                    model_path=str(tmp_path), device="cpu"))
    assert ev.evaluate() == ([], {"success_rate": 0.0}) and ev.extras["bounds"].shape == (6, 2, 7, 3, 3)
    assert seen["n"] == 3 and seen["nParticles"] == 500 and seen["fisher"] is True and seen["montecarlo_runs"] == 2
    assert sorted(seen["agents"]) == [0, 1] and all(hasattr(a.agent, "gru_cell") for a in seen["agents"].values())
    assert seen["steps_per_episode"] == 7 and seen["team_mode"] == "individual" and "alpha" not in seen
