"""The refusals of the three lane-per-run team runners that need no device (evaluate._run_lane_per_run_team): ids other than 0..A-1
and, for the two RAD-TEAM runners, a device that is not cuda.  Each comes before an agent, the library or an environment is touched:
the agents are placeholders, and _lib.load and RadSearchVec fail when they are reached."""
import numpy as np
import pytest


@pytest.fixture
def ev(monkeypatch):
    from radiation_ppo_amd import _lib, evaluate

    def reached(*a, **k):
        raise AssertionError("the refusal must come before the library is loaded and before an environment is built")
    monkeypatch.setattr(_lib, "load", reached)
    monkeypatch.setattr(evaluate, "RadSearchVec", reached)
    return evaluate


SETS = {"env_0": (np.zeros(2), np.zeros(2), 1, 1)}
CNN_RUNNERS = ["run_test_environments_cnn_team", "run_test_environments_cnn_team_sized"]


@pytest.mark.parametrize("runner", CNN_RUNNERS)
def test_cnn_team_runners_refuse_other_ids_and_name_the_runner_that_takes_them(ev, runner):
    with pytest.raises(ValueError, match="run_test_environments_cnn"):
        getattr(ev, runner)({0: object(), 2: object()}, SETS)


@pytest.mark.parametrize("runner", CNN_RUNNERS)
def test_cnn_team_runners_refuse_a_device_that_is_not_cuda(ev, runner):
    with pytest.raises(ValueError, match="run_test_environments_cnn"):
        getattr(ev, runner)({0: object(), 1: object()}, SETS, device="cpu")


def test_feed_forward_team_runner_refuses_other_ids(ev):
    with pytest.raises(ValueError):
        ev.run_test_environments_team({0: object(), 2: object()}, SETS)
