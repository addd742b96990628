"""rs_ppo_prepare (episode weights and advantage normalisation of the finished buffer in HIP) against the tensor code it replaces on
one rank: RolloutBuffer.episode_weights() / n_total and normalize_advantages(), compared with torch.equal, and the float32 mean and
std compared exactly.

The two float64 sums behind mean and std are taken in a different order by every implementation.  The advantages' seed is therefore
chosen on the CPU, per case, as the first one for which numpy's pairwise sum, a sequential float64 sum and math.fsum all round to
the same float32 mean and, with that mean, to the same float32 std: the equality below then does not rest on a summation order."""
import functools
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(12, 64), (480, 128), (12, 48)]        # 48 columns: 1 / n_total is no power of two, and a wave has idle lanes
PATTERNS = ["every_step", "final_only", "at_t0", "random", "single_episode_column"]


def _cuts(T, N, pattern):
    rng = np.random.default_rng(T * 1000 + N)
    cut = np.zeros((T, N), dtype=np.uint8)
    if pattern == "every_step":
        cut[:] = 1
    elif pattern == "final_only":
        cut[T - 1] = 1
    elif pattern == "at_t0":
        cut[0] = 1
        cut[T - 1] = 1
    else:
        cut[:] = rng.random((T, N)) < (0.3 if T < 100 else 0.02)
        cut[T - 1, ::2] = 1                      # every other column: the last step closes its episode without a cut flag
        if pattern == "single_episode_column":
            cut[:, 3] = 0
            cut[T - 1, 3] = 1                    # one column is a single episode of all T steps
    return cut


def _three_sums(x64):
    return float(np.sum(x64)), float(np.cumsum(x64)[-1]), math.fsum(x64.tolist())


@functools.lru_cache(maxsize=None)
def _advantages(T, N):
    """(adv [T, N] float32, mean, std) for the first seed whose mean and std do not depend on the order of the sums"""
    n = T * N
    for seed in range(1000):
        adv = (0.7 + 1.9 * np.random.default_rng(seed).standard_normal((T, N))).astype(np.float32)
        means = {np.float32(s / n) for s in _three_sums(adv.astype(np.float64).ravel())}
        if len(means) != 1:
            continue
        mean = means.pop()
        d = adv - mean                                        # float32
        stds = {np.float32(math.sqrt(s / n)) for s in _three_sums((d * d).astype(np.float64).ravel())}
        if len(stds) != 1:
            continue
        return adv, mean, stds.pop()
    raise AssertionError("no seed found")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T,N", SHAPES)
def test_prepare_equals_tensor_code(T, N, pattern):
    from radiation_ppo_amd.ppo import RolloutBuffer, normalize_advantages, prepare_update_hip
    adv_h, mean_h, std_h = _advantages(T, N)
    buf = RolloutBuffer(T, N, 1, 11, "cuda")
    buf.cut.copy_(torch.from_numpy(_cuts(T, N, pattern)).cuda().view(T, N, 1))
    buf.adv.copy_(torch.from_numpy(adv_h).cuda().view(T, N, 1))
    col = types.SimpleNamespace(buf=buf, N=N)

    w_ref = (buf.episode_weights() / N).reshape(-1)
    adv_ref = normalize_advantages(buf.adv[:, :, 0]).reshape(-1)

    w, adv_n = prepare_update_hip(col)
    torch.cuda.synchronize()
    assert w.shape == w_ref.shape and adv_n.shape == adv_ref.shape
    assert torch.equal(w, w_ref)
    assert torch.equal(adv_n, adv_ref)
    mean_std = col._prep["mean_std"].cpu().numpy()
    assert mean_std[0] == mean_h and mean_std[1] == std_h, (mean_std, mean_h, std_h)
    # the weights of a column sum to 1 / N whatever its episodes are; the buffer's advantages stay unnormalised
    assert torch.allclose(w.view(T, N).double().sum(0), torch.full((N,), 1.0 / N, dtype=torch.float64, device="cuda"), rtol=1e-5, atol=0)
    assert torch.equal(buf.adv.cpu().view(T, N), torch.from_numpy(adv_h))
    # no atomics, fixed order: a second call leaves the same bits, in the same buffers
    first = (w.clone(), adv_n.clone(), col._prep["mean_std"].clone())
    w2, adv2 = prepare_update_hip(col)
    assert w2.data_ptr() == w.data_ptr() and adv2.data_ptr() == adv_n.data_ptr()
    assert torch.equal(w2, first[0]) and torch.equal(adv2, first[1]) and torch.equal(col._prep["mean_std"], first[2])
