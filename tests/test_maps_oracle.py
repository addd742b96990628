"""The heat-map oracle (oracle/maps_oracle.py) against golden vectors captured from the reference's MapsBuffer
(tests/golden/maps.npz) and the reference's own unit-test known answers."""
import os

import numpy as np

from oracle.maps_oracle import MapsOracle, calculate_map_dimensions, calculate_resolution_accuracy, logscale


def test_constants_match_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "maps.npz"))
    ra = calculate_resolution_accuracy(0.01, 1 / 2200.0)
    assert ra == float(g["ra"]) == 22.0
    off = (1 / 2200.0) * 500.0
    assert off == float(g["offset"])
    assert calculate_map_dimensions((1, 1), ra, off) == tuple(int(v) for v in g["map_dim"]) == (27, 27)
    base = int(g["base"])
    for i, c in enumerate(range(0, 2 * base, 2)):
        assert logscale(c, base, 2) == g["logscale"][i]


def test_inflate_known_answers():
    """unit_tests/test_RADTEAM_core.py:421-449 style: int(coordinate * resolution_accuracy)."""
    m = MapsOracle(steps_per_episode=120, number_of_agents=2)
    o = np.array([1500.0, 0.5, 0.25, 0, 0, 0, 0, 0, 0, 0, 0])
    assert m._inflate(o) == (11, 5) and m._inflate((0.5, 0.25)) == (11, 5)
    assert m.dims == (27, 27) and m.base == 242


def test_maps_match_reference_step_by_step(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "maps.npz")).items())
    A, L = int(g["A"]), int(g["L"])
    bufs = [MapsOracle(steps_per_episode=L, number_of_agents=A, resolution_accuracy=float(g["ra"]), offset=float(g["offset"]))
            for _ in range(A)]
    for t in range(g["obs"].shape[0]):
        od = {i: g["obs"][t, i] for i in range(A)}
        pred = (float(g["pred"][t, 0]), float(g["pred"][t, 1]))
        for i in range(A):
            maps = bufs[i].observation_to_map(od, i, pred)
            for k in range(7):
                assert np.array_equal(maps[k], g["maps"][t, i, k]), (t, i, k)
        if g["reset_after"][t]:
            for b in bufs:
                b.reset()


def test_tall_linear_two_step_weight_gradient_matches_autograd():
    """maps._LinearTall (the Linear layers behind the CNN trunk at update-chunk sizes): same outputs and gradients as nn.Linear."""
    import torch
    from radiation_ppo_amd.maps import _LinearTall, _head
    torch.manual_seed(0)
    for fin, fout in ((32, 16), (16, 8), (48, 32)):
        lin = torch.nn.Linear(fin, fout).double()
        x = torch.randn(65536, fin, dtype=torch.float64, requires_grad=True)
        g = torch.randn(65536, fout, dtype=torch.float64)
        y_ref = lin(x)
        gx_ref, gw_ref, gb_ref = torch.autograd.grad(y_ref, (x, lin.weight, lin.bias), g)
        y = _LinearTall.apply(x, lin.weight, lin.bias)
        gx, gw, gb = torch.autograd.grad(y, (x, lin.weight, lin.bias), g)
        assert torch.equal(y, y_ref) and torch.allclose(gx, gx_ref, rtol=1e-12, atol=1e-12)
        assert torch.allclose(gw, gw_ref, rtol=1e-10, atol=1e-10) and torch.allclose(gb, gb_ref, rtol=1e-10, atol=1e-10)
        assert _head(lin, x).grad_fn is not None and "LinearTall" in type(_head(lin, x).grad_fn).__name__
    small = torch.randn(100, 32, dtype=torch.float64, requires_grad=True)
    assert "LinearTall" not in type(_head(torch.nn.Linear(32, 16).double(), small).grad_fn).__name__      # small batches: plain nn.Linear


def _replay_edge(g, tag):
    A, L = int(g[tag + "_A"]), int(g[tag + "_L"])
    bufs = [MapsOracle(steps_per_episode=L, number_of_agents=A, resolution_accuracy=float(g["ra"]), offset=float(g["offset"]),
                       grid_bounds=tuple(int(v) for v in g[tag + "_grid_bounds"])) for _ in range(A)]
    assert bufs[0].dims == tuple(int(v) for v in g[tag + "_map_dim"])
    cells = set()
    for t in range(g[tag + "_obs"].shape[0]):
        od = {i: g[tag + "_obs"][t, i] for i in range(A)}
        pred = (float(g[tag + "_pred"][t, 0]), float(g[tag + "_pred"][t, 1]))
        for i in range(A):
            maps = bufs[i].observation_to_map(od, i, pred)
            for k in range(7):
                assert np.array_equal(maps[k], g[tag + "_maps"][t, i, k]), (tag, t, i, k)
        cells |= set(bufs[0].last_coords.values()) | {bufs[0].last_prediction}
        if g[tag + "_reset_after"][t]:
            for b in bufs:
                b.reset()
    return bufs[0].dims, cells


def test_maps_match_reference_on_negative_cells_edges_and_a_non_square_map(golden_dir):
    """tests/golden/mapsedge.npz (make_golden.py gen_maps_edge): the reference's own MapsBuffer on what maps.npz does not reach -- negative
    coordinates and predictions (numpy indexes from the end), coordinates exactly on k / resolution_accuracy and on both sides of the last
    cell's edge, a chain of 24 tied readings in one cell, resets with a wrapped cell occupied, and grid_bounds = (1, 2) (27 x 49 cells).  The
    oracle reproduces all seven maps of every owner at every step, float32-exact.

    What the reference REFUSES, recorded in the same file: a coordinate or a prediction at X / ra or below -X / ra raises IndexError, a NaN
    prediction ValueError, an infinite one OverflowError.  What K5 does on those inputs (clamp and RS_MAPERR_OFF_MAP for a coordinate, the
    last prediction cell kept for a prediction) is therefore this project's own choice, pinned in tests/test_maps_direct_gpu.py."""
    g = dict(np.load(os.path.join(golden_dir, "mapsedge.npz")).items())
    dims, cells = _replay_edge(g, "sq")
    assert dims == (27, 27) and min(c[0] for c in cells) == -27 and (-1, 5) in cells and (26, 5) in cells and (0, 5) in cells
    dims, cells = _replay_edge(g, "rect")
    assert dims == (27, 49) and (26, 48) in cells and min(c[1] for c in cells) < -27 and max(c[1] for c in cells) > 27
    refused = dict(s.split(": ") for s in g["refused"])
    assert refused == {"coordinate x at X / ra": "IndexError", "coordinate x below -X / ra": "IndexError", "prediction x at X / ra": "IndexError",
                       "prediction y below -Y / ra": "IndexError", "prediction NaN": "ValueError", "prediction +inf": "OverflowError",
                       "prediction -inf": "OverflowError"}


def test_oracle_without_a_prediction_leaves_the_prediction_map():
    """loc_prediction=None (the reference's `if PFGRU:` switch off, RADTEAM_core.py:563): every other map as with a prediction, the
    prediction map and last_prediction untouched."""
    o = np.array([3.0, 0.5, 0.25, 0, 0.5, 0, 0, 0, 0, 0, 0])
    a, b = MapsOracle(steps_per_episode=10, number_of_agents=1), MapsOracle(steps_per_episode=10, number_of_agents=1)
    a.observation_to_map({0: o}, 0, (0.1, 0.2))
    b.observation_to_map({0: o}, 0, (0.1, 0.2))
    ma, mb = a.observation_to_map({0: o}, 0, None), b.observation_to_map({0: o}, 0, (0.1, 0.2))
    assert all(np.array_equal(x, y) for x, y in zip(ma, mb)) and a.last_prediction == b.last_prediction == (2, 4)
    c = MapsOracle(steps_per_episode=10, number_of_agents=1)
    assert c.observation_to_map({0: o}, 0, None)[0].max() == 0.0 and c.last_prediction == ()
