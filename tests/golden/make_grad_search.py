#!/usr/bin/env python3
"""Generate tests/golden/grad_search.npz by running the REAL reference's gradient-search controller
(algos/test_environment/eval/core.py:622-653, GradSearch) on recorded observations.

Like make_golden.py this runs only where the reference is at hand; its output is plain data.  The reference file is imported
unmodified.  Two modules it imports are not installed here and are replaced by semantics-free placeholders created in a temp
directory (never committed):

  * numba -- `jit(...)` returns the function unchanged (one decorated helper of the particle filter, never called here)
  * gym   -- gym.spaces.Box / Discrete as empty classes (imported, never used by GradSearch)

GradSearch.step looks ahead with `env.step(act)` on the OLD single-agent env (eval/test_policy.py builds it), reads the candidate
observation o and restores the detector.  ReplayEnv below is that env reduced to what step() touches: it returns the recorded
candidate observation of the move and carries the attributes step() assigns.  What is recorded per row: the current observation
`cur` [3] (reading, x, y), the eight candidate observations `cand` [8, 3], q, the controller's `grad` tensor (float32) after the
loop and softmax(grad) as the controller builds it (nn.Softmax(0) on the float32 tensor).  A candidate whose coordinates equal the
current ones is a move that did not take place (core.py:641).

Rows: random readings with q in {0.5, 1, 4}; rows with 1..8 blocked moves; saturated rows (differences of +-1e4 counts)."""
import os
import sys
import tempfile
import textwrap

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def _install_placeholders() -> str:
    d = tempfile.mkdtemp(prefix="gs_placeholders_")

    def w(rel, src):
        p = os.path.join(d, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            f.write(textwrap.dedent(src))
    w("numba/__init__.py", """
        def jit(*a, **k):
            return lambda f: f
    """)
    w("gym/__init__.py", "from . import spaces\n")
    w("gym/spaces.py", """
        class Box:
            pass
        class Discrete:
            pass
    """)
    sys.path.insert(0, d)
    return d


class _Detector:
    def set_x(self, x):
        self.x = x

    def set_y(self, y):
        self.y = y


class ReplayEnv:
    """what GradSearch.step touches of the env: det_coords, detector.set_x / set_y, step(act) -> (o, _, _, _), det_sto, meas_sto,
    iter_count"""

    def __init__(self, cur, cand):
        self.det_coords = np.array(cur[1:3])
        self.detector = _Detector()
        self.cand = cand
        self.det_sto, self.meas_sto, self.iter_count = [], [], 0

    def step(self, act):
        self.det_sto.append(None)
        self.meas_sto.append(None)
        return self.cand[int(act)].copy(), None, None, None


def main():
    _install_placeholders()
    sys.path.insert(0, os.path.join(REF, "algos", "test_environment", "eval"))
    import torch
    import core                                                    # the reference's file, unmodified
    rng = np.random.default_rng(20240229)
    scale = 1 / 2200.0
    steps = np.array([(-100, 0), (-71, 71), (0, 100), (71, 71), (100, 0), (71, -71), (0, -100), (-71, -71)], dtype=np.float64)
    rows = []
    for i in range(96):
        q = (0.5, 1.0, 4.0)[i % 3]
        xy = rng.integers(300, 2000, size=2).astype(np.float64)
        cur = np.array([float(rng.integers(0, 3000)), xy[0] * scale, xy[1] * scale])
        kind = i // 3 % 4                                          # 0, 1: plain; 2: blocked moves; 3: saturated
        spread = 10000 if kind == 3 else int(rng.choice([5, 60, 400]))
        cand = np.zeros((8, 3))
        for k in range(8):
            cand[k] = (float(max(0, int(cur[0]) + int(rng.integers(-spread, spread + 1)))), (xy[0] + steps[k, 0]) * scale, (xy[1] + steps[k, 1]) * scale)
        if kind == 3:
            cur[0] = 10000.0
            cand[:, 0] = cur[0] + rng.choice([-10000.0, 0.0, 10000.0], size=8)
        if kind == 2:
            for k in rng.choice(8, size=int(rng.integers(1, 9)), replace=False):
                cand[k, 1:3] = cur[1:3]                            # the move did not take place: the coordinates are the current ones
        rows.append((q, cur, cand))
    out = {k: [] for k in ("q", "cur", "cand", "grad", "probs")}
    for q, cur, cand in rows:
        gs = core.GradSearch(q=q, env=ReplayEnv(cur, cand))
        act = gs.step(cur)
        assert 0 <= act <= 7
        probs = gs.softmax(gs.grad)
        assert gs.grad.dtype == torch.float32
        out["q"].append(q); out["cur"].append(cur); out["cand"].append(cand)
        out["grad"].append(gs.grad.numpy().copy()); out["probs"].append(probs.numpy().copy())
    np.savez(os.path.join(OUT, "grad_search.npz"), **{k: np.asarray(v) for k, v in out.items()})
    print("grad_search.npz:", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
