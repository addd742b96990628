#!/usr/bin/env python3
"""Generate tests/golden/pfgru_sized.npz: the reference's own PFGRUCell (algos/test_cnn/RADTEAM_core.py:1533-1666) at hidden widths
other than the CNN core's 24 -- 64 (PFGRUCell's constructor default, RAD-TEAM's `--hid-rec`) and 16 -- traced exactly as gen_pfgru in
make_golden.py traces the 24-unit cell: every reparameterisation draw recorded by replaying the generator state, every resampling index
by wrapping torch.multinomial.  One 8-step trace per width with the hidden state carried, one with every step from the episode's h0.

Runs where the reference checkout is (CPU only); uses make_golden.py's placeholder modules and does not modify that file.  The output
is plain data: inputs, weights and outputs.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

WIDTHS = (64, 16)
T = 8


def gen_pfgru_sized():
    import torch
    from algos.test_cnn import RADTEAM_core as R
    out = {}
    orig_mn = torch.multinomial
    for H in WIDTHS:
        torch.manual_seed(1000 + H)
        cell = R.PFGRUCell(input_size=3, obs_size=3, activation="tanh", hidden_size=H)
        cell.eval()
        eps_log, idx_log = [], []
        orig_rep = cell.reparameterize

        def rec_rep(mean, var, orig_rep=orig_rep, eps_log=eps_log):
            st = torch.get_rng_state()
            res = orig_rep(mean, var)
            end = torch.get_rng_state()
            torch.set_rng_state(st)
            eps_log.append(torch.FloatTensor(var.shape).normal_().clone())   # the same draw the reference just consumed
            assert torch.equal(torch.get_rng_state(), end)
            return res
        cell.reparameterize = rec_rep

        def rec_mn(*a, idx_log=idx_log, **k):
            r = orig_mn(*a, **k)
            idx_log.append(r.clone())
            return r
        torch.multinomial = rec_mn
        try:
            rng = np.random.default_rng(37 + H)
            obs = np.stack([rng.poisson(800, T).astype(np.float32) / 100.0, rng.uniform(0.1, 1.0, T).astype(np.float32),
                            rng.uniform(0.1, 1.0, T).astype(np.float32)], axis=1)
            out[f"h{H}_obs"] = obs
            out.update({f"h{H}_sd_" + k: v.numpy() for k, v in cell.state_dict().items()})
            with torch.no_grad():
                for tag, carry in (("carry", True), ("fresh", False)):
                    hidden = cell.init_hidden(1)
                    h0 = hidden[0].clone()
                    eps_log.clear(); idx_log.clear()
                    locs, hs, ps = [], [], []
                    for t in range(T):
                        loc, new_hidden = cell(torch.from_numpy(obs[t:t + 1]), hidden)
                        if carry:
                            hidden = new_hidden
                        locs.append(loc.numpy().copy()); hs.append(new_hidden[0].numpy().copy())
                        ps.append(new_hidden[1].numpy().reshape(-1).copy())
                    out.update({f"h{H}_{tag}_h0": h0.numpy(), f"h{H}_{tag}_eps": torch.stack(eps_log).numpy(),
                                f"h{H}_{tag}_idx": torch.stack(idx_log).numpy().reshape(T, -1).astype(np.int64),
                                f"h{H}_{tag}_loc": np.stack(locs), f"h{H}_{tag}_h": np.stack(hs), f"h{H}_{tag}_p": np.stack(ps)})
        finally:
            torch.multinomial = orig_mn
    path = os.path.join(make_golden.OUT, "pfgru_sized.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make_golden._install_placeholders()
    sys.path.insert(0, os.path.join(make_golden.REF, "gym_rad_search"))
    sys.path.insert(0, make_golden.REF)
    gen_pfgru_sized()
