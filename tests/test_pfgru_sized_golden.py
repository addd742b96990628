"""The torch PFGRUCell (radiation_ppo_amd/pfgru.py) at hidden widths other than 24 against the reference's own cell
(RADTEAM_core.PFGRUCell at hidden_size 64 and 16, tests/golden/pfgru_sized.npz) with every random draw replayed: location
predictions, resampled particles and log weights step by step, hidden state carried and every step from h0; state_dict keys
interchange (a predictor.pt of either side loads in the other).  Plus the packer of the sized kernels' weights."""
import os

import numpy as np
import pytest
import torch

from radiation_ppo_amd.pfgru import PFGRUCell, SIZED_WIDTHS, pack_sized_weights, sized_layout


def _cell(g, H):
    pre = f"h{H}_sd_"
    cell = PFGRUCell(input_size=3, obs_size=3, hidden_size=H)
    sd = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    assert sorted(sd) == sorted(cell.state_dict())
    cell.load_state_dict(sd)
    return cell.eval()


@pytest.mark.parametrize("H", [64, 16])
def test_cell_matches_reference_step_by_step(golden_dir, H):
    g = np.load(os.path.join(golden_dir, "pfgru_sized.npz"))
    cell = _cell(g, H)
    obs = torch.from_numpy(g[f"h{H}_obs"])
    with torch.no_grad():
        for tag, carry in (("carry", True), ("fresh", False)):
            h, p = cell.init_hidden(1, u=torch.from_numpy(g[f"h{H}_{tag}_h0"]).unsqueeze(0), device="cpu")
            for t in range(obs.shape[0]):
                loc, (h1, p1) = cell(obs[t:t + 1], (h, p), torch.from_numpy(g[f"h{H}_{tag}_eps"][t]).unsqueeze(0),
                                     resample_idx=torch.from_numpy(g[f"h{H}_{tag}_idx"][t]).unsqueeze(0))
                assert np.allclose(loc[0].numpy(), g[f"h{H}_{tag}_loc"][t].reshape(-1), rtol=1e-5, atol=1e-6), (tag, t)
                assert np.allclose(h1[0].numpy(), g[f"h{H}_{tag}_h"][t], rtol=1e-5, atol=1e-6), (tag, t)
                assert np.allclose(p1[0].numpy(), g[f"h{H}_{tag}_p"][t], rtol=1e-5, atol=2e-6), (tag, t)
                if carry:
                    h, p = h1, p1


@pytest.mark.parametrize("H", SIZED_WIDTHS)
def test_sized_packer_places_every_parameter(H):
    """pack_sized_weights writes each parameter exactly once where csrc/rs_pfgru_sized.hip reads it (checked by packing a cell whose
    parameters are all distinct and reading the blocks back)."""
    torch.manual_seed(H)
    cell = PFGRUCell(hidden_size=H)
    with torch.no_grad():
        n = 0
        for prm in cell.parameters():
            prm.copy_(torch.arange(n + 1, n + 1 + prm.numel(), dtype=torch.float32).view_as(prm))
            n += prm.numel()
    w = pack_sized_weights([cell])[0]
    L, K = sized_layout(H), H + 3
    assert w.numel() == L["stride"] and L["stride"] % 16 == 0
    assert sorted(int(v) for v in w[w != 0]) == list(range(1, n + 1))              # every parameter once, nothing else
    assert torch.equal(w[:K * H].view(K, H), cell.fc_r.weight.t())
    for b in range(H // 8):
        blk = w[L["ZN"] + b * K * 24:L["ZN"] + (b + 1) * K * 24].view(K, 24)
        assert torch.equal(blk[:, :8], cell.fc_z.weight[8 * b:8 * b + 8].t())
        assert torch.equal(blk[:, 8:16], cell.fc_n.weight[8 * b:8 * b + 8].t())
        assert torch.equal(blk[:, 16:], cell.fc_n.weight[H + 8 * b:H + 8 * b + 8].t())
    assert torch.equal(w[L["H0"]:L["H0B"]].view(H, 24), cell.hid_obs[0].weight.t())
