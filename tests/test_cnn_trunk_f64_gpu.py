"""K9 / K10 (rs_cnn_trunk_forward / rs_cnn_trunk_backward, csrc/rs_cnn.hip) against float64, element by element, through the C ABI.
These two kernels are what the team forward kernels, rs_cnn_trunk_infer and the tiled trunk at 27 x 27 are held to bit for bit, so
their own check is the root of that tree.  Reference, error model, kink rule and inputs: tests/_cnn_trunk_ref.py (its CPU self-checks,
float32 torch under the same rule and the planted faults the rule must report: test_cnn_trunk_ref_cpu.py).

  K9   a2 and p1 at EVERY element within RTOL |ref| + k U mag (K1 = 14.5 on conv1's magnitude; K2 = 17.1 on conv2's plus p1's allowance
       carried through |w2|); amax and relu_mask equal outside the kink exclusions, which may cover at most 1 % of either.  Outputs are
       prefilled with NaN / 0x77 and followed by one guard image that must come back untouched.
  K10  fed the REFERENCE's branch data (relu_mask, amax, p1 rounded to float32) it is a linear map of da2: all four gradients at every
       element, no exclusions, k from the operation counts (_cnn_trunk_ref.backward_k).  The slab is prefilled with NaN, one guard row
       behind it; every row comes back finite and a second run gives the same bits.  The rows are summed as ConvTrunk.backward sums
       them (float32, on the device).
  Grid edges: Gf = rs_cnn_trunk_forward_grid(2^20, Cin) and Gb = rs_cnn_trunk_slab_rows(2^20, Cin) are the persistent grids; K9 runs at
       S = 1, 2, 4, 3 Gf + 1 (workgroup 0 wraps into a round of one image) and 6 Gf + 2 (two wraps, a round of two), K10 at S = 1, 2,
       Gb + 1 and 2 Gb + 1.  One batch of the largest size is built, and its float64 forward computed, once per module; every test
       takes a prefix of it.  Its first 38 images are the stamp images (_cnn_trunk_ref.stamp_pairs).
  ConvTrunk.apply at S = 5 per network: K10 on the kernel's own float32 branch data; an image whose branch data differ from the
       reference's gets zero weight, and at most 10 % of the images may.

Every worst ratio is printed; profiles/cnn_trunk_float64_ratios.txt keeps a copy."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_trunk_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
NETS = ("actor", "critic")
N_STAMP = len(T.stamp_pairs())                    # 38
S_DIRECT = N_STAMP + 3                            # the stamp images and three random ones: 41 = 13 rounds of three and a round of two
S_K9 = N_STAMP + 27                               # 65 = 21 rounds and a round of two
AUTO_LO = N_STAMP                                 # ConvTrunk.apply: images 38..42 of the batch
PATTERNS = ("reference", "amax 0", "amax 1", "amax 2", "amax 3", "amax random", "mask 0x0000", "mask 0xFFFF", "mask random", "p1 zero",
            "p1 chequerboard", "da2 channels 0..12", "da2 channels 13..15", "da2 pixel 168", "da2 zero for image 7")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


class Net:
    """One network of the module's batch: seq (float32, CPU), seq64, cin, the persistent grids Gf / Gb, dense (float64), fwd (the
    float64 forward of the whole batch), conv (the four convolution parameters on the device)."""


class Big:
    """The module's batch: lib, nets {name: Net}, S (the largest size any test runs), maps / own / pred (CPU), maps_d (device), da2."""


@pytest.fixture(scope="module")
def big():
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    b = Big()
    b.lib = lib
    actor, critic = T.networks(3)
    b.nets = {}
    for name, seq, cin in (("actor", actor.actor, 6), ("critic", critic.critic, 4)):
        n = Net()
        n.name, n.seq, n.cin = name, seq, cin
        n.Gf, n.Gb = lib.rs_cnn_trunk_forward_grid(1 << 20, cin), lib.rs_cnn_trunk_slab_rows(1 << 20, cin)
        assert 1 <= n.Gf <= 4096 and 1 <= n.Gb <= 4096, (n.Gf, n.Gb)
        # the query is cnn_grid of the ROUND count: below the cap it is the number of rounds
        assert lib.rs_cnn_trunk_forward_grid(1, cin) == 1 and lib.rs_cnn_trunk_forward_grid(4, cin) == 2
        assert lib.rs_cnn_trunk_forward_grid(3 * n.Gf, cin) == n.Gf == lib.rs_cnn_trunk_forward_grid(3 * n.Gf + 1, cin)
        b.nets[name] = n
    b.S = max(max(6 * n.Gf + 2, 2 * n.Gb + 1) for n in b.nets.values())
    b.maps, b.own, b.pred = T.make_batch(b.S, seed=11)
    b.maps_d = b.maps.cuda()
    for n in b.nets.values():
        n.dense = T.dense_input(b.maps, b.own, b.pred) if n.cin == 6 else T.dense_input(b.maps)
        n.seq64 = T.F64(n.seq)
        n.fwd = T.trunk_forward_f64(n.seq64, n.dense)
        n.conv = [t.detach().clone().cuda().contiguous() for t in (n.seq[0].weight, n.seq[0].bias, n.seq[3].weight, n.seq[3].bias)]
    b.da2 = torch.randn(b.S, 2704, generator=torch.Generator().manual_seed(5))
    return b


def _columns(b, n, S, A, agent):
    """(cells, pcells, A, agent) on the device for the first S images: NULL columns for the critic."""
    if n.cin == 4:
        return None, None, 0, -1
    cells, pcells = T.cell_columns(b.own[:S], b.pred[:S], A, agent, seed=100 + A)
    return cells.cuda(), pcells.cuda(), A, agent


def _k9(b, n, S, A=3, agent=1):
    """rs_cnn_trunk_forward on the first S images with NaN / 0x77 prefilled outputs of S + 1 images: checks that every element of the S
    images was written and that the guard image kept its bits; returns (a2, p1, amax, relu_mask) of the S images on the CPU."""
    from radiation_ppo_amd import _lib
    cells, pcells, A, agent = _columns(b, n, S, A, agent)
    a2 = torch.full((S + 1, 2704), float("nan"), device="cuda")
    p1 = torch.full((S + 1, 169, 8), float("nan"), device="cuda")
    amax = torch.full((S + 1, 169, 8), 0x77, dtype=torch.uint8, device="cuda")
    mask = torch.full((S + 1, 169), 0x7777, dtype=torch.int16, device="cuda")
    guards = [_bits(t[S]) for t in (a2, p1, amax, mask)]
    wt = torch.empty(b.lib.rs_cnn_trunk_scratch_floats(n.cin), dtype=torch.float32, device="cuda")
    _lib.check(b.lib.rs_cnn_trunk_forward(b.maps_d.data_ptr(), None if cells is None else cells.data_ptr(),
                                          None if pcells is None else pcells.data_ptr(), A, agent, S, *(t.data_ptr() for t in n.conv),
                                          a2.data_ptr(), p1.data_ptr(), amax.data_ptr(), mask.data_ptr(), wt.data_ptr(), _stream()),
               "rs_cnn_trunk_forward")
    torch.cuda.synchronize()
    for t, g, what in zip((a2, p1, amax, mask), guards, ("a2", "p1", "amax", "relu_mask")):
        assert torch.equal(_bits(t[S]), g), f"{n.name} S{S}: the guard image behind {what} was written"
    a2, p1, amax, mask = a2[:S].cpu(), p1[:S].cpu(), amax[:S].cpu(), mask[:S].cpu()
    assert bool(torch.isfinite(a2).all()) and bool(torch.isfinite(p1).all()), f"{n.name} S{S}: an element of a2 / p1 was not written"
    assert bool((amax <= 3).all()), f"{n.name} S{S}: an arg-max code was not written"
    assert bool(((mask != 0x7777) | (n.fwd.relu_mask[:S] == 0x7777)).all()), f"{n.name} S{S}: a ReLU mask was not written"
    return a2, p1, amax, mask


def _k10(b, n, S, da2, mask, p1, amax, A=3, agent=1):
    """rs_cnn_trunk_backward on the first S images with the given branch data (CPU tensors: mask [S, 169] int64 bits, p1 float32, amax
    uint8) into a NaN slab with one guard row; run twice; returns the four gradients, the rows summed as ConvTrunk.backward does."""
    from radiation_ppo_amd import _lib
    cells, pcells, A, agent = _columns(b, n, S, A, agent)
    rows, row = b.lib.rs_cnn_trunk_slab_rows(S, n.cin), b.lib.rs_cnn_trunk_slab_row(n.cin)
    assert rows == min(S, n.Gb) and row == 8 * n.cin * 9 + 8 + 1152 + 16
    dev = [da2.float().contiguous().cuda(), T.int16_mask(mask).contiguous().cuda(), p1.float().contiguous().cuda(), amax.contiguous().cuda()]
    assert dev[0].shape == (S, 2704) and dev[1].shape == (S, 169) and dev[2].shape == (S, 169, 8) and dev[3].shape == (S, 169, 8)
    wt = torch.empty(b.lib.rs_cnn_trunk_scratch_floats(n.cin), dtype=torch.float32, device="cuda")
    slabs = []
    for _ in range(2):
        slab = torch.full((rows + 1, row), float("nan"), device="cuda")
        guard = _bits(slab[rows])
        _lib.check(b.lib.rs_cnn_trunk_backward(b.maps_d.data_ptr(), None if cells is None else cells.data_ptr(),
                                               None if pcells is None else pcells.data_ptr(), A, agent, S, n.conv[2].data_ptr(),
                                               *(t.data_ptr() for t in dev), slab.data_ptr(), wt.data_ptr(), _stream()), "rs_cnn_trunk_backward")
        torch.cuda.synchronize()
        assert torch.equal(_bits(slab[rows]), guard), f"{n.name} S{S}: the guard row behind the slab was written"
        assert bool(torch.isfinite(slab[:rows]).all()), f"{n.name} S{S}: a slab row is not finite"
        slabs.append(slab[:rows])
    assert torch.equal(_bits(slabs[0]), _bits(slabs[1])), f"{n.name} S{S}: two runs differ"
    return T.split_slab_sum(slabs[0].sum(dim=0).cpu(), n.cin), rows


# ------------------------------------------------------------------------------------------------ K9
@pytest.mark.parametrize("net,A,agent", [("actor", 1, 0), ("actor", 8, 0), ("actor", 8, 7), ("critic", 0, -1)])
def test_k9_outputs_match_float64(big, net, A, agent):
    """The stamp images and 27 random ones: every cell of STAMP_CELLS as owner, as prediction and as both, through the first and the last
    agent column of [S, 8] cell tensors whose other columns hold other cells, and through a single column."""
    n = big.nets[net]
    rep = []
    try:
        T.check_forward(*_k9(big, n, S_K9, A, agent), n.fwd.head(S_K9), f"K9 {net} S{S_K9}" + (f" A{A} agent {agent}" if A else ""), report=rep)
    finally:
        print("\n".join(rep))


@pytest.mark.parametrize("size", ["1", "2", "4", "3Gf+1", "6Gf+2"])
@pytest.mark.parametrize("net", NETS)
def test_k9_grid_edges_match_float64(big, net, size):
    n = big.nets[net]
    S = {"1": 1, "2": 2, "4": 4, "3Gf+1": 3 * n.Gf + 1, "6Gf+2": 6 * n.Gf + 2}[size]
    rep = []
    try:
        T.check_forward(*_k9(big, n, S), n.fwd.head(S), f"K9 {net} S{S} ({size}, Gf {n.Gf})", report=rep)
    finally:
        print("\n".join(rep))


# ------------------------------------------------------------------------------------------------ K10
def _pattern(big, n, S, pattern):
    """(da2, relu_mask, p1, amax) of a K10 pattern on the first S images: the reference's branch data with one part replaced."""
    g = torch.Generator().manual_seed(PATTERNS.index(pattern))
    f = n.fwd
    da2, mask, p1, amax = big.da2[:S].clone(), f.relu_mask[:S].clone(), f.p1[:S].float(), f.amax[:S].clone()
    kind, _, arg = pattern.partition(" ")
    if kind == "amax":
        amax = torch.randint(0, 4, amax.shape, generator=g).to(torch.uint8) if arg == "random" else torch.full_like(amax, int(arg))
    elif kind == "mask":
        mask = torch.randint(0, 65536, mask.shape, generator=g) if arg == "random" else torch.full_like(mask, int(arg, 16))
    elif pattern == "p1 zero":
        p1 = torch.zeros_like(p1)
    elif pattern == "p1 chequerboard":
        cell = torch.arange(169)
        p1 = p1 * (((cell // 13 + cell % 13).view(1, 169, 1) + torch.arange(8).view(1, 1, 8)) % 2).float()
    elif kind == "da2":
        d = da2.view(S, 16, 169)
        if arg == "channels 0..12":
            d[:, 13:] = 0
        elif arg == "channels 13..15":
            d[:, :13] = 0
        elif arg == "pixel 168":
            d[:, :, :168] = 0
        else:
            d[7] = 0
    else:
        assert pattern == "reference"
    return da2, mask, p1, amax


@pytest.mark.parametrize("pattern", PATTERNS)
def test_k10_fed_the_reference_branch_data(big, pattern):
    """Both networks on the stamp images (+ 3): K10 is linear in da2 once its branch data are given, so nothing is excluded.  The
    reference pattern also runs through a single agent column and the last of eight."""
    S = S_DIRECT
    rep = []
    try:
        for n in big.nets.values():
            da2, mask, p1, amax = _pattern(big, n, S, pattern)
            ref = T.trunk_backward_f64(n.dense[:S], n.seq64[3].weight, da2, mask, p1, amax)
            cols = [(3, 1)] + ([(1, 0), (8, 7)] if pattern == "reference" and n.cin == 6 else [])
            for A, agent in cols:
                got, rows = _k10(big, n, S, da2, mask, p1, amax, A, agent)
                T.check_backward(got, ref, S, rows, f"K10 {n.name} S{S}" + (f" A{A} agent {agent}" if n.cin == 6 else "") + f" {pattern}", report=rep)
                if pattern in ("mask 0x0000", "p1 zero"):
                    dead = ("dW1", "db1", "dW2", "db2") if pattern == "mask 0x0000" else ("dW1", "db1", "dW2")
                    assert all(not bool(got[k].any()) for k in dead), (pattern, n.name)
    finally:
        print("\n".join(rep))


_PREFIX = {}


def _prefix_refs(big, n):
    """{S: Backward} for K10's grid-edge sizes on the reference's branch data: the float64 sums over image ranges, added up."""
    if n.name in _PREFIX:
        return _PREFIX[n.name]
    sizes = [1, 2, n.Gb + 1, 2 * n.Gb + 1]
    out, acc, lo = {}, T.Backward(n.cin, torch.float64), 0
    for S in sizes:
        f = n.fwd
        acc.add(T.trunk_backward_f64(n.dense[lo:S], n.seq64[3].weight, big.da2[lo:S], f.relu_mask[lo:S], f.p1[lo:S].float(), f.amax[lo:S]))
        snap = T.Backward(n.cin, torch.float64).add(acc)
        out[S], lo = snap, S
    _PREFIX[n.name] = out
    return out


@pytest.mark.parametrize("size", ["1", "2", "Gb+1", "2Gb+1"])
@pytest.mark.parametrize("net", NETS)
def test_k10_grid_edges_match_float64(big, net, size):
    n = big.nets[net]
    S = {"1": 1, "2": 2, "Gb+1": n.Gb + 1, "2Gb+1": 2 * n.Gb + 1}[size]
    ref = _prefix_refs(big, n)[S]
    f = n.fwd
    got, rows = _k10(big, n, S, big.da2[:S], f.relu_mask[:S], f.p1[:S].float(), f.amax[:S])
    rep = []
    try:
        T.check_backward(got, ref, S, rows, f"K10 {net} S{S} ({size}, Gb {n.Gb})", report=rep)
    finally:
        print("\n".join(rep))


# ------------------------------------------------------------------------------------------------ ConvTrunk.apply
@pytest.mark.parametrize("net", NETS)
def test_autograd_path_matches_float64(big, net):
    """ConvTrunk.apply at S = 5 (images 38..42 of the batch: a round of three and a round of two), backward from a given da2.  K10
    reads the kernel's own branch data here; an image where they differ from the reference's (amax, relu_mask or the sign of p1) gets
    zero weight, at most 10 % of the images.  The kernel's float32 p1 enters dW2 with its allowance."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import ConvTrunk
    n = big.nets[net]
    S, lo = 5, AUTO_LO
    maps = big.maps[lo:lo + S].contiguous().cuda()
    cells = pcells = None
    agent = -1
    if n.cin == 6:
        cells, pcells = (t.cuda() for t in T.cell_columns(big.own[lo:lo + S], big.pred[lo:lo + S], 3, 1, seed=7))
        agent = 1
    ref_f = n.fwd.rows(lo, lo + S)
    # the kernel's branch data, from the launch ConvTrunk.forward makes
    a2 = torch.empty(S, 2704, device="cuda")
    p1 = torch.empty(S, 169, 8, device="cuda")
    amax = torch.empty(S, 169, 8, dtype=torch.uint8, device="cuda")
    mask = torch.empty(S, 169, dtype=torch.int16, device="cuda")
    wt = torch.empty(big.lib.rs_cnn_trunk_scratch_floats(n.cin), dtype=torch.float32, device="cuda")
    _lib.check(big.lib.rs_cnn_trunk_forward(maps.data_ptr(), None if cells is None else cells.data_ptr(), None if pcells is None else pcells.data_ptr(),
                                            3 if n.cin == 6 else 0, agent, S, *(t.data_ptr() for t in n.conv), a2.data_ptr(), p1.data_ptr(),
                                            amax.data_ptr(), mask.data_ptr(), wt.data_ptr(), _stream()), "rs_cnn_trunk_forward")
    torch.cuda.synchronize()
    differs = (amax.cpu() != ref_f.amax).flatten(1).any(1) | ((mask.cpu().long() & 0xFFFF) != ref_f.relu_mask).any(1) \
        | ((p1.cpu() > 0) != (ref_f.p1 > 0)).flatten(1).any(1)
    assert float(differs.double().mean()) <= 0.10, differs.tolist()
    da2 = big.da2[lo:lo + S] * (~differs).float().unsqueeze(1)
    params = [t.clone().requires_grad_(True) for t in n.conv]
    out = ConvTrunk.apply(maps, cells, pcells, agent, *params, True)
    assert torch.equal(_bits(out), _bits(a2))
    out.backward(da2.cuda())
    ref = T.trunk_backward_f64(n.dense[lo:lo + S], n.seq64[3].weight, da2, ref_f.relu_mask, ref_f.p1, ref_f.amax, p1_tol=ref_f.tol_p1)
    got = dict(dW1=params[0].grad, db1=params[1].grad, dW2=params[2].grad, db2=params[3].grad)
    rep = []
    try:
        T.check_backward(got, ref, S, S, f"ConvTrunk.apply {net} S{S} ({int(differs.sum())} of {S} images zero-weighted)", report=rep)
    finally:
        print("\n".join(rep))

