"""CPU self-checks of tests/_cnn_trunk_ref.py, the float64 reference and rule that test_cnn_trunk_f64_gpu.py holds K9 / K10 to: the
written-out backward pass equals float64 autograd, the first-maximum pool equals torch's on exact ties, the rule passes the float32
torch path, and it reports every planted fault (a ratio above 1)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_trunk_ref as T  # noqa: E402

S = 47                                           # the 38 stamp images and nine random ones: 15 rounds of three and a round of two
NETS = ("actor", "critic")


class Case:
    pass


_CACHE = {}


def _case(net):
    if net in _CACHE:
        return _CACHE[net]
    c = Case()
    actor, critic = T.networks(3)
    c.seq = (actor.actor if net == "actor" else critic.critic)
    c.maps, c.own, c.pred = T.make_batch(S, seed=11)
    c.dense = T.dense_input(c.maps, c.own, c.pred) if net == "actor" else T.dense_input(c.maps)
    c.seq64 = T.F64(c.seq)
    c.fwd = T.trunk_forward_f64(c.seq64, c.dense)
    g = torch.Generator().manual_seed(5)
    c.da2 = torch.randn(S, 2704, generator=g)
    c.p1r = c.fwd.p1.float()                                          # what K10 is fed: the reference's p1 rounded to float32
    c.bwd = T.trunk_backward_f64(c.dense, c.seq64[3].weight, c.da2, c.fwd.relu_mask, c.p1r, c.fwd.amax)
    _CACHE[net] = c
    return c


def _f32_forward(c, z1=None):
    """The float32 torch path: (a2, p1, amax, relu_mask) from the library convolutions and torch's max-pool, in the kernels' layouts.
    z1: conv1's float32 output to go on from (the planted faults change it)."""
    with torch.no_grad():
        x = c.dense.float()
        if z1 is None:
            z1 = c.seq[0](x)
        best, ind = F.max_pool2d(torch.relu(z1), 2, 2, return_indices=True)
        z2 = c.seq[3](best)
    return torch.relu(z2).flatten(1), T._cells_last(best), T.amax_from_pool_indices(ind), T.pack_mask(z2 > 0)


def _worst(ratios, names):
    return max(r for b, r in ratios if b in names)


@pytest.mark.parametrize("net", NETS)
def test_backward_equals_float64_autograd(net):
    """With the branch data of trunk_forward_f64 (p1 NOT rounded), trunk_backward_f64 is the gradient of seq64[0:6]."""
    c = _case(net)
    seq = T.F64(c.seq)
    out = seq[0:6](c.dense)
    assert torch.equal(out, c.fwd.a2)
    out.backward(c.da2.double())
    b = T.trunk_backward_f64(c.dense, seq[3].weight, c.da2.double(), c.fwd.relu_mask, c.fwd.p1, c.fwd.amax)
    for name, p in zip(T.GRADS, (seq[0].weight, seq[0].bias, seq[3].weight, seq[3].bias)):
        err = float((b.grads[name] - p.grad).abs().max())
        assert err <= 1e-12 * max(1.0, float(p.grad.abs().max())), (name, err)
        assert bool((b.mags[name] >= b.grads[name].abs() * (1 - 1e-12)).all()), name


@pytest.mark.parametrize("net", NETS)
def test_amax_equals_torch_pool_indices_on_exact_ties(net):
    """Whole windows that see nothing but a positive bias tie exactly: the first maximum (code 0) wins, as in torch's max-pool."""
    c = _case(net)
    best, ind = F.max_pool2d(torch.relu(c.fwd.z1), 2, 2, return_indices=True)
    assert torch.equal(T.amax_from_pool_indices(ind), c.fwd.amax) and torch.equal(T._cells_last(best), c.fwd.p1)
    w = T._windows(torch.relu(c.fwd.z1))
    tied = (w == w.amax(dim=-1, keepdim=True)).sum(dim=-1) > 1
    positive = tied & (w.amax(dim=-1) > 0)
    assert float(positive.double().mean()) > 0.02, float(positive.double().mean())             # exact ties above zero do occur
    whole = positive & ((w == w.amax(dim=-1, keepdim=True)).sum(dim=-1) == 4)
    assert bool(whole.any()) and not bool((T._cells_last(whole) & c.fwd.ex_p1).any())           # ... and an exact tie is no kink
    assert bool((T._cells_last(whole).long() * c.fwd.amax == 0).all())                          # first maximum: code 0


@pytest.mark.parametrize("net", NETS)
def test_rule_passes_float32_torch(net, capsys):
    c = _case(net)
    rep = []
    T.check_forward(*_f32_forward(c), c.fwd, f"torch32 K9 {net} S{S}", report=rep)
    b32 = T.trunk_backward_f64(c.dense.float(), c.seq[3].weight, c.da2, c.fwd.relu_mask, c.p1r, c.fwd.amax)
    T.check_backward(b32.grads, c.bwd, S, S, f"torch32 K10 {net} S{S}", report=rep)
    with capsys.disabled():
        print("\n" + "\n".join(rep))


@pytest.mark.parametrize("net", NETS)
def test_rule_reports_planted_forward_faults(net, capsys):
    c = _case(net)
    x = c.dense.float()
    w1 = c.seq[0].weight.detach()
    found = {}
    with torch.no_grad():
        z1 = c.seq[0](x)
        # one conv1 tap (dense plane `combined`, ky = 2, kx = 1: input row 26) dropped on output row 25
        ci = 2 if net == "actor" else 0
        combined = c.maps[:, 0]
        z = z1.clone()
        z[:, :, 25, :] -= w1[:, ci, 2, 1].view(1, 8, 1) * combined[:, 26, :].unsqueeze(1)
        found["tap dropped on row 25"] = _worst(T.forward_ratios(*_f32_forward(c, z), c.fwd), ("a2", "p1"))
        if net == "actor":
            # the location stamp's share of output row / column 26, which the pool drops, lands on row / column 25
            loc = x[:, 1:2]
            st = F.conv2d(loc, w1[:, 1:2] - w1[:, 2:3], padding=1)
            z = z1.clone()
            z[:, :, 25, :] += st[:, :, 26, :]
            found["stamp row 26 applied"] = _worst(T.forward_ratios(*_f32_forward(c, z), c.fwd), ("a2", "p1"))
            z = z1.clone()
            z[:, :, :, 25] += st[:, :, :, 26]
            found["stamp column 26 applied"] = _worst(T.forward_ratios(*_f32_forward(c, z), c.fwd), ("a2", "p1"))
        # last maximum wins
        a2, p1, amax, mask = _f32_forward(c)
        w = T._windows(torch.relu(z1))
        last = ((w == w.amax(dim=-1, keepdim=True)).long() * torch.arange(4)).amax(dim=-1)
        found["last maximum wins"] = _worst(T.forward_ratios(a2, p1, T._cells_last(last).to(torch.uint8), mask, c.fwd), ("amax",))
        # the last image of the partly filled round is never written
        a2n, p1n, amaxn, maskn = a2.clone(), p1.clone(), amax.clone(), mask.clone()
        a2n[S - 1], p1n[S - 1], amaxn[S - 1], maskn[S - 1] = float("nan"), float("nan"), 0x77, 0x7777
        found["last image lost"] = _worst(T.forward_ratios(a2n, p1n, amaxn, maskn, c.fwd), ("a2", "p1", "amax", "relu_mask"))
    with capsys.disabled():
        print(f"\nK9 planted faults {net} | " + " ".join(f"{k}: {v:.3g} x" for k, v in found.items()))
    assert all(v > 1.0 for v in found.values()), found


@pytest.mark.parametrize("net", NETS)
def test_rule_reports_planted_backward_faults(net, capsys):
    c = _case(net)
    w2 = c.seq[3].weight.detach()
    run = lambda **kw: T.trunk_backward_f64(**dict(dict(dense=c.dense.float(), w2=w2, da2=c.da2, relu_mask=c.fwd.relu_mask, p1=c.p1r,
                                                        amax=c.fwd.amax), **kw)).grads
    good = run()
    ratio = lambda got, names: _worst(T.backward_ratios(got, c.bwd, S, S), names)
    found = {}
    w2cut = w2.clone()
    w2cut[13:] = 0
    found["dP1 without channels 13..15"] = ratio(run(w2=w2cut), ("dW1", "db1"))
    da = c.da2.clone().view(S, 16, 169)
    da[:, :, 168] = 0
    cut = run(da2=da.view(S, 2704))
    found["dW2 without pixel 168"] = ratio(dict(good, dW2=cut["dW2"]), ("dW2",))
    found["db2 without pixel 168"] = ratio(dict(good, db2=cut["db2"]), ("db2",))
    if net == "actor":
        dW1 = good["dW1"].clone()
        dW1[:, 2] += dW1[:, 1]                                        # `others` convolved as `combined`, the location gather not subtracted
        found["dW1 others without - location"] = ratio(dict(good, dW1=dW1), ("dW1",))
    lost = T.trunk_backward_f64(c.dense.float()[:S - 1], w2, c.da2[:S - 1], c.fwd.relu_mask[:S - 1], c.p1r[:S - 1], c.fwd.amax[:S - 1]).grads
    for name in T.GRADS:
        found[f"last image lost, {name}"] = ratio(dict(good, **{name: lost[name]}), (name,))
    with capsys.disabled():
        print(f"\nK10 planted faults {net} | " + " ".join(f"{k}: {v:.3g} x" for k, v in found.items()))
    assert all(v > 1.0 for v in found.values()), found


def test_rule_reports_a_lost_image_at_the_grid_edge(capsys):
    """S = 2 x 768 + 1, the largest size K10 runs at with 768 resident workgroups, where the allowance is widest: the one image of
    workgroup 0's third trip lost is still far outside it in every block."""
    S, G = 2 * 768 + 1, 768
    actor, _ = T.networks(3)
    maps, own, pred = T.make_batch(S, seed=11)
    dense = T.dense_input(maps, own, pred)
    seq64 = T.F64(actor.actor)
    f = T.trunk_forward_f64(seq64, dense)
    da2 = torch.randn(S, 2704, generator=torch.Generator().manual_seed(5))
    ref = T.trunk_backward_f64(dense, seq64[3].weight, da2, f.relu_mask, f.p1.float(), f.amax)
    last = T.trunk_backward_f64(dense[S - 1:], seq64[3].weight, da2[S - 1:], f.relu_mask[S - 1:], f.p1[S - 1:].float(), f.amax[S - 1:])
    lost = {k: (ref.grads[k] - last.grads[k]).float() for k in T.GRADS}
    kept = {k: ref.grads[k].float() for k in T.GRADS}
    found = dict(T.backward_ratios(lost, ref, S, G))
    with capsys.disabled():
        print(f"\nK10 planted fault actor S{S} | last image lost: " + " ".join(f"{k} {v:.3g} x" for k, v in found.items()))
    assert all(v > 1.0 for v in found.values()), found
    assert all(r <= 1.0 for _, r in T.backward_ratios(kept, ref, S, G))


def test_stamp_images_cover_the_edges():
    pairs = T.stamp_pairs()
    cells = [r * 27 + c for r, c in T.STAMP_CELLS]
    for c in cells:
        assert (c, -1) in pairs and (-1, c) in pairs and (c, c) in pairs
    assert (-1, -1) in pairs and len(pairs) == len(set(pairs)) == 38
    both = [(o, p) for o, p in pairs if o >= 0 and p >= 0 and o != p]
    assert both and all((o // 27) // 2 == (p // 27) // 2 and (o % 27) // 2 == (p % 27) // 2 for o, p in both)    # one pool window
    maps, own, pred = T.make_batch(S, seed=11)
    assert own[:38].tolist() == [p[0] for p in pairs] and pred[:38].tolist() == [p[1] for p in pairs]
    assert bool((maps[:, 0].reshape(S, 729).gather(1, own.clamp(min=0).unsqueeze(1)).squeeze(1)[own >= 0] >= 1).all())
