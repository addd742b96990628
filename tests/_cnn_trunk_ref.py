"""Float64 reference, error model and inputs for the 27 x 27 CNN trunk kernels K9 / K10 (rs_cnn_trunk_forward / rs_cnn_trunk_backward,
csrc/rs_cnn.hip), shared by test_cnn_trunk_f64_gpu.py and its CPU self-checks test_cnn_trunk_ref_cpu.py.  Nothing here calls the
library: the forward pass is torch's float64 convolutions, the pool's first-maximum rule and the backward pass are written out.

The rule, per element:  |got - ref| <= RTOL |ref| + k U mag + TINY,  U = 2^-24, mag the sum of the absolute terms of the element's sum,
after the model of _f64_ref.py's module docstring: a sum of depth n is charged sqrt(n) U of its absolute terms, SAFETY = 2 multiplies
every constant (the model is an expectation), RTOL = 4 U covers the roundings relative to the result itself (the last add, the store).

Forward (K9)
  conv1   a pooled cell's thread adds 36 dense taps (4 planes x 9, one fma each), up to two stamps (the one-hot prediction and location
          channels: one add each) and the bias: depth 39.  The location stamp is the PREPARED difference w_loc - w_others, rounded once
          (+ 1 on its own magnitude, charged to the whole sum).  K1 = 2 (sqrt(39) + 1) = 14.5 on mag1 = |w1| * |x| + |b1|, where the
          kernel's terms at the owner's cell, |w_others| combined + |w_loc - w_others|, exceed the dense input's |w_others| (combined
          - 1) + |w_loc| by at most 2 |w_others|: mag1 has that added.  p1 = max over the window of relu: 1-Lipschitz in the largest
          error of the window, so p1 is held to K1 U max-pool(mag1).
  conv2   72 taps (one fma each) and the bias: depth 73, K2 = 2 sqrt(73) = 17.1 on mag2 = |w2| * p1 + |b2|, plus p1's allowance carried
          through |w2| (linear: no cancellation is assumed between the 72 carried errors).  a2 = relu(z2) is 1-Lipschitz.
  kinks   only the discrete outputs can differ by more than the allowance: amax[s, cell, c] is excused when a window value within the two
          allowances of the winner's is either not exactly equal to it (a near tie; exact ties are decided by the first-maximum rule on
          both sides) or has its pre-activation within its own allowance of 0; bit co of relu_mask[s, cell] when |z2| is within its
          allowance.  The values p1 and a2 are held at every element.

Backward (K10), given the branch data (relu_mask, p1, amax) a linear map of da2: no kinks.  G = min(S, resident workgroups) slab rows,
n = ceil(S / G) images per workgroup.
  dW2, db2   the products dz2 x p1 are exact inputs of the matrix cores; a wave's accumulator takes 11 k-steps of 4 pixels per image
             (depth 44 n), the four waves are added (4), the caller sums G slab rows (G):  k = 2 (sqrt(44 n) + 2 + sqrt(G)) on
             sum |dz2| |p1 patch| (db2: sum |dz2|, the ones column rides in the same accumulators).
  dP1        two fma chains of 117 and 27 taps (output channels 0..12 on the pixel threads, 13..15 on the helper wave), added where they
             are read: (sqrt(117) + 1) U of the sum WITHOUT cancellation |w2|^T |dz2|; it is carried to dW1 / db1 as the magnitude
             bp_mag = sum u |x| with u = (|w2|^T |dz2|) [p1 > 0] placed like dz1:  K_BP = 2 (sqrt(117) + 1) = 23.6 on bp_mag.
  dW1, db1   a thread's fma chain runs over the 13 cells of a pooled row per image (13 n), 16 groups are added (16), the `others`
             channel subtracts the location gather (1), the slab sum (G):  k = 2 (sqrt(13 n) + 4 + 1 + sqrt(G)) on sum |dz1| |x|; the
             stamp gathers (one add per image) are shallower and take the same k.  As in mag1, `others` is convolved as `combined`:
             its magnitude has twice the location channel's added.
The autograd path feeds K10 the kernel's own float32 p1: its allowance enters dW2 as sum |dz2| patches(p1 allowance)."""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
from _f64_ref import U, f64 as F64  # noqa: E402,F401

SAFETY = 2.0                                    # as in _f64_ref.py
RTOL = 4 * U
TINY = 1e-30
K1 = SAFETY * (math.sqrt(36 + 2 + 1) + 1)       # 14.5
K2 = SAFETY * math.sqrt(72 + 1)                 # 17.1
K_BP = SAFETY * (math.sqrt(117) + 1)            # 23.6


def backward_k(S, G):
    """(k of dW1 / db1, k of dW2 / db2) for S images on G = min(S, resident workgroups) slab rows; see the module docstring."""
    n = (S + G - 1) // G
    return SAFETY * (math.sqrt(13 * n) + 4 + 1 + math.sqrt(G)), SAFETY * (math.sqrt(44 * n) + 2 + math.sqrt(G))


# ------------------------------------------------------------------------------------------------ inputs
# (row, column) cells the one-hot stamps are placed on: the four corners, the last cell the pool still sees (25, 25), the dropped row and
# column 26 away from the corners, and an interior cell at each parity of (row, column)
STAMP_CELLS = ((0, 0), (0, 26), (26, 0), (26, 26), (25, 25), (26, 13), (13, 26), (10, 10), (10, 11), (11, 10), (11, 11))


def stamp_pairs():
    """(owner cell, prediction cell) of the stamp images, -1 = none: every STAMP_CELL as owner only, as prediction only and as both
    (owner and prediction on the same cell); owner and prediction on neighbouring cells inside one pool window; neither."""
    flat = [r * 27 + c for r, c in STAMP_CELLS]
    out = [(c, -1) for c in flat] + [(-1, c) for c in flat] + [(c, c) for c in flat]
    w = 10 * 27 + 10                                                   # the pool window of cells (10..11, 10..11)
    out += [(w, w + 1), (w, w + 27), (w, w + 28), (w + 28, w)]
    return out + [(-1, -1)]


def make_batch(S, seed):
    """(maps [S, 4, 27, 27] float32, own [S], pred [S] int64) on the CPU: sparse maps (a tenth of the cells of every plane is set in the
    even images, a fiftieth in the odd ones, where whole pool windows see nothing but the bias: exact ties), combined = small integers
    + the owner, readings of both signs; the
    first images carry stamp_pairs(), the others a random owner (one in sixteen without a recorded position) and, at p = 0.6, a random
    prediction."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(S, 4, 27, 27, generator=g)
    maps = r() * (r() < torch.where(torch.arange(S) % 2 == 0, 0.1, 0.02).view(S, 1, 1, 1))
    maps[:, 1] = (maps[:, 1] * 6 - 3) * (maps[:, 1] != 0)
    maps[:, 0] = torch.round(maps[:, 0] * 3)
    own = torch.randint(0, 729, (S,), generator=g)
    own[torch.rand(S, generator=g) < 1 / 16] = -1
    pred = torch.where(torch.rand(S, generator=g) < 0.6, torch.randint(0, 729, (S,), generator=g), torch.full((S,), -1))
    pairs = stamp_pairs()[:S]
    own[:len(pairs)] = torch.tensor([p[0] for p in pairs])
    pred[:len(pairs)] = torch.tensor([p[1] for p in pairs])
    maps[:, 0].reshape(S, 729).scatter_add_(1, own.clamp(min=0).unsqueeze(1), (own >= 0).float().unsqueeze(1))
    return maps.contiguous(), own, pred


def cell_columns(own, pred, A, agent, seed):
    """cells, pcells [S, A] int64 whose column `agent` is (own, pred); the other columns are random cells."""
    g = torch.Generator().manual_seed(seed)
    S = own.shape[0]
    cells, pcells = torch.randint(0, 729, (S, A), generator=g), torch.randint(-1, 729, (S, A), generator=g)
    cells[:, agent], pcells[:, agent] = own, pred
    return cells.contiguous(), pcells.contiguous()


def dense_input(maps, own=None, pred=None):
    """The float64 dense input: maps.actor_stack_from for an actor (own / pred given), the shared maps for a critic."""
    if own is None:
        return maps.double()
    from radiation_ppo_amd.maps import actor_stack_from
    return actor_stack_from(maps.double(), own.view(-1, 1), pred.view(-1, 1), 0).double()


def networks(seed):
    """(CNNActor, CNNCritic) on the CPU at their initialisation with biases that matter (pool ties on empty regions, ReLU gates)."""
    from radiation_ppo_amd.maps import CNNActor, CNNCritic
    torch.manual_seed(seed)
    actor, critic = CNNActor(), CNNCritic()
    with torch.no_grad():
        for m in (actor.actor, critic.critic):
            m[0].bias.uniform_(-0.05, 0.15)
            m[3].bias.uniform_(-0.1, 0.1)
    return actor, critic


# ------------------------------------------------------------------------------------------------ forward
def _windows(t):
    """[S, C, 27, 27] -> [S, C, 13, 13, 4]: the 2 x 2 pool windows, row-major inside the window (row / column 26 dropped)."""
    S, C = t.shape[:2]
    return t[:, :, :26, :26].reshape(S, C, 13, 2, 13, 2).permute(0, 1, 2, 4, 3, 5).reshape(S, C, 13, 13, 4)


def _cells_last(t):
    """[S, C, 13, 13] -> the kernels' [S, 169, C]."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], 169, t.shape[1]).contiguous()


def _planes(t):
    """[S, 169, C] -> [S, C, 13, 13]."""
    return t.reshape(t.shape[0], 13, 13, t.shape[2]).permute(0, 3, 1, 2)


def first_max(win):
    """(value, code 0..3) over the last dimension, FIRST maximum wins (a later value replaces the best only if it is greater)."""
    best, idx = win[..., 0], torch.zeros(win.shape[:-1], dtype=torch.int64)
    for p in range(1, 4):
        better = win[..., p] > best
        best, idx = torch.where(better, win[..., p], best), torch.where(better, torch.full_like(idx, p), idx)
    return best, idx


def pack_mask(live):
    """[S, 16, 13, 13] bool -> [S, 169] int64, bit co = live[s, co, cell]."""
    return (live.long() << torch.arange(16).view(1, 16, 1, 1)).sum(dim=1).reshape(live.shape[0], 169)


class Forward:
    """trunk_forward_f64's result.  z1 [S, 8, 27, 27], z2 [S, 16, 13, 13]: the pre-activations; p1 [S, 169, 8], amax [S, 169, 8] (uint8),
    relu_mask [S, 169] (int64 holding 16 bits), a2 [S, 2704]: the kernels' outputs in their layouts; mag1 / mag2: the magnitudes of z1 /
    z2; tol_p1 / tol_a2: the allowances of p1 / a2 (RTOL |ref| + k U mag + TINY); tol_p1_abs: the part of tol_p1 that does not depend on
    the result (what is carried on); ex_p1 [S, 169, 8], ex_a2 [S, 2704]: the kink exclusions of amax and of relu_mask's bits."""

    def rows(self, lo, hi):
        out = Forward()
        for k, v in self.__dict__.items():
            setattr(out, k, v[lo:hi])
        return out

    def head(self, S):
        return self.rows(0, S)


def _forward_chunk(w1, b1, w2, b2, dense):
    f = Forward()
    f.z1 = F.conv2d(dense, w1, b1, padding=1)
    f.mag1 = F.conv2d(dense.abs(), w1.abs(), b1.abs(), padding=1)
    if w1.shape[1] == 6:
        f.mag1 = f.mag1 + 2 * F.conv2d(dense[:, 1:2], w1[:, 2:3].abs(), padding=1)
    zw = _windows(f.z1)
    vw = torch.relu(zw)
    best, idx = first_max(vw)
    f.p1, f.amax = _cells_last(best), _cells_last(idx).to(torch.uint8)
    f.z2 = F.conv2d(best, w2, b2, padding=1)
    f.mag2 = F.conv2d(best, w2.abs(), b2.abs(), padding=1)
    f.a2 = torch.relu(f.z2).flatten(1)
    f.relu_mask = pack_mask(f.z2 > 0)
    # allowances and kinks
    alw = K1 * U * _windows(f.mag1)
    carried = alw.amax(dim=-1)
    f.tol_p1_abs = _cells_last(carried)
    f.tol_p1 = RTOL * f.p1 + f.tol_p1_abs + TINY
    tol_z2 = K2 * U * f.mag2 + F.conv2d(carried, w2.abs(), None, padding=1)
    f.tol_a2 = RTOL * f.a2 + tol_z2.flatten(1) + TINY
    al_best = torch.gather(alw, -1, idx.unsqueeze(-1))
    rival = (best.unsqueeze(-1) - vw) <= al_best + alw                 # within the two allowances of the winner (the winner itself too)
    f.ex_p1 = _cells_last((rival & ((vw != best.unsqueeze(-1)) | (zw.abs() <= alw))).any(dim=-1))
    f.ex_a2 = (f.z2.abs() <= tol_z2).flatten(1)
    return f


def trunk_forward_f64(seq, dense, chunk=512):
    """conv3x3 - ReLU - maxpool 2 x 2 - conv3x3 - ReLU - flatten of seq (its layers 0 and 3) on the dense input, in the dtype of the
    input (float64 for the reference), with the kernels' outputs in their layouts, the magnitudes, allowances and kink exclusions
    (class Forward)."""
    dt = dense.dtype
    w1, b1, w2, b2 = (t.detach().to(dt) for t in (seq[0].weight, seq[0].bias, seq[3].weight, seq[3].bias))
    with torch.no_grad():
        parts = [_forward_chunk(w1, b1, w2, b2, dense[lo:lo + chunk]) for lo in range(0, dense.shape[0], chunk)]
    out = Forward()
    for k in parts[0].__dict__:
        setattr(out, k, torch.cat([getattr(p, k) for p in parts]))
    return out


def amax_from_pool_indices(ind):
    """F.max_pool2d(..., 2, 2, return_indices=True)'s indices [S, C, 13, 13] (flat in the 27 x 27 plane) -> codes [S, 169, C]."""
    return _cells_last(((ind // 27) % 2) * 2 + (ind % 27) % 2).to(torch.uint8)


def forward_ratios(a2, p1, amax, relu_mask, ref):
    """[(block, ratio)]: a2 and p1 worst |got - ref| / allowance over EVERY element (inf for a NaN); amax and relu_mask: inf if a code
    / a bit outside the exclusions differs, else 0; the excluded shares of amax and of relu_mask's bits."""
    out = []
    for name, got, want, tol in (("a2", a2, ref.a2, ref.tol_a2), ("p1", p1, ref.p1, ref.tol_p1)):
        g = got.detach().double().cpu().reshape(want.shape)
        r = (g - want).abs() / tol
        r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
        out.append((name, float(r.max())))
    bad = (amax.cpu().reshape(ref.amax.shape) != ref.amax) & ~ref.ex_p1
    out.append(("amax", float("inf") if bool(bad.any()) else 0.0))
    diff = (relu_mask.cpu().long().reshape(ref.relu_mask.shape) & 0xFFFF) ^ ref.relu_mask                     # [S, 169]
    bits = ((diff.unsqueeze(1) >> torch.arange(16).view(1, 16, 1)) & 1).bool().reshape(diff.shape[0], 2704)  # a2's flatten order
    out.append(("relu_mask", float("inf") if bool((bits & ~ref.ex_a2).any()) else 0.0))
    out.append(("excluded amax", float(ref.ex_p1.double().mean())))
    out.append(("excluded mask", float(ref.ex_a2.double().mean())))
    return out


def check_forward(a2, p1, amax, relu_mask, ref, name, report=None):
    """K9's four outputs under the rule; at most 1 % of amax's codes and 1 % of relu_mask's bits may be excluded."""
    ratios = forward_ratios(a2, p1, amax, relu_mask, ref)
    if report is not None:
        report.append(f"{name} | " + " ".join(f"{b} {r:.4f}" for b, r in ratios[:4]) + " " + " ".join(f"{b} {r:.1e}" for b, r in ratios[4:]))
    bad = [(b, r) for b, r in ratios[:4] if not r <= 1.0] + [(b, r) for b, r in ratios[4:] if not r <= 0.01]
    assert not bad, (name, bad)
    return ratios


# ------------------------------------------------------------------------------------------------ backward
GRADS = ("dW1", "db1", "dW2", "db2")


class Backward:
    """trunk_backward_f64's result: grads, mags, bp_mags, carried -- four tensors each (GRADS) in torch's parameter shapes."""

    def __init__(self, cin, dt):
        z = lambda *s: torch.zeros(*s, dtype=dt)
        mk = lambda: dict(dW1=z(8, cin, 3, 3), db1=z(8), dW2=z(16, 8, 3, 3), db2=z(16))
        self.grads, self.mags, self.bp_mags, self.carried = mk(), mk(), mk(), mk()

    def add(self, other):
        for mine, theirs in ((self.grads, other.grads), (self.mags, other.mags), (self.bp_mags, other.bp_mags), (self.carried, other.carried)):
            for k in GRADS:
                mine[k] = mine[k] + theirs[k]
        return self


def _place(t, flat):
    """[S, 8, 169] values at the pixels flat [S, 8, 169] of zero 27 x 27 planes -> [S, 8, 729] (a window's pixels are its own)."""
    return torch.zeros(t.shape[0], 8, 729, dtype=t.dtype).scatter_(2, flat, t)


def trunk_backward_f64(dense, w2, da2, relu_mask, p1, amax, p1_tol=None, chunk=128):
    """The four weight gradients of the trunk from da2 [S, 2704] as linear algebra on the GIVEN branch data, in the dtype of dense:
    dz2 = da2 * mask, db2 = sum dz2, dW2 = sum dz2 x patches(p1), dp1 = conv2^T(dz2) * [p1 > 0], dz1 = dp1 at each window's arg-max
    pixel, dW1 = sum dz1 x patches(dense) in torch's channel order, db1 = sum dz1; with each gradient's magnitude (the same sums over
    absolute terms), the magnitude behind dP1's own rounding (bp_mags) and, with p1_tol [S, 169, 8] (the absolute allowance of a p1 that
    is not the given one), what it adds to dW2 (carried).  Returns a Backward."""
    dt, cin = dense.dtype, dense.shape[1]
    w2 = w2.detach().to(dt)
    out = Backward(cin, dt)
    pos = torch.arange(13)
    with torch.no_grad():
        for lo in range(0, dense.shape[0], chunk):
            x, g = dense[lo:lo + chunk], da2[lo:lo + chunk].to(dt)
            S = x.shape[0]
            m = relu_mask[lo:lo + chunk].long() & 0xFFFF
            live = ((m.unsqueeze(1) >> torch.arange(16).view(1, 16, 1)) & 1).to(dt)             # [S, 16, 169]
            dz2 = g.reshape(S, 16, 169) * live
            pv = _planes(p1[lo:lo + chunk].to(dt))
            P = F.unfold(pv, 3, padding=1)                                                       # [S, 72, 169]
            out.grads["dW2"] += torch.einsum("sop,skp->ok", dz2, P).view(16, 8, 3, 3)
            out.mags["dW2"] += torch.einsum("sop,skp->ok", dz2.abs(), P.abs()).view(16, 8, 3, 3)
            if p1_tol is not None:
                T = F.unfold(_planes(p1_tol[lo:lo + chunk].to(dt)), 3, padding=1)
                out.carried["dW2"] += torch.einsum("sop,skp->ok", dz2.abs(), T).view(16, 8, 3, 3)
            out.grads["db2"] += dz2.sum(dim=(0, 2))
            out.mags["db2"] += dz2.abs().sum(dim=(0, 2))
            gate = (pv > 0).to(dt)
            dp1 = F.conv_transpose2d(dz2.view(S, 16, 13, 13), w2, padding=1) * gate
            u = F.conv_transpose2d(dz2.abs().view(S, 16, 13, 13), w2.abs(), padding=1) * gate
            am = _planes(amax[lo:lo + chunk].long())
            flat = ((2 * pos.view(13, 1) + (am >> 1)) * 27 + 2 * pos.view(1, 13) + (am & 1)).reshape(S, 8, 169)
            dz1, uz1 = _place(dp1.reshape(S, 8, 169), flat), _place(u.reshape(S, 8, 169), flat)
            X = F.unfold(x, 3, padding=1)                                                        # [S, cin * 9, 729]
            out.grads["dW1"] += torch.einsum("sop,skp->ok", dz1, X).view(8, cin, 3, 3)
            out.mags["dW1"] += torch.einsum("sop,skp->ok", dz1.abs(), X.abs()).view(8, cin, 3, 3)
            out.bp_mags["dW1"] += torch.einsum("sop,skp->ok", uz1, X.abs()).view(8, cin, 3, 3)
            out.grads["db1"] += dz1.sum(dim=(0, 2))
            out.mags["db1"] += dz1.abs().sum(dim=(0, 2))
            out.bp_mags["db1"] += uz1.sum(dim=(0, 2))
    if cin == 6:                                     # `others` is convolved as `combined`, the location gather subtracted: see the docstring
        for d in (out.mags, out.bp_mags):
            d["dW1"][:, 2] += 2 * d["dW1"][:, 1]
    return out


def split_slab_sum(g, cin):
    """The summed slab row [8 cin 9 + 8 + 1152 + 16] -> {dW1, db1, dW2, db2} as ConvTrunk.backward splits it."""
    n1 = 8 * cin * 9
    return dict(dW1=g[:n1].view(8, cin, 3, 3), db1=g[n1:n1 + 8], dW2=g[n1 + 8:n1 + 8 + 1152].view(16, 8, 3, 3), db2=g[n1 + 8 + 1152:])


def backward_ratios(got, ref, S, G):
    """[(block, worst |got - ref| / allowed)], allowed = RTOL |ref| + U (k mag + K_BP bp_mag) + carried + TINY with k = backward_k(S, G);
    inf for an element that is not finite.  got: {block: tensor}."""
    k1, k2 = backward_k(S, G)
    out = []
    for name in GRADS:
        g, r = got[name].detach().double().cpu(), ref.grads[name].double()
        assert g.shape == r.shape, (name, g.shape, r.shape)
        k = k1 if name in ("dW1", "db1") else k2
        allowed = RTOL * r.abs() + U * (k * ref.mags[name].double() + K_BP * ref.bp_mags[name].double()) + ref.carried[name].double() + TINY
        ratio = (g - r).abs() / allowed
        ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
        out.append((name, float(ratio.max())))
    return out


def check_backward(got, ref, S, G, name, report=None):
    ratios = backward_ratios(got, ref, S, G)
    if report is not None:
        report.append(f"{name} | " + " ".join(f"{b} {r:.4f}" for b, r in ratios))
    bad = [(b, round(r, 3)) for b, r in ratios if not r <= 1.0]
    assert not bad, (name, bad)
    return ratios


def int16_mask(m):
    """[S, 169] int64 holding 16 bits -> the int16 tensor with the same bits (torch has no uint16 arithmetic)."""
    m = m.long() & 0xFFFF
    return torch.where(m >= 32768, m - 65536, m).to(torch.int16)
