"""The occupancy-aware tiled CNN trunk (rs_cnn_sized_occupancy / _forward_occ / _backward_occ) restated in float64 torch on the CPU:
the flag rule, the empty-unit rule with the owner's cells, and the empty unit's backward algebra (the S and R sums of dZ2 with c1 and
w2 folded in); and the inputs the CPU and the GPU tests share.  Nothing here calls the library.

A unit is (image, tile of 16 x 16 pooled cells); tile k covers the pixels [32 k, 32 k + 32) of an axis and its forward window the pixels
[32 k - 3, 32 k + 35), clipped to the map."""
import torch
import torch.nn.functional as F

TS = 16


def tiles_per_side(M: int) -> int:
    return (M // 2 + TS - 1) // TS


def window(M: int, k: int):
    """the clipped forward-window span of tile k along one axis"""
    return max(0, 2 * TS * k - 3), min(M, 2 * TS * k + 2 * TS + 3)


def flags_ref(maps: torch.Tensor) -> torch.Tensor:
    """uint8 [S, tiles]: bit 0 = the unit's window holds an element != 0.0 (a NaN does, -0.0 does not)"""
    S, M = maps.shape[0], maps.shape[-1]
    nt = tiles_per_side(M)
    out = torch.zeros(S, nt * nt, dtype=torch.uint8)
    for ty in range(nt):
        r0, r1 = window(M, ty)
        for tx in range(nt):
            c0, c1 = window(M, tx)
            out[:, ty * nt + tx] = (maps[:, :, r0:r1, c0:c1] != 0.0).flatten(1).any(dim=1).to(torch.uint8)
    return out


def cell_in_window(at: torch.Tensor, M: int) -> torch.Tensor:
    """bool [S, tiles]: the flat cell index at [S] (-1: none) lies in the unit's window"""
    nt = tiles_per_side(M)
    out = torch.zeros(at.shape[0], nt * nt, dtype=torch.bool)
    r, c = torch.div(at, M, rounding_mode="floor"), at % M
    for ty in range(nt):
        r0, r1 = window(M, ty)
        for tx in range(nt):
            c0, c1 = window(M, tx)
            out[:, ty * nt + tx] = (at >= 0) & (r >= r0) & (r < r1) & (c >= c0) & (c < c1)
    return out


def empty_ref(maps, cells, pcells, agent: int) -> torch.Tensor:
    """bool [S, tiles]: the unit is empty for this network (agent < 0: a critic, no owner cells)"""
    M = maps.shape[-1]
    e = flags_ref(maps) == 0
    if agent >= 0:
        e &= ~cell_in_window(cells[:, agent], M) & ~cell_in_window(pcells[:, agent], M)
    return e


def unit_masks(empty: torch.Tensor, M: int) -> torch.Tensor:
    """[S, 1, P, P] float64: 1 on the pooled cells (= conv2 output pixels) of the empty units"""
    S, P, nt = empty.shape[0], M // 2, tiles_per_side(M)
    m = empty.view(S, 1, nt, nt).double().repeat_interleave(TS, dim=2).repeat_interleave(TS, dim=3)
    return m[:, :, :P, :P].contiguous()


def empty_unit_grads(dz2: torch.Tensor, em: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor):
    """The empty units' contributions (dW1, db1, dW2, db2) by the shortcut.  dz2 [S, 16, P, P]: dL/d(conv2 pre-activation) of EVERY
    pixel (zero outside the map by construction); em: unit_masks.  c1[ci] = max(0 + b1[ci], 0) is their P1 inside the map:
      db2[co] = sum over their pixels of dz2;  dW2[co][ci][ky][kx] = c1[ci] S[co][ky][kx],  S = sum of dz2[co][y][x] over their pixels
      whose neighbour (y + ky - 1, x + kx - 1) is in the map;  db1[ci] = [c1 > 0] sum w2[co][ci][ky][kx] R[co][ky][kx],  R = sum over their
      cells (cy, cx) of dz2[co][cy - ky + 1][cx - kx + 1];  dW1 = 0."""
    P = dz2.shape[-1]
    c1 = torch.clamp(0.0 + b1, min=0.0)
    own = dz2 * em                                              # the empty units' own pixels
    in_map = F.pad(torch.ones(P, P, dtype=dz2.dtype), (1, 1, 1, 1))
    halo = F.pad(dz2, (1, 1, 1, 1))                             # dz2 with its zero ring
    S = torch.zeros(16, 3, 3, dtype=dz2.dtype)
    R = torch.zeros(16, 3, 3, dtype=dz2.dtype)
    for ky in range(3):
        for kx in range(3):
            S[:, ky, kx] = (own * in_map[ky:ky + P, kx:kx + P]).sum(dim=(0, 2, 3))
            # cell (cy, cx) reads dz2 at (cy - ky + 1, cx - kx + 1) = halo (cy + 2 - ky, cx + 2 - kx)
            R[:, ky, kx] = (halo[:, :, 2 - ky:2 - ky + P, 2 - kx:2 - kx + P] * em).sum(dim=(0, 2, 3))
    db2 = own.sum(dim=(0, 2, 3))
    dW2 = c1.view(1, 8, 1, 1) * S.view(16, 1, 3, 3)
    db1 = (c1 > 0).to(dz2.dtype) * (w2 * R.view(16, 1, 3, 3)).sum(dim=(0, 2, 3))
    return None, db1, dW2, db2


def trunk_grads_with_shortcut(seq64, dense64, empty, wgt64):
    """The four conv gradients of L = sum(a2 * wgt) for the float64 trunk seq64[0:6] on the dense stack, the occupied units' part by
    autograd and the empty units' part by empty_unit_grads.  A unit's part: dW2 / db2 over its conv2 pixels, dW1 / db1 through its
    pooled cells.  Autograd is given twin parameters that act on the occupied units only; the twins' gradients are that part."""
    M = dense64.shape[-1]
    P = M // 2
    em = unit_masks(empty, M)
    w1, b1, w2, b2 = (seq64[0].weight.detach(), seq64[0].bias.detach(), seq64[3].weight.detach(), seq64[3].bias.detach())
    tw = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    p1 = F.max_pool2d(torch.relu(F.conv2d(dense64, w1, b1, padding=1)), 2, 2)
    p1_twin = F.max_pool2d(torch.relu(F.conv2d(dense64, tw[0], tw[1], padding=1)), 2, 2)
    p1_mix = em * p1 + (1 - em) * p1_twin                       # the gradient reaches conv1's twins through the occupied units' cells
    z2 = em * F.conv2d(p1_mix, w2, b2, padding=1) + (1 - em) * F.conv2d(p1_mix, tw[2], tw[3], padding=1)
    a2 = torch.relu(z2)
    (a2.flatten(1) * wgt64).sum().backward()
    dz2 = (wgt64.view(-1, 16, P, P) * (z2 > 0)).detach()
    short = empty_unit_grads(dz2, em, b1, w2)
    return [t.grad if s is None else t.grad + s for t, s in zip(tw, short)], a2.detach()


# ---- the shared inputs
KINDS = ("cluster", "zero", "dense", "loc_ring", "pc_ring", "edge")


def occ_inputs(M: int, S: int, A: int, agent: int, seed: int, kinds=KINDS):
    """maps [S, 4, M, M] float32, cells / pcells [S, A] int64 on the CPU; image i is of kind kinds[i % len(kinds)]:
      cluster   one occupied unit: a non-zero at pixel (0, 0) for two tiles a side (tile 1's window starts at pixel 29), at five tiles a
                side a cluster over the pixels 32 k + 3 .. 32 k + 28 of tile k = 2 on both axes, which lies in no other window; the
                owner's cell on it, no prediction cell
      zero      nothing, no cells: every unit empty
      dense     non-zero everywhere
      loc_ring  the cluster, and the owner's cell at pixel (30, 5) resp. (30, 40): inside tile row 0, in the 3-pixel ring of tile row 1
      pc_ring   the same with the prediction cell there and no location
      edge      a non-zero at pixel (M - 1, 0), the row an odd M drops from the pool; the owner's cell on it
    The other owners' cells are random."""
    g = torch.Generator().manual_seed(seed)
    nt = tiles_per_side(M)
    maps = torch.zeros(S, 4, M, M)
    cells = torch.randint(0, M * M, (S, A), generator=g)
    pcells = torch.randint(0, M * M, (S, A), generator=g)
    ring = 30 * M + (5 if nt <= 2 else 40)
    for i in range(S):
        kind = kinds[i % len(kinds)]
        if kind in ("cluster", "loc_ring", "pc_ring"):
            if nt <= 2:
                maps[i, :, 0, 0] = torch.tensor([2.0, -1.5, 0.25, 1.0])
                on = 0
            else:
                lo, hi = 32 * 2 + 3, 32 * 2 + 29
                v = torch.randn(4, hi - lo, hi - lo, generator=g) * (torch.rand(4, hi - lo, hi - lo, generator=g) < 0.5)
                v[:, 0, 0] = torch.tensor([1.0, -2.0, 0.5, 1.0])
                maps[i, :, lo:hi, lo:hi] = v
                on = (lo + 7) * M + lo + 9
            cells[i, agent], pcells[i, agent] = on, -1
            if kind == "loc_ring":
                cells[i, agent], pcells[i, agent] = ring, on
            if kind == "pc_ring":
                cells[i, agent], pcells[i, agent] = -1, ring
        elif kind == "zero":
            cells[i, agent], pcells[i, agent] = -1, -1
        elif kind == "dense":
            maps[i] = torch.rand(4, M, M, generator=g) + 0.5
            maps[i, 1] -= 2.0
        elif kind == "edge":
            maps[i, :, M - 1, 0] = torch.tensor([1.0, 0.75, -0.5, 1.0])
            cells[i, agent], pcells[i, agent] = (M - 1) * M, -1
        else:
            raise ValueError(kind)
    return maps.contiguous(), cells.contiguous(), pcells.contiguous()


def set_biases(seq, seed: int):
    """biases of both signs, as tests/test_cnn_sized_trunk_gpu.py::_modules sets them: conv1 channels with c1 = 0 and with c1 > 0"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        seq[0].bias.copy_(torch.rand(8, generator=g) * 0.2 - 0.05)
        seq[3].bias.copy_(torch.rand(16, generator=g) * 0.2 - 0.1)
        seq[0].bias[0], seq[0].bias[1] = -0.04, 0.12              # both signs whatever the draw
