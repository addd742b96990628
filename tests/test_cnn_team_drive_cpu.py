"""What the GPU suites of the RAD-TEAM (CNN) team kernels trust, held to planted faults without a GPU: the one copy of the float64 rule
(tests/_cnn_team_ref.py: reference, value_ratios) on the float32 torch composition of a small team at depth 256 (P = 4) and at 2704, the
sentinel and guard checks and the family records of tests/_cnn_team_drive.py, and both lists of one-hot positions
(tests/_cnn_sized_team_ref.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_sized_team_ref as S  # noqa: E402
import _cnn_team_drive as D  # noqa: E402
import _cnn_team_ref as T  # noqa: E402
import _f64_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("fam,key,depth", [(D.SIZED, (4, 2), 256), (D.FAMILY27, 3, 2704)], ids=["depth256", "depth2704"])
def test_the_rule_passes_the_float32_composition_and_sees_a_moved_y1_and_a_moved_value(fam, key, depth):
    t = fam.team(key)
    k1 = fam.k1(t.flat)
    assert t.flat == depth and k1 == S.k1(depth) and (depth != 2704 or k1 == T.K1)
    N, n, j = t.N, t.N // 2, 7
    alive = T.alive_for(t, N)
    # ---- an actor's rows: reference
    seq, a2, u = t.actors[0].actor, T.trunk_cpu(t)[0], t.u[:, 0]
    ref = T.reference(seq, a2, u, k1)
    y1, act, logp, act8 = T.torch32(seq, a2, u, alive)
    q = T.ratios(ref, u, alive, act, logp, act8, y1=y1)
    assert T.passes(q) and q["y1"] < 1.0 and q["logp"] < 1.0, q
    moved = y1.double().clone()
    moved[n, j] += 2.0 * ref.y1_allow[n, j]
    qm = T.ratios(ref, u, alive, act, logp, act8, y1=moved)
    assert 1.0 < qm["y1"] < 3.1 and not T.passes(qm), qm
    if fam is D.SIZED:                                                # the any-side module's one-line reference is this one
        assert torch.equal(S.reference(seq, a2, u).y1_allow, ref.y1_allow) and torch.equal(S.reference(seq, a2, u).lp_allow, ref.lp_allow)
    else:
        assert torch.equal(T.reference(seq, a2, u).lp_allow, ref.lp_allow)                          # K1 is the default
    # ---- a critic's rows: value_ratios, through the same first layer
    crit = D.critics(1, 5, t.M)[0].critic
    with torch.no_grad():
        a2c = crit[:6](t.maps)
        y1c = torch.nn.functional.linear(a2c, crit[6].weight, crit[6].bias)
        v = crit[7:11](y1c)
        s64 = R.f64(crit)
        ref_y1, _, y1_allow, through = T.first_layer(s64, a2c, k1)
        val, mag3, carried = R.cnn_head_f64(s64, ref_y1)
        allow = T.output_allow(val, through, carried, mag3, k1)
    qy, qv = T.value_ratios(crit, a2c, v, y1c, k1)
    assert 0.0 <= qy < 1.0 and 0.0 <= qv < 1.0, (qy, qv)
    moved_y1, moved_v = y1c.double().clone(), v.double().clone()
    moved_y1[n, j] += 2.0 * y1_allow[n, j]
    moved_v[n] += 2.0 * allow[n]
    qy_m, qv_same = T.value_ratios(crit, a2c, v, moved_y1, k1)
    qy_same, qv_m = T.value_ratios(crit, a2c, moved_v, y1c, k1)
    assert 1.0 < qy_m < 3.1 and 1.0 < qv_m < 3.1 and qv_same == qv and qy_same == qy, (qy_m, qv_m)
    assert T.value_passes(qy, qv) and not T.value_passes(qy_m, qv) and not T.value_passes(qy, qv_m)
    with pytest.raises(AssertionError):                              # a NaN is no small error
        T.value_ratios(crit, a2c, torch.where(torch.arange(N) == n, float("nan"), v.squeeze(-1)), y1c, k1)


# ------------------------------------------------------------------------------------------------ sentinels, guards, bits
def test_a_single_changed_guard_float_and_a_negative_zero_are_seen():
    buf = torch.full((12,), D.SENTINEL)
    assert D.is_sentinel(buf) and D.guards_intact(buf, 4, 8)
    buf[5] = 1.0                                                     # between the guards
    assert not D.is_sentinel(buf) and D.guards_intact(buf, 4, 8)
    for at in (0, 3, 8, 11):
        spoilt = buf.clone()
        spoilt[at] = torch.nextafter(spoilt[at], torch.tensor(0.0))  # one ulp
        assert not D.guards_intact(spoilt, 4, 8), at
    rows = torch.full((6, 32), D.SENTINEL)                           # a [rows, 32] buffer with one guard row on each side
    assert D.guards_intact(rows, 1, -1)
    rows[-1, 31] = 0.0
    assert not D.guards_intact(rows, 1, -1)
    zero, minus = torch.zeros(4), torch.zeros(4)
    minus[2] = -0.0
    assert torch.equal(zero, minus) and not torch.equal(D.bits(zero), D.bits(minus))
    assert D.ptr(None) is None and D.ptr(zero) == zero.data_ptr()


# ------------------------------------------------------------------------------------------------ the one-hot positions
def test_onehot_positions_of_the_27_by_27_depth():
    ks = S.onehot_ks(13)
    assert {0, 15, 16, 31, 32, 671, 672, 675, 676, 2703} <= set(ks) and ks == sorted(set(ks)) and ks[-1] == T.FLAT - 1


@pytest.mark.parametrize("sl", [1024, 2048, 4096, 8192])
def test_sliced_onehot_positions_hold_both_sides_of_every_slice_boundary(sl):
    for P in (4, 5, 15, 32, 73):
        flat = S.flat_of(P)
        ks = S.onehot_ks_sliced(flat, sl)
        assert ks == sorted(set(ks)) and ks[0] == 0 and ks[-1] == flat - 1
        for s in range(1, -(-flat // sl)):
            assert s * sl - 1 in ks and s * sl in ks, (P, s)
        if flat > sl:
            assert {sl - 1, sl, sl // 4 - 1, sl // 4, 15, 16, 31, 32} <= set(ks), P
    assert S.flat_of(32) % sl == 0                                   # a depth that is a whole number of slices is among them


# ------------------------------------------------------------------------------------------------ the family records
def test_both_families_name_entry_points_the_header_declares():
    from radiation_ppo_amd import _lib
    declared = {name for name, _, _ in _lib.SYMBOLS}
    roles = ("team_trunk", "critic_trunk", "one_trunk", "eval_head", "step_head")
    for fam in (D.FAMILY27, D.SIZED):
        assert tuple(fam.names) == roles and set(fam.names.values()) <= declared, fam.label
        assert all(callable(getattr(fam, r)) for r in roles + ("team", "case", "k1", "critic_seed", "weights"))
    assert not set(D.FAMILY27.names.values()) & set(D.SIZED.names.values())
    assert {"rs_cnn_head", "rs_cnn_trunk_prepare", "rs_cnn_sized_team_head_scratch_floats"} <= declared
