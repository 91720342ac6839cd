"""CPU: the float64 reference of the PointNet encoder's training path (tests/pointnet_train_ref.py) is pinned against torch.autograd
through the project's own layers and against the oracle's pools and scatter, the seeded inputs prepared for the GPU tests
(tests/pointnet_train_cases.py) are shown to hold the edges they claim, LocalPoolPointnet._fused_mlp_fits() is held to the kernels'
LDS arithmetic, and the gate of tests/test_pointnet_train_f64_gpu.py is shown to bite on the reference alone."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointnet_train_cases as cases
import pointnet_train_ref as ref
from decode_train_ref import gate_ratio

GATE = 8.0
F64 = torch.float64


def _close(got, want, what):
    want = want.detach()
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got.double() - want.double()).abs().max()) if want.numel() else 0.0
    assert err <= 1e-12 * scale, f"{what}: {err:.3e} of {scale:.3e}"


def _block64(width, w):
    from vtaco_amd.layers import ResnetBlockFC
    C1, C2, H, O, short = width
    blk = ResnetBlockFC(C1 + C2, O, H).double()
    assert (blk.shortcut is not None) == short
    with torch.no_grad():
        blk.fc_0.weight.copy_(w["w0"]); blk.fc_0.bias.copy_(w["b0"]); blk.fc_1.weight.copy_(w["w1"]); blk.fc_1.bias.copy_(w["b1"])
        if short:
            blk.shortcut.weight.copy_(w["ws"])
    return blk


# ---- 1. the restatements against autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", cases.with_bound_width(), ids=str)
def test_block_reference_equals_autograd_through_the_layer(width):
    C1, C2, H, O, short = width
    N = 129
    w = cases.block_weights(width)
    x1, x2, dout = cases.block_rows(N, width)
    blk = _block64(width, w)
    x = (torch.cat([x1, x2], 1) if C2 else x1).double().requires_grad_()
    out = blk(x)
    out.backward(dout.double())
    _close(ref.resblock_fwd(x1, x2, w["w0"], w["b0"], w["w1"], w["b1"], w["ws"]), out.detach(), "out")
    h = ref.resblock_hidden(x1, x2, w["w0"], w["b0"])
    _close(ref.resblock_act(x1, x2, w["w0"], w["b0"]), torch.relu(blk.fc_0(torch.relu(x.detach()))), "act")
    dx1, dx2, dh = ref.resblock_bwd(x1, x2, w["w0"], w["w1"], w["ws"], dout, h > 0)
    _close(torch.cat([dx1, dx2], 1) if C2 else dx1, x.grad, "dx")
    act = torch.relu(h)
    dw1, db1 = ref.rows_wgrad(dout, act)
    dw0, db0 = ref.rows_wgrad(dh, x1, x2, relu_x=True)
    for got, want, what in ((dw1, blk.fc_1.weight.grad, "dW1"), (db1, blk.fc_1.bias.grad, "db1"), (dw0, blk.fc_0.weight.grad, "dW0"),
                            (db0, blk.fc_0.bias.grad, "db0")):
        _close(got, want, what)
    if short:
        _close(ref.rows_wgrad(dout, x1, x2)[0], blk.shortcut.weight.grad, "dWs")
    # the bounds dominate the values they bound
    assert bool((ref.resblock_fwd(x1, x2, w["w0"], w["b0"], w["w1"], w["b1"], w["ws"], absolute=True) >= out.detach().abs() - 1e-12).all())
    bx1, _, bh = ref.resblock_bwd(x1, x2, w["w0"], w["w1"], w["ws"], dout, h > 0, absolute=True)
    assert bool((bx1 >= dx1.abs() - 1e-12).all()) and bool((bh >= dh.abs() - 1e-12).all())


@pytest.mark.parametrize("Cin,Cout", cases.LINEAR)
def test_linear_reference_equals_autograd(Cin, Cout):
    N = 257
    x, w, b = cases.linear_case(N, Cin, Cout)
    lin = nn.Linear(Cin, Cout).double()
    with torch.no_grad():
        lin.weight.copy_(w); lin.bias.copy_(b)
    xd = x.double().requires_grad_()
    out = lin(xd)
    g = torch.randn(N, Cout, generator=torch.Generator().manual_seed(Cin))
    out.backward(g.double())
    _close(ref.linear_rows(x, w, b), out.detach(), "out")
    _close(ref.linear_rows(g, w.t()), xd.grad, "dx")
    dW, db = ref.rows_wgrad(g, x)
    _close(dW, lin.weight.grad, "dW")
    _close(db, lin.bias.grad, "db")


def test_pool_and_scatter_references_equal_the_oracle_under_autograd():
    from oracle import vtaco_oracle as orc
    g = torch.Generator().manual_seed(5)
    B, T, C, R = 2, 301, 24, 4
    p = (torch.rand(B, T, 3, generator=g) - 0.5)
    idx = cases.cell_ids32(p.numpy(), R)
    assert bool((idx == orc.voxel_index(p, R, 0.1)).all())
    feat = torch.randn(B, T, C, generator=g)          # (no ties: torch's amax backward would split a tie's gradient)
    grad = torch.randn(B, T, C, generator=g)
    f = feat.double().requires_grad_()
    out = orc.segment_pool_max(f, idx)
    out.backward(grad.double())
    got, arg = ref.pool_max(feat, idx)
    assert torch.equal(got.double(), out.detach())
    _close(ref.pool_max_bwd(grad, arg, idx), f.grad, "pool_max_bwd")
    f.grad = None
    out = orc.segment_pool_mean(f, idx)
    out.backward(grad.double())
    _close(ref.pool_mean(feat, idx), out.detach(), "pool_mean")
    _close(ref.pool_mean(grad, idx), f.grad, "pool_mean backward (self-adjoint)")
    f.grad = None
    grid = orc.scatter_mean_grid(f, idx, R)
    gg = torch.randn(B, C, R ** 3, generator=g)
    grid.backward(gg.double().view(B, C, R, R, R))
    _close(ref.scatter_mean(feat, idx, R ** 3), grid.detach().view(B, C, -1), "scatter_mean")
    _close(ref.scatter_mean(feat, idx, R ** 3, channels_last=True), grid.detach().view(B, C, -1).permute(0, 2, 1), "scatter_mean cl")
    _close(ref.scatter_mean_bwd(gg, idx), f.grad, "scatter_mean_bwd")
    _close(ref.scatter_mean_bwd(gg.permute(0, 2, 1).contiguous(), idx, channels_last=True), f.grad, "scatter_mean_bwd cl")
    # the partitions' sums
    idxs = [cases.cell_ids32(p.numpy(), 3, plane=k) for k in cases.PLANES]
    f.grad = None
    out = sum(orc.segment_pool_max(f, i) for i in idxs)
    out.backward(grad.double())
    _close(ref.pool_max_sum(feat, idxs), out.detach(), "pool_max_sum")
    _close(ref.pool_max_sum_bwd(grad, [ref.pool_max(feat, i)[1] for i in idxs], idxs), f.grad, "pool_max_sum_bwd")
    f.grad = None
    planes = torch.cat([orc.scatter_mean_grid(f, i, 3)[:, :, :1].reshape(B, C, -1)[:, :, :9] for i in idxs], 0)   # ids < 9: the first 9 cells
    gp = torch.randn(3 * B, C, 9, generator=g)
    planes.backward(gp.double())
    _close(ref.scatter_mean_multi(feat, idxs, 9), planes.detach(), "scatter_mean_multi")
    _close(ref.scatter_mean_multi_bwd(gp, idxs), f.grad, "scatter_mean_multi_bwd")


def test_arg_max_is_the_first_maximum_in_point_order():
    _, ids = cases.pool_points()
    feat, _ = cases.pool_features(8)
    out, arg = ref.pool_max(feat, ids)
    f = feat.numpy()
    for b in range(2):
        for t in range(0, cases.POOL_T, 17):
            mem = np.nonzero(ids[b].numpy() == int(ids[b, t]))[0]
            for c in range(8):
                col = f[b, mem, c]
                assert out[b, t, c] == col.max() and int(arg[b, t, c]) == int(mem[np.nonzero(col == col.max())[0][0]])


# ---- 2. the cases hold what they claim -----------------------------------------------------------------------------------------------
def test_pool_points_hold_the_constructed_segments():
    pts, ids = cases.pool_points()
    T = cases.POOL_T
    assert pts.shape == (2, T, 3) and T <= 1100 and T % 32 != 0
    assert bool((cases.cell_ids32(pts.numpy(), cases.POOL_R) == ids).all())          # the kernels' arithmetic puts them there
    cells, counts = torch.unique(ids[0], return_counts=True)                          # ascending ids = the sorted order
    assert tuple(cells.tolist()) == cases.SCENE0_CELLS and tuple(counts.tolist()) == cases.SCENE0_LENGTHS
    assert {1, 2, 31, 32, 33, 64, 65} <= set(counts.tolist())
    start = np.concatenate([[0], np.cumsum(counts.numpy())])
    k = cases.ALIGNED_LONG
    assert counts[k] > 32 and start[k] % 32 == 0
    k = cases.OFFSET31_LONG
    assert counts[k] > 32 and start[k] % 32 == 31
    k = cases.LAST_LONG
    assert counts[k] > 32 and start[k + 1] == T
    assert bool((ids[1] == cases.SCENE1_CELL).all())
    assert not bool((ids[0][1:] >= ids[0][:-1]).all())                                 # shuffled: point order is not the sorted order
    # the planes regroup the same points; every plane keeps short and long cells
    for plane in cases.PLANES:
        n = torch.unique(cases.cell_ids32(pts.numpy(), cases.POOL_R, plane=plane)[0], return_counts=True)[1]
        assert int(n.min()) <= 32 < int(n.max()) and int(n.sum()) == T


def test_tie_rows_are_ties_at_the_maximum():
    _, ids = cases.pool_points()
    groups = cases.tie_rows(ids)
    lengths = []
    for C in (8, 320):
        feat, grad = cases.pool_features(C)
        assert bool((grad.view(-1, C)[::7] == 0).all()) and bool((grad.view(-1, C)[1::7] != 0).any())
        out, arg = ref.pool_max(feat, ids)
        for b in range(2):
            for grp in groups[b]:
                assert len(set(ids[b, grp].tolist())) == 1
                n = int((ids[b] == ids[b, grp[0]]).sum())
                lengths.append(n)
                for t in grp[1:]:
                    assert torch.equal(feat[b, t], feat[b, grp[0]])
                won = out[b, grp[0]] == feat[b, grp[0]]
                assert float(won.float().mean()) >= 0.9          # the tie decides the arg-max in most channels
                assert bool((arg[b, grp[0]][won] == min(grp)).all())
    assert min(lengths) <= 32 < max(lengths)


def test_widths_take_the_kernels_they_are_listed_for():
    ws = cases.with_bound_width()
    mfma = [w for w in ws if cases.takes_mfma(*w[:4])]
    assert mfma == [(64, 0, 32, 32, True), (32, 32, 32, 32, True), (32, 0, 32, 32, False)]
    for w in ws:
        C1, C2, H, O, short = w
        assert short or C1 + C2 == O
        assert cases.fwd_lds_bytes(C1 + C2, H, O, short) <= cases.LDS_LIMIT
        if w not in mfma:
            assert cases.bwd_fma_lds_bytes(C1 + C2, H, O, short) <= cases.LDS_LIMIT
    assert 256 % 24 == 16 and cases.bwd_rows(40, 40, 40, 40) == 3 and 48 > 32 > 24          # idle threads, three rows, K straddles a tile
    assert 25 % 4 and 17 % 4 and 9 % 4 and (47, 47, 47, 47, True) in ws and (48, 0, 24, 48, False) in ws
    h = cases.HIDDEN_BOUND
    assert (h, h, h, h, True) in ws
    for Cin, Cout in cases.LINEAR:
        assert Cout <= 256 and 4 * (Cin * (Cout | 1) + (256 // Cout) * Cin) <= 160 * 1024          # (64, 256) needs 64.5 KiB: past the default allowance


def test_row_counts_cross_every_boundary():
    cus = 256
    for w in cases.with_bound_width():
        C1, C2, H, O, _ = w
        ns = cases.row_counts(w, cus)
        assert ns[0] == 1 and max(ns) < 40000
        for r in (cases.fwd_rows(H, O), cases.bwd_rows(C1, C2, H, O)):
            assert max(r - 1, 1) in ns and r + 1 in ns
        assert {31, 33, 127, 129, 255, 257, 1023, 1025, 9 * 1024 + 37} <= set(ns)
        assert cases.fwd_cap(cus, H, O) + 69 in ns and cases.bwd_cap(cus, C1, C2, H, O) + 69 in ns
    assert (cases.TEN_CHUNKS + 1023) // 1024 == 10                                       # eight partials at a time plus a tail of two
    assert cases.fwd_cap(cus, 32, 32) == 8192 and cases.bwd_cap(cus, 32, 32, 32, 32) == 32768
    n = cases.bwd_cap(cus, 32, 32, 32, 32) + 69
    tiles = (n + 31) // 32 - cus * 4
    assert tiles == 3 and n % 32 == 5                                                     # second round: three live tiles (the last ragged), one dead wave
    for _, Cout in cases.LINEAR:
        assert 4 * cus * (256 // Cout) + 69 in cases.linear_row_counts(Cout, cus)


@pytest.mark.parametrize("width", cases.with_bound_width(), ids=str)
def test_pre_activations_are_negative_about_half_of_the_time(width):
    w = cases.block_weights(width)
    x1, x2, dout = cases.block_rows(1025, width)
    h = ref.resblock_hidden(x1, x2, w["w0"], w["b0"])
    share = float((h < 0).double().mean())
    assert 0.3 <= share <= 0.7, share
    assert bool((dout[::7] == 0).all()) and bool((dout[1::7] != 0).all())
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    assert 0.3 <= float((x < 0).double().mean()) <= 0.7


# ---- 3. the admitted widths ----------------------------------------------------------------------------------------------------------
def test_fused_mlp_fits_is_the_kernels_lds_arithmetic(monkeypatch):
    from vtaco_amd.encoder.pointnet import LocalPoolPointnet
    monkeypatch.delenv("VTACO_RESBLOCK_MFMA", raising=False)
    assert cases.fwd_lds_bytes(112, 56, 56, True) == 66528
    assert cases.bwd_fma_lds_bytes(96, 48, 48, True) == 67392 and cases.bwd_fma_lds_bytes(112, 56, 56, True) == 91168
    assert cases.bwd_fma_lds_bytes(94, 47, 47, True) <= cases.LDS_LIMIT
    assert cases.HIDDEN_BOUND == 47
    for h in range(1, 65):
        net = LocalPoolPointnet(c_dim=8, dim=3, hidden_dim=h, grid_resolution=4, plane_type='grid')
        assert net._fused_mlp_fits() == cases.hidden_fits(h) == (h <= 47), h
    # with the MFMA backward switched off, hidden 32 takes the FMA kernel, which holds it
    monkeypatch.setenv("VTACO_RESBLOCK_MFMA", "0")
    assert LocalPoolPointnet(c_dim=8, dim=3, hidden_dim=32, grid_resolution=4, plane_type='grid')._fused_mlp_fits()


# ---- 4. the gate bites ------------------------------------------------------------------------------------------------------------------
def _ratio(got32, perturbed):
    p64, p32, pb = perturbed
    return gate_ratio(got32, p64, p32, pb)[0]


def test_the_gate_bites_on_the_dense_perturbations():
    width = (24, 24, 24, 24, True)
    w = cases.block_weights(width)
    N = 1025
    x1, x2, dout = cases.block_rows(N, width)
    h = ref.resblock_hidden(x1, x2, w["w0"], w["b0"])
    # the unperturbed float32 reference passes its own gate
    args = (x1, x2, w["w0"], w["b0"], w["w1"], w["b1"], w["ws"])
    good = ref.forms(ref.resblock_fwd, *args)
    assert _ratio(good[1], good) <= 1.0
    # x1 and x2 swapped in the concat
    assert _ratio(good[1], ref.forms(ref.resblock_fwd, *args, swap=True)) > GATE
    # the last row of an odd N left out of dW
    dh = ref.resblock_bwd(x1, x2, w["w0"], w["w1"], w["ws"], dout, h > 0, dtype=torch.float32)[2]
    full32 = ref.rows_wgrad(dh, x1, x2, relu_x=True, dtype=torch.float32)
    cut = ref.forms(ref.rows_wgrad, dh, x1, x2, relu_x=True, rows=N - 1)
    for k in range(2):
        assert _ratio(full32[k], tuple(f[k] for f in cut)) > GATE, k
    whole = ref.forms(ref.rows_wgrad, dh, x1, x2, relu_x=True)
    for k in range(2):
        assert _ratio(full32[k], tuple(f[k] for f in whole)) <= 1.0
    # '>=' in the h mask: taken from act = relu(h), that is every element
    act = torch.relu(h)
    bargs = (x1, x2, w["w0"], w["w1"], w["ws"], dout)
    good32 = ref.resblock_bwd(*bargs, act > 0, dtype=torch.float32)
    bad = ref.forms(ref.resblock_bwd, *bargs, act >= 0)
    for k in (0, 1, 2):
        assert _ratio(good32[k], tuple(f[k] for f in bad)) > GATE, k
    ok = ref.forms(ref.resblock_bwd, *bargs, act > 0)
    for k in (0, 1, 2):
        assert _ratio(good32[k], tuple(f[k] for f in ok)) <= 1.0


def test_the_gate_bites_on_the_pool_perturbations():
    _, ids = cases.pool_points()
    feat, grad = cases.pool_features(24)
    # last maximum in place of the first: the arg-maxima differ at the ties, and the routed gradient with them
    _, first = ref.pool_max(feat, ids)
    _, last = ref.pool_max(feat, ids, last=True)
    assert not torch.equal(first, last)
    good32 = ref.pool_max_bwd(grad, first, ids, dtype=torch.float32)
    assert _ratio(good32, ref.forms(ref.pool_max_bwd, grad, last, ids)) > GATE
    assert _ratio(good32, ref.forms(ref.pool_max_bwd, grad, first, ids)) <= 1.0
    # a long segment's mean divided by 32 in place of its length
    V = cases.POOL_R ** 3
    good32 = ref.scatter_mean(feat, ids, V, dtype=torch.float32)
    assert _ratio(good32, ref.forms(ref.scatter_mean, feat, ids, V, long_div=32)) > GATE
    assert _ratio(good32, ref.forms(ref.scatter_mean, feat, ids, V)) <= 1.0
    good32 = ref.pool_mean(feat, ids, dtype=torch.float32)
    assert _ratio(good32, ref.forms(ref.pool_mean, feat, ids, long_div=32)) > GATE
    # an element nothing contributes to must be exactly zero
    z = ref.forms(ref.scatter_mean, feat, ids, V)
    dirty = z[1].clone()
    empty = torch.nonzero(z[2].view(-1) == 0).view(-1)
    assert empty.numel() > 0
    dirty.view(-1)[empty[0]] = 1e-30
    assert ref.stray(z[1], z[2]) == 0 and ref.stray(dirty, z[2]) == 1


# ---- 5. the module cases' seeds ----------------------------------------------------------------------------------------------------------
def test_recorded_seeds_are_the_reference_s_choice():
    assert set(cases.MODULE_SEEDS) == {(24, "grid"), (24, "planes"), (32, "grid"), (32, "planes"),
                                       (cases.HIDDEN_BOUND, "grid"), (cases.HIDDEN_BOUND + 1, "grid")}
    for (hidden, kind), (seed, pre, gap) in cases.MODULE_SEEDS.items():
        net, p, _ = cases.module_case(hidden, seed)
        got = cases.module_gaps(net, p, cases.module_indices(p, kind))
        assert abs(got[0] - pre) <= 0.01 * pre and abs(got[1] - gap) <= 0.01 * gap, ((hidden, kind), got)
    # the search itself, for one case
    hidden, kind = 24, "grid"
    best = None
    for seed in range(40):
        net, p, _ = cases.module_case(hidden, seed)
        pre, gap = cases.module_gaps(net, p, cases.module_indices(p, kind))
        if best is None or min(pre, gap) > best[1]:
            best = (seed, min(pre, gap))
    assert best[0] == cases.MODULE_SEEDS[(hidden, kind)][0]
