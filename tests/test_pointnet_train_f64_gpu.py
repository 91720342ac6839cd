"""GPU: the kernels of the PointNet encoder's training path against the float64 reference of tests/pointnet_train_ref.py -- the dense
kernels of pointnet.hip (vt_linear_rows, vt_resblock_fc, vt_resblock_fc_bwd in its MFMA and FMA forms, vt_rows_wgrad,
vt_resblock_wgrad) at the widths and row counts of tests/pointnet_train_cases.py (every tile edge, one grid-stride round past each
kernel's cap), the pools and scatter-means of voxel.hip at 8 to 512 channels over constructed segments, and LocalPoolPointnet's
point features under autograd (tests/test_pointnet_train_ref_cpu.py asserts what the cases hold and that the gate bites).

The gate, for every compared tensor and elementwise: |got - ref64| <= 8 max(e32, 2^-24 bound), e32 the largest error of the same
reference run in float32 on the CPU, bound the same sums over magnitudes; an element nothing contributes to must be exactly 0.  The
block's ``act`` is gated first and the backward's reference then takes its h mask from the kernel's own act; the weight gradients'
reference takes the kernel's act and d h as its inputs.  Max-pool values and arg-maxima are compared for equality.  The module cases use
the L2 form per tensor, || t - t64 || / || t64 || <= 8 e32.  Every comparison prints `RATIO <tag>: err / gate-base`."""
import copy
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointnet_train_cases as cases
import pointnet_train_ref as ref
from decode_train_ref import gate_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gate(tag, got, r64, r32, bound):
    ratio, e32 = gate_ratio(got, r64, r32, bound)
    stray = ref.stray(got, bound)
    print(f"RATIO {tag}: {ratio:.3f} (e32 {e32:.3e})")
    assert stray == 0, f"{tag}: {stray} elements nothing contributes to are not exactly 0"
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(e32, 2^-24 bound), above {GATE}"
    return ratio


def _gate_forms(tag, got, forms):
    return _gate(tag, got, *forms)


def _d(t):
    return t.to(DEV) if t is not None else None


# ---- 1. the block: forward, data gradient, weight gradients ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", cases.with_bound_width(), ids=lambda w: "C%d+%d_H%d_O%d_%s" % (w[0], w[1], w[2], w[3], "ws" if w[4] else "id"))
def test_resblock_kernels_vs_float64(width):
    """ops.resblock_fc, ops.resblock_fc_bwd, ops.rows_wgrad and ops.resblock_wgrad at one width and every row count of
    cases.row_counts: out; act, then d x1, d x2 and d h with the kernel's own mask; the five weight and bias gradients from the
    kernel's act and d h, per product and in the one pair of launches (bit-equal to each other)."""
    from vtaco_amd import ops
    C1, C2, H, O, short = width
    w = cases.block_weights(width)
    wd = {k: _d(v) for k, v in w.items()}
    fc_0, fc_1 = SimpleNamespace(weight=wd["w0"], bias=wd["b0"]), SimpleNamespace(weight=wd["w1"], bias=wd["b1"])
    sc = SimpleNamespace(weight=wd["ws"]) if short else None
    kind = "mfma" if cases.takes_mfma(C1, C2, H, O) else "fma"
    for N in cases.row_counts(width, _cus()):
        tag = f"block/{kind} C{C1}+{C2} H{H} O{O} {'ws' if short else 'id'} N{N}"
        x1, x2, dout = cases.block_rows(N, width)
        x1d, x2d, dd = _d(x1), _d(x2), _d(dout)
        out = ops.resblock_fc(x1d, x2d, fc_0, fc_1, sc)
        assert out.shape == (N, O)
        _gate_forms(f"{tag} out", out, ref.forms(ref.resblock_fwd, x1, x2, w["w0"], w["b0"], w["w1"], w["b1"], w["ws"]))
        dx1, dx2, act, dh = ops.resblock_fc_bwd(x1d, x2d, wd["w0"], wd["b0"], wd["w1"], wd["ws"], dd)
        _gate_forms(f"{tag} act", act, ref.forms(ref.resblock_act, x1, x2, w["w0"], w["b0"]))
        assert bool((act >= 0).all())
        actc, dhc = act.cpu(), dh.cpu()
        b64, b32, bb = ref.forms(ref.resblock_bwd, x1, x2, w["w0"], w["w1"], w["ws"], dout, actc > 0)
        _gate(f"{tag} dh", dh, b64[2], b32[2], bb[2])
        _gate(f"{tag} dx1", dx1, b64[0], b32[0], bb[0])
        if C2:
            _gate(f"{tag} dx2", dx2, b64[1], b32[1], bb[1])
            dx1b, none, actb, dhb = ops.resblock_fc_bwd(x1d, x2d, wd["w0"], wd["b0"], wd["w1"], wd["ws"], dd, want_dx2=False)
            assert none is None and torch.equal(dx1b, dx1) and torch.equal(actb, act) and torch.equal(dhb, dh), tag
        else:
            assert dx2 is None
        # the weight gradients, from the kernel's own act and d h
        f1 = ref.forms(ref.rows_wgrad, dout, actc)
        f0 = ref.forms(ref.rows_wgrad, dhc, x1, x2, relu_x=True)
        dw1, db1 = ops.rows_wgrad(dd, act)
        dw0, db0 = ops.rows_wgrad(dh, x1d, x2d, relu_x=True)
        for name, got, k, f in (("dW1", dw1, 0, f1), ("db1", db1, 1, f1), ("dW0", dw0, 0, f0), ("db0", db0, 1, f0)):
            _gate(f"{tag} {name}", got, f[0][k], f[1][k], f[2][k])
        dws = None
        if short:
            fs = ref.forms(ref.rows_wgrad, dout, x1, x2)
            dws, none = ops.rows_wgrad(dd, x1d, x2d, want_bias=False)
            assert none is None
            _gate(f"{tag} dWs", dws, fs[0][0], fs[1][0], fs[2][0])
        multi = ops.resblock_wgrad(x1d, x2d, act, dh, dd, short)
        assert multi is not None, tag
        for a, b in zip(multi, (dw0, db0, dw1, db1, dws)):
            assert (a is None and b is None) or torch.equal(a, b), tag


# ---- 2. the linear layer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,Cout", cases.LINEAR)
def test_linear_rows_vs_float64(Cin, Cout):
    """ops.linear_rows with and without a bias, its data gradient (the same kernel on W^T) and ops.rows_wgrad of the layer."""
    from vtaco_amd import ops
    for N in cases.linear_row_counts(Cout, _cus()):
        tag = f"linear {Cin}->{Cout} N{N}"
        x, w, b = cases.linear_case(N, Cin, Cout)
        g = torch.randn(N, Cout, generator=torch.Generator().manual_seed(N + Cout))
        g[::7] = 0.0
        xd, wdev, bd, gd = _d(x), _d(w), _d(b), _d(g)
        _gate_forms(f"{tag} out", ops.linear_rows(xd, wdev, bd), ref.forms(ref.linear_rows, x, w, b))
        _gate_forms(f"{tag} out (no bias)", ops.linear_rows(xd, wdev, None), ref.forms(ref.linear_rows, x, w))
        _gate_forms(f"{tag} dx", ops.linear_rows(gd, wdev.t().contiguous(), None), ref.forms(ref.linear_rows, g, w.t()))
        f = ref.forms(ref.rows_wgrad, g, x)
        dW, db = ops.rows_wgrad(gd, xd)
        _gate(f"{tag} dW", dW, f[0][0], f[1][0], f[2][0])
        _gate(f"{tag} db", db, f[0][1], f[1][1], f[2][1])


# ---- 3. pools and scatters ------------------------------------------------------------------------------------------------------------
def _same_routing(tag, got, r64):
    assert torch.equal(got.cpu() != 0, r64 != 0), f"{tag}: the non-zero entries differ"


@pytest.fixture(scope="module")
def pool_index():
    """The constructed point set on the device: its volume index and its three plane indices, with the cell ids checked."""
    from vtaco_amd import ops
    pts, ids = cases.pool_points()
    pd = pts.to(DEV)
    vi = ops.VoxelIndex(pd, cases.POOL_R, 0.1)
    assert torch.equal(vi.idx.cpu().long(), ids)
    pis = ops.plane_indices(pd, cases.POOL_R, 0.1, cases.PLANES)
    pids = [cases.cell_ids32(pts.numpy(), cases.POOL_R, plane=k) for k in cases.PLANES]
    for pi, pid in zip(pis, pids):
        assert torch.equal(pi.idx.cpu().long(), pid)
    # the sorted order is (cell, point) and every point knows its cell's range
    order, lo, hi = vi.order.cpu().long(), vi.seg_lo.cpu().long(), vi.seg_hi.cpu().long()
    for b in range(2):
        key = ids[b][order[b]] * cases.POOL_T + order[b]
        assert bool((key[1:] > key[:-1]).all())
        n = torch.unique(ids[b], return_counts=True)
        count = dict(zip(n[0].tolist(), n[1].tolist()))
        assert [int(h - l) for l, h in zip(lo[b], hi[b])] == [count[int(c)] for c in ids[b]]
    return vi, ids, pis, pids


@pytest.mark.parametrize("C", cases.POOL_CHANNELS)
def test_pools_and_scatters_vs_float64(pool_index, C):
    """Every pool and scatter-mean of voxel.hip at C channels over the constructed segments (lengths 1, 2, 31, 32, 33, 64, 65; long
    segments from an aligned position, from 31 past one and to the scene's end; a scene in one cell; exact ties): max-pool values and
    arg-maxima equal to the reference's, the routing of its gradient exact, sums and means within the gate."""
    from vtaco_amd import ops
    vi, ids, pis, pids = pool_index
    B, T, R = 2, cases.POOL_T, cases.POOL_R
    V = R ** 3
    feat, grad = cases.pool_features(C)
    fd, gd = feat.to(DEV), grad.to(DEV)
    tag = f"pool C{C}"
    # max-pool over the volume's cells
    want, warg = ref.pool_max(feat, ids)
    out, arg = ops.voxel_pool_max_fwd(fd, vi)
    assert torch.equal(out.cpu(), want) and torch.equal(arg.cpu().long(), warg), tag
    assert torch.equal(ops.voxel_pool_max_fwd(fd, vi, want_argmax=False)[0], out)
    f = ref.forms(ref.pool_max_bwd, grad, warg, ids)
    got = ops.voxel_pool_max_bwd(gd, arg, vi)
    _gate_forms(f"{tag} pool_max_bwd", got, f)
    _same_routing(f"{tag} pool_max_bwd", got, f[0])
    # mean-pool (its backward is the same call on the gradient)
    _gate_forms(f"{tag} pool_mean", ops.voxel_pool_mean(fd, vi), ref.forms(ref.pool_mean, feat, ids))
    _gate_forms(f"{tag} pool_mean(grad)", ops.voxel_pool_mean(gd, vi), ref.forms(ref.pool_mean, grad, ids))
    # scatter-mean into the volume, both layouts, and back
    gg = torch.randn(B, C, V, generator=torch.Generator().manual_seed(C))
    ggd = gg.to(DEV)
    _gate_forms(f"{tag} scatter_mean_fwd", ops.voxel_scatter_mean_fwd(fd, vi).view(B, C, V), ref.forms(ref.scatter_mean, feat, ids, V))
    _gate_forms(f"{tag} scatter_mean_cl_fwd", ops.voxel_scatter_mean_cl_fwd(fd, vi).view(B, V, C),
                ref.forms(ref.scatter_mean, feat, ids, V, channels_last=True))
    _gate_forms(f"{tag} scatter_mean_bwd", ops.voxel_scatter_mean_bwd(ggd.view(B, C, R, R, R), vi, C), ref.forms(ref.scatter_mean_bwd, gg, ids))
    ggcl = gg.permute(0, 2, 1).contiguous()
    _gate_forms(f"{tag} scatter_mean_cl_bwd", ops.voxel_scatter_mean_cl_bwd(ggcl.to(DEV).view(B, R, R, R, C), vi, C),
                ref.forms(ref.scatter_mean_bwd, ggcl, ids, channels_last=True))
    # the three planes: the sum of their max-pools, each plane's arg-maxima
    wargs = [ref.pool_max(feat, pid)[1] for pid in pids]
    out, args = ops.voxel_pool_max_sum_fwd(fd, pis)
    for k in range(3):
        assert torch.equal(args[k].cpu().long(), wargs[k]), f"{tag} plane {k}"
    _gate_forms(f"{tag} pool_max_sum_fwd", out, ref.forms(ref.pool_max_sum, feat, pids))
    assert torch.equal(ops.voxel_pool_max_sum_fwd(fd, pis, want_argmax=False)[0], out)
    f = ref.forms(ref.pool_max_sum_bwd, grad, wargs, pids)
    got = ops.voxel_pool_max_sum_bwd(gd, args, pis)
    _gate_forms(f"{tag} pool_max_sum_bwd", got, f)
    _same_routing(f"{tag} pool_max_sum_bwd", got, f[0])
    # a plane's max-pool by the volume's kernel (PlaneIndex is a VoxelIndex)
    out, arg = ops.voxel_pool_max_fwd(fd, pis[1])
    assert torch.equal(out.cpu(), ref.pool_max(feat, pids[1])[0]) and torch.equal(arg.cpu().long(), wargs[1]), tag
    # scatter-means into the planes, one at a time and the three in one launch, and back
    V2 = R * R
    gp = torch.randn(3 * B, C, V2, generator=torch.Generator().manual_seed(C + 1))
    gpd = gp.to(DEV)
    for k in (0, 2):
        _gate_forms(f"{tag} plane_scatter_mean_fwd[{cases.PLANES[k]}]", ops.plane_scatter_mean_fwd(fd, pis[k]).view(B, C, V2),
                    ref.forms(ref.scatter_mean, feat, pids[k], V2))
        _gate_forms(f"{tag} plane_scatter_mean_bwd[{cases.PLANES[k]}]", ops.plane_scatter_mean_bwd(gpd[:B].view(B, C, R, R), pis[k], C),
                    ref.forms(ref.scatter_mean_bwd, gp[:B], pids[k]))
    assert ops.plane_group(pis) is not None
    _gate_forms(f"{tag} plane_scatter_mean_multi_fwd", ops.plane_scatter_mean_multi_fwd(fd, pis).view(3 * B, C, V2),
                ref.forms(ref.scatter_mean_multi, feat, pids, V2))
    _gate_forms(f"{tag} plane_scatter_mean_multi_bwd", ops.plane_scatter_mean_multi_bwd(gpd.view(3 * B, C, R, R), pis, C),
                ref.forms(ref.scatter_mean_multi_bwd, gp, pids))


# ---- 4. the module -------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Counts and records the calls of one ops function while it is patched in."""

    def __init__(self, monkeypatch, name):
        from vtaco_amd import ops
        self.fn, self.calls = getattr(ops, name), []
        monkeypatch.setattr(ops, name, self)

    def __call__(self, *a, **k):
        out = self.fn(*a, **k)
        self.calls.append((a, k, out))
        return out


def _device_indices(p, kind):
    from vtaco_amd import ops
    pd = p.to(DEV)
    if kind == "grid":
        return pd, ops.VoxelIndex(pd, cases.GRID_R, 0.1)
    return pd, ops.plane_indices(pd, cases.PLANE_R, 0.1, cases.PLANES)


@pytest.mark.parametrize("hidden,kind", sorted(cases.MODULE_SEEDS), ids=lambda v: str(v))
def test_point_features_under_autograd_vs_float64_module(monkeypatch, hidden, kind):
    """LocalPoolPointnet.point_features with train_mlp = "hip" on one VoxelIndex and on the three-plane list (B = 2, T = 301), output
    and every parameter gradient against a .double() copy of the module on the CPU, L2 per tensor within 8 e32.  hidden_dim 24 takes
    the FMA backward, 32 the MFMA one; the largest admitted hidden_dim (47) runs on the HIP kernels and 48 on nn.Linear, both
    without raising."""
    monkeypatch.delenv("VTACO_RESBLOCK_MFMA", raising=False)
    seed = cases.MODULE_SEEDS[(hidden, kind)][0]
    net, p, wgt = cases.module_case(hidden, seed)
    idxs = cases.module_indices(p, kind)
    r64 = cases.module_step(net, p, wgt, idxs, torch.float64)
    r32 = cases.module_step(net, p, wgt, idxs, torch.float32)
    m = copy.deepcopy(net).to(DEV)
    m.train_mlp = "hip"
    fits = hidden <= cases.HIDDEN_BOUND
    assert m._fused_mlp_fits() == fits
    pd, vi = _device_indices(p, kind)
    for got, want in zip([vi] if kind == "grid" else vi, idxs):
        assert torch.equal(got.idx.cpu().long(), want)
    bwd = _Spy(monkeypatch, "resblock_fc_bwd")
    out = m.point_features(pd, vi)
    (out * wgt.to(DEV)).sum().backward()
    assert len(bwd.calls) == (5 if fits else 0)
    got = {"out": out.detach()}
    got.update({"grad:" + n: q.grad for n, q in m.named_parameters() if q.grad is not None})
    assert set(got) == set(r64) and len(got) == 1 + 4 + 5 * 5
    for k in sorted(r64):
        e32 = cases.rel_err(r32[k], r64[k])
        err = cases.rel_err(got[k], r64[k])
        print(f"RATIO module h{hidden} {kind} {k}: {err / e32:.3f} (e32 {e32:.3e})")
        assert err <= GATE * e32, f"{k}: relative L2 error {err:.3e} against e32 {e32:.3e}"


def test_reference_default_widths_pools_and_scatter_vs_float64(monkeypatch):
    """hidden_dim = c_dim = 128, the reference's class defaults: the dense layers are the framework's (nn.Linear), the four max-pools
    and the scatter-mean around them the HIP kernels at C = 128.  Each pool's values and arg-maxima equal the reference's on the
    features it was given, the gradients it routes and the grid and its gradient are within the gate."""
    from vtaco_amd import ops
    from vtaco_amd.encoder.pointnet import LocalPoolPointnet
    torch.manual_seed(128)
    R = cases.GRID_R
    m = LocalPoolPointnet(grid_resolution=R, plane_type='grid')
    assert m.hidden_dim == 128 and m.c_dim == 128 and not m._fused_mlp_fits()
    g = torch.Generator().manual_seed(129)
    with torch.no_grad():
        for blk in m.blocks:
            blk.fc_1.weight.copy_(torch.randn(blk.fc_1.weight.shape, generator=g) * 0.05)
    m = m.to(DEV)
    p = (torch.rand(cases.MODULE_B, cases.MODULE_T, 3, generator=g) - 0.5)
    wgt = torch.randn(cases.MODULE_B, 128, R, R, R, generator=g)
    ids = cases.cell_ids32(p.numpy(), R)
    spies = {n: _Spy(monkeypatch, n) for n in ("voxel_pool_max_fwd", "voxel_pool_max_bwd", "voxel_scatter_mean_fwd", "voxel_scatter_mean_bwd",
                                                "resblock_fc_bwd", "linear_rows", "rows_wgrad")}
    grid = m(p.to(DEV))["grid"]
    (grid * wgt.to(DEV)).sum().backward()
    for n in ("resblock_fc_bwd", "linear_rows", "rows_wgrad"):
        assert not spies[n].calls, n
    assert len(spies["voxel_pool_max_fwd"].calls) == 4 and len(spies["voxel_pool_max_bwd"].calls) == 4
    args = []
    for i, ((feat, vi), _, (out, arg)) in enumerate(spies["voxel_pool_max_fwd"].calls):
        assert feat.shape[2] == 128 and torch.equal(vi.idx.cpu().long(), ids)
        want, warg = ref.pool_max(feat, ids)
        assert torch.equal(out.cpu(), want) and torch.equal(arg.cpu().long(), warg), i
        args.append(warg)
    for i, ((gout, arg, vi), _, got) in enumerate(spies["voxel_pool_max_bwd"].calls):          # the backward runs the pools last to first
        warg = args[3 - i]
        assert torch.equal(arg.cpu().long(), warg)
        f = ref.forms(ref.pool_max_bwd, gout, warg, ids)
        _gate_forms(f"module h128 pool_max_bwd[{3 - i}]", got, f)
        _same_routing(f"module h128 pool_max_bwd[{3 - i}]", got, f[0])
    ((feat, vi), _, out), = spies["voxel_scatter_mean_fwd"].calls
    assert out.data_ptr() == grid.data_ptr()
    _gate_forms("module h128 scatter_mean_fwd", out.view(cases.MODULE_B, 128, -1), ref.forms(ref.scatter_mean, feat, ids, R ** 3))
    ((gg, vi, C), _, got), = spies["voxel_scatter_mean_bwd"].calls
    _gate_forms("module h128 scatter_mean_bwd", got, ref.forms(ref.scatter_mean_bwd, gg.reshape(cases.MODULE_B, 128, -1), ids))
