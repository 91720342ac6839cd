"""GPU: the kernels of the 32/32 decoder's training path against the float64 reference of tests/decode_train_ref.py -- the forward's
save buffer (vt_decode_fwd with save, vt_decode_mlp_fwd_train), the backward (vt_decode_bwd / _contact / _dc, vt_decode_mlp_bwd), the
weight gradients (vt_decode_wgrad / _contact) and the grid scatter (vt_sample_grid_bwd / _sorted) on both routes, at the seeded inputs of
tests/decode_train_cases.py (tests/test_decode_train_ref_cpu.py asserts what those hold).

The gate, for every compared tensor and elementwise: |got - ref64| <= 8 max(e32, 2^-24 bound), e32 the largest error of the same
reference run in float32 on the CPU, bound the same sums over magnitudes.  The backward's reference takes the ReLU masks and layer inputs
from the kernel's own save buffer, which the first test gates by itself.  Every comparison prints `RATIO <tag>: err / gate-base`.

That the gates bite was tried on the reference: two save slots swapped in its forward or in its backward, or the last point of an odd
total left out of its weight gradients, and the save, backward, mlp and lattice tests fail.  Dropping its top-border weight zeroing
changes nothing: no input reaches that corner (tests/test_decode_train_ref_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_train_cases as cases
import decode_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
FORMS = ("plain", "img", "contact")
PARAM_KEYS = ("fc_p.weight", "fc_p.bias", "fc_c.weight", "fc_c.bias", "fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias",
              "fc_out.weight", "fc_out.bias")
SLOTS = ("c",) + tuple(f"relu_x{i}" for i in range(5)) + tuple(f"relu_h{i}" for i in range(5)) + ("relu_net5",)


@pytest.fixture(autouse=True)
def _default_route():
    if os.environ.get("VTACO_GRID_SCATTER"):
        pytest.skip("the grid scatter's route is forced by VTACO_GRID_SCATTER")


class _Weights:
    """One weight set on the device: the module (for its packing) and its blobs, packed once."""

    def __init__(self, sd):
        from vtaco_amd.conv_onet.models import decoder_dict
        self.sd = sd
        self.dec = decoder_dict['simple_local'](dim=3, c_dim=32, hidden_size=32, with_contact=True)
        self.dec.load_state_dict(sd, strict=True)
        self.dec.to(DEV)
        self._t = {}

    def blob(self, form="plain"):
        with torch.no_grad():
            return self.dec._blob(img=form == "img", contact=form == "contact")

    def blob_t(self, form="plain"):
        if form not in self._t:
            with torch.no_grad():
                self._t[form] = self.dec._blob_t(img=form == "img", contact=form == "contact")
        return self._t[form]


@pytest.fixture(scope="module")
def weights():
    return {k: _Weights(sd) for k, sd in cases.weight_sets().items()}


def _gate(tag, got, r64, r32, bound):
    ratio, e32 = ref.gate_ratio(got, r64, r32, bound)
    print(f"RATIO {tag}: {ratio:.3f} (e32 {e32:.3e})")
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(e32, 2^-24 bound), above {GATE}"
    return ratio


def _route(monkeypatch, sorted_):
    from vtaco_amd.ops import decode_train
    monkeypatch.setattr(decode_train, "GRID_SCATTER_SORTED", sorted_)


def _forward(W, inp, form):
    """The training forward on the device: (logits or the pair, the save buffer)."""
    from vtaco_amd import ops
    pts = inp["pts"].to(DEV)
    B, N = pts.shape[:2]
    save = ops.decode_save_buffer(B * N, DEV)
    out = ops.decode_fwd(inp["grid"].to(DEV), W.blob(form), pts=pts, c_img=inp["c_img"].to(DEV) if form == "img" else None,
                         save=save, want_contact=form == "contact")
    return out, save


def _backward(W, inp, form, save, **kw):
    from vtaco_amd import ops
    img = form == "img"
    return ops.decode_bwd(tuple(inp["grid"].shape), W.blob_t(form), inp["grad_out"].to(DEV), save, pts=inp["pts"].to(DEV),
                          with_c_img=img, c_img=inp["c_img"].to(DEV) if img else None,
                          grad_out2=inp["grad_out2"].to(DEV) if form == "contact" else None, **kw)


def _check_saves(tag, W, inp, form, out, save, c=None):
    B, N = inp["pts"].shape[:2]
    args = (W.sd, inp["pts"], None if c is not None else inp["grid"], inp["c_img"] if form == "img" else None, form == "contact", c)
    (o64, s64), (o32, s32), (ob, sb) = ref.forward64(*args), ref.forward32(*args), ref.forward_bound(*args)
    got = save.view(12, B, N, 32).cpu()
    for k in range(12):
        _gate(f"{tag} save[{k}] {SLOTS[k]}", got[k], s64[k], s32[k], sb[k])
    if form == "contact":
        for j, name in enumerate(("logits", "contact logits")):
            _gate(f"{tag} {name}", out[j], o64[j], o32[j], ob[j])
    else:
        _gate(f"{tag} logits", out, o64, o32, ob)


def _check_backward(tag, W, inp, form, save, ggrid, gimg, flat, grid_grad=True):
    """Gate the grid gradient, d c_img and every entry of the flat gradient against backward64 with the kernel's own saves."""
    from vtaco_amd import ops
    B, N = inp["pts"].shape[:2]
    img, contact = form == "img", form == "contact"
    saves = save.view(12, B, N, 32).cpu()
    args = (W.sd, inp["pts"], tuple(inp["grid"].shape) if grid_grad else None, saves, inp["grad_out"],
            inp["grad_out2"] if contact else None, inp["c_img"] if img else None)
    (r64, bnd), r32 = ref.backward64(*args), ref.backward32(*args)
    if grid_grad:
        _gate(f"{tag} grad_grid", ggrid.permute(0, 2, 3, 4, 1), r64["grad_grid"], r32["grad_grid"], bnd["grad_grid"])
    if img:
        _gate(f"{tag} grad_c_img", gimg, r64["grad_c_img"], r32["grad_c_img"], bnd["grad_c_img"])
    g = ops.split_decoder_grads(flat, 35 if img else 3)
    keys = PARAM_KEYS + (("fc_out_contact.weight", "fc_out_contact.bias") if contact else ())
    assert set(g) == set(keys)
    for k in keys:
        _gate(f"{tag} {k}", g[k], r64[k], r32[k], bnd[k])


def _full_backward(monkeypatch, weights, B, N, Rs, sorted_, route):
    _route(monkeypatch, sorted_)
    for R in Rs:
        inp = cases.make_inputs(B, N, R)
        for wname, W in weights.items():
            for form in FORMS:
                tag = f"bwd/{route}/{form}/{wname} B{B} N{N} R{R}"
                _, save = _forward(W, inp, form)
                ggrid, gimg, flat = _backward(W, inp, form, save)
                assert ggrid.shape == inp["grid"].shape
                _check_backward(tag, W, inp, form, save, ggrid, gimg, flat)
                # fixed-order reductions: the parameter gradients and d c_img are the same bits on every call
                _, gimg2, flat2 = _backward(W, inp, form, save)
                assert torch.equal(flat, flat2), tag
                if form == "img":
                    assert torch.equal(gimg, gimg2), tag
                if not sorted_ or R < 3:
                    gnone, gimg3, flat3 = _backward(W, inp, form, save, want_grid_grad=False)
                    assert gnone is None and torch.equal(flat, flat3), tag
                    if form == "img":
                        assert torch.equal(gimg, gimg3), tag
                if form == "img" and B == 3:
                    # a scene's d c_img does not depend on what shares its tiles
                    for b in range(B):
                        one = {k: v[b:b + 1].contiguous() for k, v in inp.items()}
                        _, s1 = _forward(W, one, form)
                        _, g1, _ = _backward(W, one, form, s1)
                        assert torch.equal(g1[0], gimg[b]), f"{tag}: scene {b} alone"


# ---- 1. the save buffer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", cases.TOTALS)
def test_save_buffer_and_logits_vs_float64(weights, B, N):
    """vt_decode_fwd with a save buffer -- plain, with c_img and with the contact head -- and vt_decode_mlp_fwd_train (features given):
    all twelve saved tensors and the logits within the gate, at every total and R in {2, 3, 5, 8}, both weight sets."""
    from vtaco_amd import ops
    for R in cases.RS:
        inp = cases.make_inputs(B, N, R)
        for wname, W in weights.items():
            for form in FORMS:
                out, save = _forward(W, inp, form)
                _check_saves(f"fwd/{form}/{wname} B{B} N{N} R{R}", W, inp, form, out, save)
    inp = cases.make_inputs(B, N, 5)
    c = torch.randn(B, N, 32, generator=torch.Generator().manual_seed(B * 10007 + N))
    for wname, W in weights.items():
        out, save = ops.decode_mlp_fwd_train(c.to(DEV), W.blob(), inp["pts"].to(DEV))
        _check_saves(f"mlp_fwd/{wname} B{B} N{N}", W, inp, "plain", out, save, c=c)


# ---- 2. the full backward, grid gradient by cell ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", cases.TOTALS)
def test_backward_sorted_route_vs_float64(monkeypatch, weights, B, N):
    """ops.decode_bwd on the default route (vt_decode_bwd_dc + vt_sample_grid_bwd_sorted + vt_decode_wgrad[_contact]) in the plain,
    c_img and contact forms at R in {3, 5, 8}: grid gradient, d c_img and every parameter gradient within the gate; parameter gradients
    and d c_img bit-identical on a second call; d c_img of B = 3 equal to the three scenes run alone, bit for bit."""
    _full_backward(monkeypatch, weights, B, N, (3, 5, 8), True, "sorted")


# ---- 3. the same on the per-point atomics route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", cases.TOTALS)
def test_backward_points_route_vs_float64(monkeypatch, weights, B, N):
    """The same cases with the data kernel's own scatter (vt_decode_bwd[_contact]), plus R = 2, which takes it whatever the switch
    says; want_grid_grad=False leaves the parameter gradients and d c_img bit-identical."""
    _full_backward(monkeypatch, weights, B, N, (2, 3, 5, 8), False, "points")


def test_r2_takes_the_points_route_under_the_default_switch(monkeypatch, weights):
    _full_backward(monkeypatch, weights, 3, 427, (2,), True, "points(R=2, switch sorted)")


# ---- 4. the scatter alone ------------------------------------------------------------------------------------------------------------
def _scatter_refs(pts, gf, R):
    r64, bnd = ref.scatter64(pts, gf, R)
    r32, _ = ref.scatter64(pts, gf, R, dtype=torch.float32)
    return r64, r32, bnd


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "points"])
def test_sample_grid_bwd_vs_float64(monkeypatch, C, sorted_):
    """ops.sample_grid_bwd (vt_sample_grid_bwd_sorted / vt_sample_grid_bwd) at 32, 64 and 128 channels -- the blockIdx.y slices --
    against the float64 scatter, at partial and batch-straddling tiles and R in {2, 3, 5, 8}."""
    from vtaco_amd import ops
    _route(monkeypatch, sorted_)
    for B, N in ((1, 1), (3, 11), (5, 205), (1, 2303)):
        for R in cases.RS:
            pts = cases.make_points(B, N, R)
            gf = torch.randn(B, N, C, generator=torch.Generator().manual_seed(C + N))
            gf.view(-1, C)[::5] = 0.0
            got = ops.sample_grid_bwd((B, C, R, R, R), pts.to(DEV), gf.to(DEV))
            assert got.shape == (B, C, R, R, R)
            _gate(f"scatter/{'sorted' if sorted_ else 'points'}/C{C} B{B} N{N} R{R}", got.permute(0, 2, 3, 4, 1), *_scatter_refs(pts, gf, R))


# ---- 5. the sorted kernel's fallback ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [5, 8])
@pytest.mark.parametrize("reso", [1, 2])
def test_sorted_scatter_with_foreign_segments_vs_float64(R, reso):
    """vt_sample_grid_bwd_sorted with segments that are not its cells -- vt_voxel_build at resolution 1 and 2 instead of R - 1, so each
    segment spans many cells and every point outside its head's cell takes the kernel's fallback (its own atomics): the same sum, within
    the same gate."""
    from vtaco_amd import _lib
    from vtaco_amd.ops._base import I32, check, dev_ptr, stream_ptr
    from vtaco_amd.ops.voxel import VoxelIndex
    B, N = 3, 427
    pts = cases.make_points(B, N, R)
    cell = np.floor(np.minimum(cases.grid_coord32(pts.numpy(), R), np.float32(R - 2))).astype(np.int64)
    pd = pts.to(DEV)
    vi = VoxelIndex(pd, reso, 0.1)
    order, lo, hi = vi.order.cpu().long(), vi.seg_lo.cpu().long(), vi.seg_hi.cpu().long()
    foreign = 0
    for b in range(B):                                           # points whose cell is not their segment head's: they take the fallback
        head = order[b][lo[b]]
        foreign += int((cell[b] != cell[b][head.numpy()]).any(-1).sum())
        assert int((hi[b] - lo[b]).max()) <= N and len(torch.unique(lo[b])) <= reso ** 3
    assert foreign >= B * N // 4, foreign
    for C in (32, 64):
        gf = torch.randn(B, N, C, generator=torch.Generator().manual_seed(R * 100 + reso + C))
        gf.view(-1, C)[::5] = 0.0
        gd = gf.to(DEV)
        gg = torch.zeros((B, R, R, R, C), dtype=torch.float32, device=DEV)
        check(_lib.load().vt_sample_grid_bwd_sorted(B, R, C, dev_ptr(pd, "pts"), N, 0.1, dev_ptr(gd, "grad_feat"),
                                                    dev_ptr(vi.order, "order", I32), dev_ptr(vi.seg_lo, "seg_lo", I32),
                                                    dev_ptr(vi.seg_hi, "seg_hi", I32), dev_ptr(gg, "grad_grid"), stream_ptr()),
              "vt_sample_grid_bwd_sorted")
        _gate(f"scatter/fallback/C{C} segments at {reso} R{R}", gg, *_scatter_refs(pts, gf, R))


# ---- 6. the MLP alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", cases.TOTALS)
def test_decode_mlp_bwd_vs_float64(weights, B, N):
    """ops.decode_mlp_bwd (vt_decode_mlp_bwd + vt_decode_wgrad) after vt_decode_mlp_fwd_train: d c and the flat gradients."""
    from vtaco_amd import ops
    inp = cases.make_inputs(B, N, 5)
    c = torch.randn(B, N, 32, generator=torch.Generator().manual_seed(B * 10007 + N + 1))
    for wname, W in weights.items():
        tag = f"mlp_bwd/{wname} B{B} N{N}"
        pd = inp["pts"].to(DEV)
        _, save = ops.decode_mlp_fwd_train(c.to(DEV), W.blob(), pd)
        grad_c, flat = ops.decode_mlp_bwd(W.blob_t(), inp["grad_out"].to(DEV), save, pd)
        saves = save.view(12, B, N, 32).cpu()
        (r64, bnd), r32 = ref.backward64(W.sd, inp["pts"], None, saves, inp["grad_out"]), ref.backward32(W.sd, inp["pts"], None, saves, inp["grad_out"])
        _gate(f"{tag} grad_c", grad_c, r64["grad_c"], r32["grad_c"], bnd["grad_c"])
        g = ops.split_decoder_grads(flat, 3)
        assert set(g) == set(PARAM_KEYS)
        for k in PARAM_KEYS:
            _gate(f"{tag} {k}", g[k], r64[k], r32[k], bnd[k])
        grad_c2, flat2 = ops.decode_mlp_bwd(W.blob_t(), inp["grad_out"].to(DEV), save, pd)
        assert torch.equal(grad_c, grad_c2) and torch.equal(flat, flat2), tag


# ---- 7. the lattice form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,first,count,B,R", [(6, 5, 200, 2, 5), (12, 17, 1100, 2, 8)])
def test_lattice_backward_equals_the_point_form(weights, nx, first, count, B, R):
    """ops.decode_bwd(lattice=...) -- the points generated in the kernels (point_of's lattice branch in the scatter, job 15 of the weight
    gradients) -- on a slab that starts inside a row: parameter gradients bit-equal to the point form on the same coordinates, the grid
    gradient within the gate; vt_decode_fwd with a lattice and a save buffer saves what the point form saves."""
    from vtaco_amd import ops
    lat = (nx, 1.1, first, count)
    pts = torch.from_numpy(cases.lattice_points(nx)[first:first + count]).unsqueeze(0).expand(B, -1, -1).contiguous()
    inp = cases.make_inputs(B, count, R)
    inp["pts"] = pts
    for wname, W in weights.items():
        for form in ("plain", "img"):
            tag = f"lattice/{form}/{wname} nx{nx} B{B} N{count} R{R}"
            img = form == "img"
            out, save = _forward(W, inp, form)
            ci = inp["c_img"].to(DEV) if img else None
            save_l = ops.decode_save_buffer(B * count, DEV)
            out_l = ops.decode_fwd(inp["grid"].to(DEV), W.blob(form), c_img=ci, lattice=lat, save=save_l)
            assert torch.equal(out_l, out) and torch.equal(save_l, save), tag
            _, gimg_p, flat_p = _backward(W, inp, form, save)
            ggrid, gimg, flat = ops.decode_bwd(tuple(inp["grid"].shape), W.blob_t(form), inp["grad_out"].to(DEV), save, lattice=lat,
                                               with_c_img=img, c_img=ci)
            assert torch.equal(flat, flat_p), tag
            if img:
                assert torch.equal(gimg, gimg_p), tag
            _check_backward(tag, W, inp, form, save, ggrid, gimg, flat)
