"""GPU: the voxel encoder's fused kernels (vt_voxel_encode_grid / _planes / _bwd) against the reference's own outputs
(tests/golden/g25_voxel_encoder.npz) and against the float64 statement of tests/voxel_encoder_ref.py.

The float64 gate, for every compared tensor and elementwise: |got - ref64| <= 8 max(e32, 2^-24 bound) -- e32 the largest error of the
host composition in float32 (torch on the CPU: F.conv3d, index_add, autograd) against float64 over that tensor, bound the same sums over
magnitudes (one f32 rounding of the magnitude sum); 8 is the project's gate (tests/test_decode_train_f64_gpu.py).  A cell no voxel
lands in must be exactly 0.  Every comparison prints ``RATIO <tag>: err / gate-base``.

The ReLU mask is discontinuous, so the gradient fixtures are seeds whose float64 pre-activations keep min |pre| >= 1e-5 over all
(scene, channel, voxel): asserted on the CPU before anything runs; no element is left out of a comparison."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_encoder_ref as ref
from conftest import load_golden, sub_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
PAD = 0.1
T = torch.from_numpy
SHAPES = (((5, 6, 7), 8), ((12, 9, 10), 4), ((8, 8, 8), 8), ((2, 2, 2), 4))      # D < R (empty cells), D > R (ragged boxes), D = R, tiny
SUBSETS = (("xz",), ("xy",), ("yz",), ref.PLANES)
# seeds with min |pre| >= 1e-5 in float64 (asserted below); every case not named here uses 1000
SEEDS = {((12, 9, 10), 64, 3): 1002, ((12, 9, 10), 128, 3): 1003, ((8, 8, 8), 128, 1): 1001}
CASES = [(dims, R, C, k) for dims, R in SHAPES for C in (32, 64, 128) for k in (1, 3)]
FORMS = {"grid": dict(grid_resolution=8, plane_type="grid"),
         "planes": dict(plane_resolution=8, plane_type=["xz", "xy", "yz"]),
         "grid_unet": dict(grid_resolution=8, plane_type="grid", unet3d=True,
                           unet3d_kwargs=dict(num_levels=2, f_maps=8, in_channels=32, out_channels=32)),
         "k1": dict(grid_resolution=8, plane_type="grid", kernel_size=1)}


def _ratio(tag, got, r64, r32, bound):
    """max |got - r64| / max(e32, 2^-24 bound); an element whose base is 0 must be exactly 0."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, np.float64).reshape(r64.shape)
    err = np.abs(got - r64)
    e32 = float(np.abs(np.asarray(r32, np.float64) - r64).max())
    base = np.maximum(bound * 2.0 ** -24, e32)
    ratio = np.where(base > 0, err / np.maximum(base, 1e-300), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    print(f"RATIO {tag}: {worst:.3f} (e32 {e32:.3e})")
    assert worst <= GATE, f"{tag}: |got - ref64| is {worst:.3f} x max(e32, 2^-24 bound), above {GATE}"
    return worst


@functools.lru_cache(maxsize=None)
def _case(dims, R, C, k, B):
    """The fixture of a case and its references, computed once and shared by the tests (read-only)."""
    x, w, b = ref.fixture(dims, C, k, SEEDS.get((dims, C, k), 1000))
    x = x[:B]
    names = ("grid",) + ref.PLANES
    out64, bound, pre = ref.forward(x, w, b, R, PAD, names)
    out32, _, _ = ref.host32(x, w, b, R, PAD, names)
    return dict(x=x, w=w, b=b, out64=out64, out32=out32, bound=bound, min_pre=float(np.abs(pre).min()))


def _up(c, names, seed):
    g = np.random.RandomState(seed)
    return {n: g.standard_normal(c["out64"][n].shape).astype(np.float32) for n in names}


def _stack(d, names):
    """{name: [B,C,R,R]} -> [P B,C,R,R] in the encoder's order."""
    return np.concatenate([d[n] for n in names], axis=0)


def _dev(c):
    return T(c["x"]).to(DEV), T(c["w"]).to(DEV), T(c["b"]).to(DEV)


def _encoder(tag, sd, **extra):
    from vtaco_amd.encoder import encoder_dict
    enc = encoder_dict["voxel_simple_local"](dim=3, c_dim=32, padding=0.1, **FORMS[tag], **extra)
    enc.load_state_dict(sub_sd(sd, tag + "."), strict=True)
    return enc.to(DEV)


@pytest.mark.parametrize("tag", list(FORMS))
def test_reference_goldens(tag):
    """The four reference-made forms at the tolerances tests/test_encoder_gpu.py holds the reference-made encoder goldens to: 1e-5, and
    1e-4 behind a UNet3D; inference path and autograd path; conv_in's gradients of the first two forms against the reference's."""
    a, sd = load_golden("g25_voxel_encoder.npz")
    enc = _encoder(tag, sd)
    x = T(a["x"]).to(DEV)
    tol = 1e-4 if tag == "grid_unet" else 1e-5
    with torch.no_grad():
        fea = enc(x)
    out = enc(x)
    names = [k[len(tag) + 5:] for k in a if k.startswith(tag + ".fea.")]
    assert list(fea) == ([n for n in ref.PLANES if n in names] if tag == "planes" else ["grid"]) and sorted(fea) == sorted(names)
    for n in names:
        want = T(a[f"{tag}.fea.{n}"])
        assert fea[n].shape == want.shape
        assert float((fea[n].cpu() - want).abs().max()) <= tol and float((out[n].detach().cpu() - want).abs().max()) <= tol, (tag, n)
    if tag in ("grid", "planes"):
        sum((out[n] * T(a[f"{tag}.up.{n}"]).to(DEV)).sum() for n in names).backward()
        for prm, key in ((enc.conv_in.weight, "weight"), (enc.conv_in.bias, "bias")):
            want = T(a[f"{tag}.grad.{key}"])
            assert float((prm.grad.cpu() - want).abs().max()) <= 2e-4 * max(1.0, float(want.abs().max())), (tag, key)


@pytest.mark.parametrize("dims,R,C,k", CASES)
def test_forward_against_float64(dims, R, C, k):
    from vtaco_amd.ops import voxel_encoder as ve
    scene0 = {}
    for B in (1, 2):
        c = _case(dims, R, C, k, B)
        x, w, b = _dev(c)
        grid = ve.encode_grid(x, w, b, R, PAD)
        assert grid.shape == (B, R, R, R, C) and torch.equal(grid, ve.encode_grid(x, w, b, R, PAD))
        got = {"grid": grid.permute(0, 4, 1, 2, 3)}
        for sub in SUBSETS:
            planes = ve.encode_planes(x, w, b, R, PAD, sub)
            assert planes.shape == (len(sub) * B, C, R, R) and torch.equal(planes, ve.encode_planes(x, w, b, R, PAD, sub))
            for n, p in zip(sub, planes.split(B, dim=0)):
                if len(sub) == 1:
                    got[n] = p
                else:
                    assert torch.equal(p, got[n]), (sub, n)          # a plane does not depend on which others are asked for
        for n, v in got.items():
            tag = f"fwd {dims}->{R} C{C} k{k} B{B} {n}"
            _ratio(tag, v, c["out64"][n], c["out32"][n], c["bound"][n])
            ids, cells = ref.cell_ids(dims, R, PAD, n)
            empty = T(np.bincount(ids, minlength=cells) == 0).reshape(v.shape[2:])
            assert dims != (5, 6, 7) or bool(empty.any())             # D < R leaves cells without a voxel ...
            assert int(torch.count_nonzero(v.cpu()[:, :, empty])) == 0, tag     # ... which are exactly 0
            if B == 1:
                scene0[n] = v.clone()
            else:
                assert torch.equal(v[:1], scene0[n]), tag             # scene 0 does not depend on the batch around it


@pytest.mark.parametrize("dims,R,C,k", CASES)
def test_weight_gradient_against_float64(dims, R, C, k):
    from vtaco_amd.ops import voxel_encoder as ve
    for B in (1, 2):
        c = _case(dims, R, C, k, B)
        assert c["min_pre"] >= 1e-5, (dims, C, k, c["min_pre"])       # the ReLU masks are safe from f32 rounding: checked before any launch
        x, w, b = _dev(c)
        for which, names in (("grid", ("grid",)), ("planes", ref.PLANES), ("xy", ("xy",)), ("both", ("grid",) + ref.PLANES)):
            up = _up(c, names, 7 + B)
            dw64, db64, dwb, dbb = ref.backward(c["x"], c["w"], c["b"], R, PAD, up)
            _, dw32, db32 = ref.host32(c["x"], c["w"], c["b"], R, PAD, names, up)
            kw = {}
            if "grid" in names:
                kw["grad_grid"] = T(np.ascontiguousarray(up["grid"].transpose(0, 2, 3, 4, 1))).to(DEV)
            sub = tuple(n for n in names if n != "grid")
            if sub:
                kw.update(grad_planes=T(_stack(up, sub)).to(DEV), planes=sub)
            dw, db = ve.encode_bwd(x, w, b, PAD, **kw)
            again = ve.encode_bwd(x, w, b, PAD, **kw)
            assert dw.shape == w.shape and db.shape == b.shape and torch.equal(dw, again[0]) and torch.equal(db, again[1])
            tag = f"bwd {dims}->{R} C{C} k{k} B{B} up on {which}"
            _ratio(tag + " dW", dw, dw64, dw32, dwb)
            _ratio(tag + " dbias", db, db64, db32, dbb)


def test_tables_are_cached_per_shape():
    from vtaco_amd.ops import voxel_encoder as ve
    c = _case((5, 6, 7), 8, 32, 3, 2)
    x, w, b = _dev(c)
    ve.encode_grid(x, w, b, 8, PAD)
    ve.encode_planes(x, w, b, 8, PAD)
    n = len(ve._tables)
    key = ((5, 6, 7), 8, PAD, torch.device(DEV), "grid")
    first = ve._tables[key]
    ve.encode_grid(x, w, b, 8, PAD)
    ve.encode_planes(x, w, b, 8, PAD, ("xz",))
    ve.encode_bwd(x, w, b, PAD, grad_grid=torch.zeros(2, 8, 8, 8, 32, device=DEV))
    assert len(ve._tables) == n and ve._tables[key] is first and ve.tables((5, 6, 7), 8, PAD, DEV).buf.data_ptr() == first.buf.data_ptr()
    ve.encode_grid(x, w, b, 4, PAD)                                   # another resolution is another table
    assert len(ve._tables) == n + 1


def test_unsupported_shapes_raise():
    from vtaco_amd._lib import VtError
    from vtaco_amd.encoder import encoder_dict
    from vtaco_amd.ops import voxel_encoder as ve
    x = torch.zeros(1, 4, 4, 4, device=DEV)
    for C in (16, 48, 160):
        w, b = torch.zeros(C, 1, 3, 3, 3, device=DEV), torch.zeros(C, device=DEV)
        with pytest.raises(VtError, match="multiple of 32"):
            ve.encode_grid(x, w, b, 4)
        with pytest.raises(VtError, match="multiple of 32"):
            ve.encode_planes(x, w, b, 4)
        with pytest.raises(VtError, match="multiple of 32"):
            ve.encode_bwd(x, w, b, grad_grid=torch.zeros(1, 4, 4, 4, C, device=DEV))
    enc = encoder_dict["voxel_simple_local"](c_dim=48, grid_resolution=4, plane_type="grid").to(DEV)
    with pytest.raises(VtError, match="multiple of 32"):              # the encoder does not quietly take the host route
        enc(x)
    w, b = torch.zeros(32, 1, 3, 3, 3, device=DEV), torch.zeros(32, device=DEV)
    with pytest.raises(VtError):
        ve.encode_grid(torch.zeros(1, 4, 1, 4, device=DEV), w, b, 4)  # a dimension below 2
    with pytest.raises(VtError):
        ve.encode_planes(x, w, b, 4, PAD, ("xz", "grid"))
    with pytest.raises(VtError, match="HIP device"):
        ve.encode_grid(x.cpu(), w, b, 4)


@pytest.mark.parametrize("tag", ["grid", "planes"])
def test_hip_and_host_knobs_agree(tag):
    """VTACO_VOXEL_ENCODER=host (nn.Conv3d + the point encoders' scatter-means on the generated coordinates) against the fused
    kernels, outputs and conv_in gradients: each within the float64 gate of the same reference."""
    a, sd = load_golden("g25_voxel_encoder.npz")
    x = a["x"]
    w, b = sd[f"{tag}.conv_in.weight"].numpy(), sd[f"{tag}.conv_in.bias"].numpy()
    names = ref.PLANES if tag == "planes" else ("grid",)
    up = {n: a[f"{tag}.up.{n}"] for n in names}
    out64, bound, pre = ref.forward(x, w, b, 8, PAD, names)
    assert float(np.abs(pre).min()) >= 1e-5
    out32, dw32, db32 = ref.host32(x, w, b, 8, PAD, names, up)
    dw64, db64, dwb, dbb = ref.backward(x, w, b, 8, PAD, up)
    for knob in ("hip", "host"):
        enc = _encoder(tag, sd)
        enc.voxel_encoder = knob
        with torch.no_grad():
            plain = enc(T(x).to(DEV))
        out = enc(T(x).to(DEV))
        sum((out[n] * T(up[n]).to(DEV)).sum() for n in names).backward()
        for n in names:
            assert torch.equal(plain[n], out[n].detach()) or knob == "host"
            _ratio(f"{knob} {tag} {n}", out[n], out64[n], out32[n], bound[n])
            _ratio(f"{knob} {tag} {n} (no grad)", plain[n], out64[n], out32[n], bound[n])
        _ratio(f"{knob} {tag} dW", enc.conv_in.weight.grad, dw64, dw32, dwb)
        _ratio(f"{knob} {tag} dbias", enc.conv_in.bias.grad, db64, db32, dbb)


def test_unet3d_wiring_on_the_hip_kernels():
    """A UNet3D the HIP conv kernels cover behind the fused grid: the inference route (forward_channels_last) and the training route
    (forward_channels_last_train) against the module's own forward on the same mean grid; gradients reach conv_in."""
    from vtaco_amd.encoder import encoder_dict
    torch.manual_seed(3)
    enc = encoder_dict["voxel_simple_local"](c_dim=32, grid_resolution=8, plane_type="grid", unet3d=True,
                                             unet3d_kwargs=dict(num_levels=2, f_maps=32, in_channels=32, out_channels=32)).to(DEV)
    assert enc.unet3d.hip_supported()
    x = T(_case((5, 6, 7), 8, 32, 3, 2)["x"]).to(DEV)
    with torch.no_grad():
        fast = enc(x)["grid"]
        mean = enc._mean_grid_cl(x)
        want = enc.unet3d(mean)
    scale = max(1.0, float(want.abs().max()))
    assert fast.shape == want.shape == (2, 32, 8, 8, 8) and float((fast - want).abs().max()) <= 1e-4 * scale
    out = enc(x)["grid"]
    assert float((out.detach() - want).abs().max()) <= 1e-4 * scale
    out.square().sum().backward()
    for prm in (enc.conv_in.weight, enc.conv_in.bias):
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0
