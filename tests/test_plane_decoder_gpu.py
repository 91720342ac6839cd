"""GPU: LocalDecoder / AttentionDecoder on plane features.  Logits against the real reference's (tests/golden/g21_plane_decode.npz)
at the project's 1e-4 parity bar in "f32" and "f16x3"; gradients under the gate of tests/plane_decode_ref.py with F.grid_sample and
F.linear made to raise.  ReLU flips: as tests/test_decode_train_f64_gpu.py does, the float64 backward takes the activation masks and
layer inputs from the kernels' own save buffer; every gradient is compared with the reference's own at the parity bar as well."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_decode_ref as ref
from test_plane_decode_ref_cpu import load_case, sample_index

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0


@pytest.fixture
def no_framework_ops(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a framework operator was reached")
    monkeypatch.setattr(F, "grid_sample", boom)
    monkeypatch.setattr(F, "linear", boom)


def _decoder(case, kind="simple_local", **kw):
    from vtaco_amd.conv_onet.models import decoder_dict
    hidden = case["sd"]["fc_p.weight"].shape[0]
    dec = decoder_dict[kind](dim=3, c_dim=32, hidden_size=hidden, n_blocks=5, leaky=case["leaky"], padding=0.1, **kw)
    missing = dec.load_state_dict(case["sd"], strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("fuser")] and not missing.unexpected_keys
    return dec.to(DEV)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("tag", ["A", "B"])
def test_logits_match_the_reference(tag, precision, no_framework_ops):
    case = load_case(tag)
    dec = _decoder(case).eval()
    dec.precision = precision
    c_plane = {k: v.to(DEV) for k, v in case["c_plane"].items()}            # B: grid, yz, xz, xy -- the shuffled order
    with torch.no_grad():
        got = dec(case["p"].to(DEV), c_plane).cpu()
    err = float((got - case["logits"]).abs().max())
    print(f"plane decoder {tag} {precision}: max |logit diff| vs the reference {err:.3e}")
    assert err <= 1e-4


def _kernel_saves(dec, c, p):
    """(rx [nb,B,N,H], rh [nb,B,N,H], af [B,N,H]) from the training forward's own save buffer on the sampled features ``c``: the layer
    inputs whose signs are the activation masks (the kernels are deterministic: the same bits the autograd node kept)."""
    from vtaco_amd import ops
    B, N, C = c.shape
    H, nb, P = dec.hidden_size, dec.n_blocks, B * N
    if dec._wide:
        out, save = ops.decode_mlp_fwd_wide_train(c, dec._blob(), p, H, nb, dec.leaky)
        blk = save[P * C:P * C + 2 * nb * P * H].view(nb, 2, B, N, H).cpu()
        return out, blk[:, 0], blk[:, 1], save[P * C + 2 * nb * P * H:].view(B, N, H).cpu()
    out, save = ops.decode_mlp_fwd_train(c, dec._blob(), p)
    sv = save.view(12, B, N, 32).cpu()
    return out, sv[1:6], sv[6:11], sv[11]


@pytest.mark.parametrize("tag", ["A", "B"])
def test_gradients(tag, no_framework_ops):
    """d planes, d grid and every parameter gradient of logits.sum() through the decoder's own autograd route, each under the gate
    against the float64 backward of tests/plane_decode_ref.py run on the kernels' own saved layer inputs (the ReLU-flip treatment of
    tests/test_decode_train_f64_gpu.py), e32 from the same backward in float32, the floor from the same sums over magnitudes; and,
    in addition, against the reference's own gradients (g21) at the parity bar."""
    case = load_case(tag)
    dec = _decoder(case).train()
    p = case["p"].to(DEV)
    feats = {k: v.to(DEV).requires_grad_(True) for k, v in case["c_plane"].items()}
    logits = dec(p, feats)
    assert float((logits.detach().cpu() - case["logits"]).abs().max()) <= 1e-4
    logits.sum().backward()
    with torch.no_grad():
        vol, planes = dec._features_of({k: v.detach() for k, v in feats.items()})
        c = dec._sample(p, vol, planes)
        out2, rx, rh, af = _kernel_saves(dec, c, p)
    assert torch.equal(out2, logits.detach())                      # the saves are those of the forward the decoder ran
    sd = {k: v for k, v in case["sd"].items() if not k.startswith("fc_p_img")}
    go = torch.ones(case["p"].shape[:2])
    args = (sd, case["p"], c.cpu(), rx, rh, af, go, case["leaky"])
    r64, r32 = ref.mlp_backward(*args, dtype=torch.float64), ref.mlp_backward(*args, dtype=torch.float32)
    bnd = ref.mlp_backward(*args, dtype=torch.float64, absolute=True)
    worst = 0.0

    def gate(name, got, a64, a32, b):
        nonlocal worst
        ratio, e32 = ref.gate_ratio(got, a64, a32, b)
        print(f"RATIO {tag} d {name}: {ratio:.3f} (e32 {e32:.3e})")
        worst = max(worst, ratio)
        return ratio

    bad = []
    params = dict(dec.named_parameters())
    for name in sorted(sd):
        assert params[name].grad is not None, name
        if gate(name, params[name].grad, r64[name], r32[name], bnd[name]) > GATE:
            bad.append(name)
    f64 = ref.feature_grads(case["c_plane"], case["p"], r64["grad_c"], dtype=torch.float64)
    f32 = ref.feature_grads(case["c_plane"], case["p"], r32["grad_c"], dtype=torch.float32)
    fb = ref.feature_grads(case["c_plane"], case["p"], bnd["grad_c"], dtype=torch.float64, absolute=True)
    for k in case["keys"]:
        assert feats[k].grad is not None and feats[k].grad.shape == feats[k].shape, k
        if gate(k, feats[k].grad, f64[k], f32[k], fb[k]) > GATE:
            bad.append(k)
    assert not bad, f"{tag}: above the gate of {GATE}: {bad} (worst ratio {worst:.3f})"
    # in addition: the reference's own gradients, at the parity bar relative to the tensor's size
    for k in case["keys"]:
        want = case["grad"][k]
        assert float((feats[k].grad.cpu() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max())), k
    for name in sorted({n.rsplit(".", 1)[0] for n in case["pgrad"]}):
        g = params[name].grad.reshape(-1).cpu()
        s, sa = case["pgrad"][name + ".sum"]
        want = torch.from_numpy(case["pgrad"][name + ".samples"])
        assert abs(float(g.double().sum()) - s) <= 1e-4 * max(1.0, sa), name
        assert float((g[sample_index(name, g.numel())] - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max())), name


def test_attention_decoder_forward_img_with_planes(no_framework_ops):
    from seeded_fill import seeded_fill
    from vtaco_amd.conv_onet.models import decoder_dict
    g = torch.Generator().manual_seed(11)
    B, N, C, R = 1, 64, 32, 9
    dec = seeded_fill(decoder_dict["attention_local"](dim=3, c_dim=C, hidden_size=32, n_blocks=5, padding=0.1), 5).to(DEV).eval()
    planes = {k: torch.randn(B, C, R, R, generator=g) for k in ("yz", "xz", "xy")}
    p = (torch.rand(B, N, 3, generator=g) - 0.5) * 1.2
    c_img = torch.randn(B, N, C, generator=g) * (torch.rand(B, N, 1, generator=g) < 0.3)
    with torch.no_grad():
        got = dec.forward_img(p.to(DEV), {k: v.to(DEV) for k, v in planes.items()}, c_img.to(DEV)).cpu()
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    c = ref.features(planes, p, dtype=torch.float32)
    fused = ref.orc.transformer_fusion({k[len("fuser."):]: v for k, v in sd.items() if k.startswith("fuser.")}, c_img, c)
    want = ref.forward(sd, p, None, dtype=torch.float32, c=fused)
    err = float((got - want).abs().max())
    print(f"attention decoder on planes: max |logit diff| {err:.3e}")
    assert err <= 1e-4
    # under autograd the planes get gradients through the same sampler
    dec.train()
    leaf = {k: v.to(DEV).requires_grad_(True) for k, v in planes.items()}
    dec.forward_img(p.to(DEV), leaf, c_img.to(DEV)).sum().backward()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0 for v in leaf.values())


def test_refused_routes_name_the_missing_kernel():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.models import decoder_dict
    dec = decoder_dict["simple_local"](dim=3, c_dim=32, hidden_size=32, with_contact=True).to(DEV)
    planes = {k: torch.zeros(1, 32, 5, 5, device=DEV) for k in ("xz", "xy", "yz")}
    p = torch.zeros(1, 4, 3, device=DEV)
    with pytest.raises(VtError, match="vt_decode_mlp_fwd"):
        dec.forward_img(p, planes, torch.zeros(1, 4, 32, device=DEV))
    with pytest.raises(VtError, match="vt_decode_mlp_fwd"):
        dec.forward_contact(p, planes)
    with pytest.raises(VtError, match="vt_decode_fwd_ids"):
        dec.decode_lattice_ids(planes, 8, torch.zeros(1, 512, dtype=torch.uint8, device=DEV), torch.zeros(5, 32, device=DEV))
    near = decoder_dict["simple_local"](dim=3, c_dim=32, hidden_size=32, sample_mode="nearest").to(DEV)
    with pytest.raises(VtError, match="vt_sample_grid"):           # the volume next to planes under 'nearest': no nearest form of vt_sample_grid
        near(p, dict(planes, grid=torch.zeros(1, 32, 4, 4, 4, device=DEV)))
    with torch.no_grad():
        assert near(p, planes).shape == (1, 4)                     # planes alone under 'nearest' are built
    with pytest.raises(VtError, match="pts .* or .*lattice"):
        ops.planes.sample_planes(planes)
    with pytest.raises(VtError):
        dec(p, {"xw": planes["xz"]})
    with pytest.raises(VtError):
        dec(p, {})


def test_grid_alone_is_the_fused_kernel_bit_for_bit():
    from vtaco_amd import ops
    case = load_case("A")
    dec = _decoder(case).eval()
    g = torch.Generator().manual_seed(3)
    grid = torch.randn(2, 32, 6, 6, 6, generator=g).to(DEV)
    p = case["p"].to(DEV)
    with torch.no_grad():
        got = dec(p, {"grid": grid})
        want = ops.decode_fwd(grid, dec._blob(precision="f32"), pts=p, padding=0.1, precision="f32")
        lat = dec.decode_lattice({"grid": grid[:1]}, 8, precision="f32")
        lat_want = ops.decode_fwd(grid[:1], dec._blob(precision="f32"), padding=0.1, lattice=(8, 1.1, 0, 512), precision="f32")
    assert torch.equal(got, want) and torch.equal(lat, lat_want)


def test_decode_lattice_with_planes_is_the_point_decode():
    """Slabs included (LATTICE_SLAB_POINTS lowered for the test), with and without the grid, bit for bit in f32."""
    from vtaco_amd.common import make_3d_grid
    from vtaco_amd.conv_onet.models import decoder as decmod
    case = load_case("B")
    dec = _decoder(case).eval()
    c_plane = {k: v[:1].to(DEV) for k, v in case["c_plane"].items()}
    nx = 12
    pts = (1.1 * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (nx,) * 3)).unsqueeze(0).to(DEV)
    old = decmod.LATTICE_SLAB_POINTS
    try:
        decmod.LATTICE_SLAB_POINTS = 500
        with torch.no_grad():
            for feats in (c_plane, {k: v for k, v in c_plane.items() if k != "grid"}):
                want = dec(pts, feats)
                assert torch.equal(dec.decode_lattice(feats, nx, precision="f32"), want)
                assert torch.equal(dec.decode_lattice(feats, nx, first=7, count=1001, precision="f32"), want[:, 7:1008])
    finally:
        decmod.LATTICE_SLAB_POINTS = old


@pytest.mark.parametrize("tag", ["A", "B"])
def test_decode_lattice_f16x3_is_the_point_decode(tag):
    """The default arithmetic: the split-f16 MLP on a lattice slab's given features (whole x-plane pairs -- the kernel's brick tiling --
    and a ragged slab) gives the bits of the point decode of the same points, narrow and wide."""
    from vtaco_amd.common import make_3d_grid
    case = load_case(tag)
    dec = _decoder(case).eval()
    dec.precision = "f16x3"
    c_plane = {k: v[:1].to(DEV) for k, v in case["c_plane"].items()}
    nx = 16
    pts = (1.1 * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (nx,) * 3)).unsqueeze(0).to(DEV)
    with torch.no_grad():
        want = dec(pts, c_plane)
        whole = dec.decode_lattice(c_plane, nx, precision="f16x3")                          # first 0, count a multiple of 2 nx^2
        pair = dec.decode_lattice(c_plane, nx, first=2 * nx * nx, count=4 * nx * nx, precision="f16x3")
        ragged = dec.decode_lattice(c_plane, nx, first=nx * nx + 3, count=2 * nx * nx + 7, precision="f16x3")
        flat = torch.empty(nx ** 3, device=DEV)
        dec.decode_lattice(c_plane, nx, precision="f16f8", out=flat)                        # runs as f16x3; a [count] out for one scene
    assert torch.equal(whole, want) and torch.equal(flat, want[0])
    assert torch.equal(pair, want[:, 2 * nx * nx:6 * nx * nx])
    assert torch.equal(ragged, want[:, nx * nx + 3:3 * nx * nx + 10])
