"""GPU: the UNet3D layer family (csrc/unet3d.hip) against float64 references at non-cubic and ragged volumes.

Every conv is compared elementwise with tests/unet3d_ref.py: |kernel - ref| <= gate * bound, bound = the same sum over absolute values.
The reference is fed the kernel's OWN (scale, shift) table, read back, so the gate holds the convolution's arithmetic alone (ReLU is
1-Lipschitz: no branch to flip); the table is gated separately against float64 GroupNorm.  Gates, with K = 27 (C1 + C2):
  exact f32, split-f16, IEEE-half pairs   1.5e-7 sqrt(K)          (the project's constant for two f32-accumulating kernels)
  split-bf16                              2^-16 + 1.5e-7 sqrt(K)  (the per-product error the kernel's header documents)
  weight gradients, K = B D H W           2e-7 sqrt(K)
  out_part per block                      1e-5 of the block's sum |y| / sum y^2, from float64 sums of the kernel's own output
  vt_gn_scale_shift                       1e-5 relative on scale, 1e-5 of |beta| + |mean scale| on shift
  vt_gn_bwd*                              1e-5 of the reference's largest entry (float64 autograd of group_norm)
Every case asserts which kernel served it: the host plans (conv_tile / conv_waves / conv_use_ksplit, conv_h_tz, conv_s_tz, conv_sk_plan)
are mirrored here and checked against the library's queries.  Each test prints every measured ratio before it asserts on it."""
import os
import sys
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet3d_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
_KNOBS = ("VTACO_CONV_KSPLIT", "VTACO_CONV_THIN", "VTACO_CONV_TZ", "VTACO_CONV_HTZ", "VTACO_CONV_HTHIN", "VTACO_CONV_SPEC", "VTACO_CONV_UP")


@pytest.fixture(autouse=True)
def _default_plans():
    for knob in _KNOBS:
        if os.environ.get(knob):
            pytest.skip(f"the conv plan is forced or turned off by {knob}")


def _report(tag, value, gate):
    print(f"RATIO {tag}: {value:.3e} (gate {gate:.3e})")
    return value


def _check(tag, got, ref, bound, gate):
    """Print the largest error / bound, then assert it elementwise against the gate."""
    _report(tag, R.ratio(got, ref, bound), gate)
    return R.assert_within(got, ref, bound, gate, tag)


# ---- the split kernels' plans (unet3d.hip), mirrored ---------------------------------------------------------------------------------

def _t8(B, D, H, W, Cout):
    return (D // 8) * (H // 8) * (W // 8) * B * (Cout // 32)


def _h_tz(B, D, H, W, Cout):
    """conv_h_tz: the persistent split-f16 kernel's tile depth (0: not covered)."""
    t8 = _t8(B, D, H, W, Cout)
    return 8 if t8 >= 256 else 4 if 2 * t8 >= 128 else 0


def _s_tz(B, D, H, W, Cout):
    """conv_s_eligible + conv_s_tz: the split-bf16 / half-pair kernel's tile depth (0: not covered)."""
    t8 = _t8(B, D, H, W, Cout)
    return 8 if t8 >= 512 else 4 if t8 >= 64 else 2 if (D // 2) * (H // 8) * (W // 8) * B * (Cout // 32) >= 64 else 0


def _sk_plan(B, D, H, W, Cin, Cout):
    """conv_sk_plan: (tile depth, K slices) of the K-split form, (0, 0) where it steps aside."""
    ncq, t8 = Cin // 16, _t8(B, D, H, W, Cout)
    if 4 * t8 > 128 or ncq < 8:
        return 0, 0
    for ks in (8, 4, 2):
        if ncq % ks == 0 and 128 <= t8 * ks <= 256:
            return 8, ks
    best = 0
    for ks in (2, 4, 8):
        if ncq % ks == 0:
            best = ks
            if 4 * t8 * ks >= 256:
                break
    return (2, best) if best else (0, 0)


# ---- one layer's inputs on the device, the kernel's own scale / shift (gated), and the float64 reference built on it -----------------

def _stats_gate(ss, x, low, gamma, beta, groups, tag):
    r_scale, r_shift = R.stats_ratios(ss, R.gn_scale_shift64(x, low, gamma, beta, groups, EPS), beta)
    _report(tag + " scale", r_scale, 1e-5)
    _report(tag + " shift", r_shift, 1e-5)
    assert r_scale <= 1e-5 and r_shift <= 1e-5, (tag, r_scale, r_shift)


@lru_cache(maxsize=4)                    # (consecutive tests share a shape; nothing older is worth its device tensors and float64 reference)
def _layer(B, D, H, W, C1, C2, Cout, relu=True, groups=8, seed=1, keep=0.3):
    """Inputs drawn on the CPU, vt_channel_stats + vt_gn_scale_shift on the device (gated against float64 GroupNorm), and (ref, bound)
    of the conv from the kernel's own table.  Computed once per case and shared; nobody writes to it."""
    from vtaco_amd import ops
    x, low, w, gamma, beta = R.make_layer(torch.Generator().manual_seed(seed), B, D, H, W, C1, C2, Cout, keep=keep)
    xd, ld, wd = x.to(DEV), (low.to(DEV) if C2 else None), w.to(DEV)
    ss = ops.gn_scale_shift(ops.channel_stats(xd), ops.channel_stats(ld) if C2 else None, C1, C2, B, D * H * W, gamma.to(DEV), beta.to(DEV),
                            groups, EPS, DEV)
    _stats_gate(ss, x, low, gamma, beta, groups, f"gn_scale_shift {B}x{D}x{H}x{W} {C1}+{C2} g{groups}")
    ref, bound = R.gcr64(x, low, ss, w, relu)
    return SimpleNamespace(x=x, low=low, w=w, gamma=gamma, beta=beta, xd=xd, ld=ld, wd=wd, ss=ss, ref=ref, bound=bound, Cin=C1 + C2)


def _part_gate(part, out, tile, tag, wgs=0, owner=None):
    want, bound = R.tile_sums64(out, tile, wgs, owner)
    assert tuple(part.shape) == tuple(want.shape), (tag, tuple(part.shape), tuple(want.shape))
    return _check(tag + " out_part", part, want, bound, 1e-5)


# ---- a. the exact-f32 kernel alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.F32_CASES, ids=[c[0] for c in R.F32_CASES])
def test_f32_conv_at_ragged_volumes(case):
    """vt_conv3d_gcr on every route of its plan -- TX = 4 / 16 / 32 with ragged tails on every axis, the K-split widths 2 and 4 over the
    virtual concat (a GroupNorm group straddling x | low), conv_launch<1,1> <1,2> <1,4> <1,8> <2,8> <4,8>, no ReLU, 1 / 4 / 32 groups --
    against float64 at 1.5e-7 sqrt(K); its out_part per ragged tile at 1e-5.  Largest ratios measured on the MI355X: conv 6.4e-7
    (launch<4,8>; gate 4.4e-6), K-split 1.5e-7 (gate 7.6e-6), out_part 2.1e-7, scale / shift 6.4e-7."""
    from vtaco_amd import _lib, ops
    name, B, D, H, W, C1, C2, Cout, relu, groups, route, tile = case
    L = _layer(B, D, H, W, C1, C2, Cout, relu, groups)
    kind, what, got_tile, n = R.conv_plan(B, D, H, W, C1 + C2, Cout)
    assert (kind, what) == route and got_tile == tile
    assert n == _lib.load().vt_conv3d_stat_blocks(B, D, H, W, C1 + C2, Cout)
    out, (part, nblk) = ops.conv3d_gcr(L.xd, L.ld, L.ss, ops.conv3d_pack(L.wd), Cout, relu=relu)
    assert nblk == n                                                   # the intended plan ran
    gate = R.gate_f32(L.Cin)
    _check(f"f32 {name}", out, L.ref, L.bound, gate)
    _part_gate(part, out, tile, f"f32 {name}")


# ---- b. the split forward kernels, each once at a non-cubic volume --------------------------------------------------------------------

SPLIT_CASES = [
    # (id, kind, B, D, H, W, C1, C2, Cout, tile depth)
    ("f16x3-tz8", "f16x3", 2, 16, 32, 64, 32, 0, 64, 8),
    ("f16x3-tz4", "f16x3", 1, 16, 32, 64, 32, 0, 32, 4),
    ("f16x3-tz4-low", "f16x3", 1, 16, 32, 64, 32, 64, 32, 4),
    ("bf16x3-tz8", "bf16x3", 2, 16, 32, 64, 32, 0, 128, 8),
    ("bf16x3-tz4", "bf16x3", 1, 16, 32, 64, 32, 0, 32, 4),
    ("bf16x3-tz2", "bf16x3", 2, 8, 16, 32, 32, 0, 32, 2),
    ("thin-tz8", "thin", 2, 16, 32, 64, 32, 0, 128, 8),
    ("thin-tz4", "thin", 1, 16, 32, 64, 32, 0, 32, 4),
    ("thin-tz2", "thin", 2, 8, 16, 32, 32, 0, 32, 2),
]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_convs_at_non_cubic_volumes(case):
    """vt_conv3d_gcr_f16x3 (tile depths 8 and 4, plain and over the virtual concat), vt_conv3d_gcr_bf16x3 and vt_conv3d_gcr_f16x3_thin
    (depths 8, 4, 2) at D != H != W against float64; out_part per tile (per persistent workgroup for the split-f16 kernel: the tiles
    wg, wg + wgs, ...) from the kernel's own output.  Largest ratios measured on the MI355X: split-f16 2.8e-7 and half pairs 3.3e-7
    (gate 4.4e-6), split-bf16 2.5e-6 (gate 2.0e-5), out_part 2.9e-7."""
    from vtaco_amd import _lib, ops
    lib = _lib.load()
    name, kind, B, D, H, W, C1, C2, Cout, tz = case
    L = _layer(B, D, H, W, C1, C2, Cout)
    nsp = (D // tz) * (H // 8) * (W // 8)
    if kind == "f16x3":
        assert _h_tz(B, D, H, W, Cout) == tz
        wgs = lib.vt_conv3d_stat_blocks_f16x3(B, D, H, W, L.Cin, Cout)
        assert wgs == min(nsp, max(1, torch.cuda.get_device_properties(0).multi_processor_count // (B * (Cout // 32))))
        out, (part, nblk) = ops.conv3d_gcr(L.xd, L.ld, L.ss, None, Cout, packed_w_f16x3=ops.conv3d_pack(L.wd, "f16x3"))
        assert nblk == wgs
        gate = R.gate_f32(L.Cin)
    else:
        assert _s_tz(B, D, H, W, Cout) == tz and _sk_plan(B, D, H, W, L.Cin, Cout) == (0, 0)
        assert lib.vt_conv3d_ksplit_workspace_bytes(B, D, H, W, L.Cin, Cout) == 0
        assert lib.vt_conv3d_stat_blocks_bf16x3(B, D, H, W, L.Cin, Cout) == nsp
        thin = kind == "thin"
        out, (part, nblk) = ops.conv3d_gcr(L.xd, L.ld, L.ss, None, Cout, packed_w_bf16x3=ops.conv3d_pack(L.wd, "f16x3_thin" if thin else "bf16x3"),
                                           thin_half=thin)
        assert nblk == nsp
        wgs = 0
        gate = R.gate_f32(L.Cin) if thin else R.gate_bf16x3(L.Cin)
    _check(name, out, L.ref, L.bound, gate)
    _part_gate(part, out, (8, 8, tz), name, wgs)


KSPLIT_CASES = [
    # (id, B, D, H, W, C1, C2, Cout, tile depth, slices)
    ("tz8-ks8", 1, 8, 16, 32, 128, 0, 128, 8, 8),
    ("tz8-ks4-low", 1, 8, 16, 32, 64, 128, 128, 8, 4),
    ("tz2-ks2", 2, 8, 8, 16, 160, 0, 32, 2, 2),
    ("tz2-ks4", 2, 8, 8, 16, 192, 0, 32, 2, 4),
    ("tz2-ks8-low", 2, 8, 8, 16, 128, 256, 32, 2, 8),
]


@pytest.mark.parametrize("half", [False, True], ids=["bf16x3", "thin"])
@pytest.mark.parametrize("case", KSPLIT_CASES, ids=[c[0] for c in KSPLIT_CASES])
def test_ksplit_convs_at_non_cubic_volumes(case, half):
    """vt_conv3d_gcr_bf16x3_ksplit / vt_conv3d_gcr_f16x3_thin_ksplit: 8^3 and 8 x 8 x 2 tiles, 2 / 4 / 8 slices of the input channels (the
    slice count read off the workspace size), 128 to 384 input channels, against float64; out_part per 128 consecutive voxels.  Largest
    ratios measured on the MI355X: split-bf16 9.0e-7 (gate 2.4e-5), half pairs 1.0e-7 (gate 9.9e-6), out_part 3.8e-7."""
    from vtaco_amd import _lib, ops
    lib = _lib.load()
    name, B, D, H, W, C1, C2, Cout, tz, ks = case
    L = _layer(B, D, H, W, C1, C2, Cout, keep=0.5)
    assert _sk_plan(B, D, H, W, L.Cin, Cout) == (tz, ks)
    assert lib.vt_conv3d_ksplit_workspace_bytes(B, D, H, W, L.Cin, Cout) == ks * B * D * H * W * Cout * 4
    out, (part, nblk) = ops.conv3d_gcr(L.xd, L.ld, L.ss, None, Cout, packed_w_bf16x3=ops.conv3d_pack(L.wd, "f16x3_thin" if half else "bf16x3"),
                                       thin_half=half)
    assert nblk == D * H * W // 128 == lib.vt_conv3d_stat_blocks_ksplit(B, D, H, W, L.Cin, Cout)
    gate = R.gate_f32(L.Cin) if half else R.gate_bf16x3(L.Cin)
    tag = f"ksplit {name} {'thin' if half else 'bf16x3'}"
    _check(tag, out, L.ref, L.bound, gate)
    blocks = out.double().cpu().reshape(B, nblk, 128, Cout)
    want = torch.stack((blocks.sum(2), (blocks * blocks).sum(2)), -1)
    bound = torch.stack((blocks.abs().sum(2), (blocks * blocks).sum(2)), -1)
    _check(tag + " out_part", part, want, bound, 1e-5)


def test_decoder_entry_per_parity_conv_vs_float64():
    """vt_conv3d_gcr_f16x3_up at 16 x 32 x 64 (tile depth 4) and a batch of two at depth 8 against float64 -- an independent yardstick for
    the kernel whose only non-cubic check was the f32 kernel.  Largest ratios measured on the MI355X: 1.6e-7 (gate 6.2e-6), out_part
    1.8e-7."""
    from vtaco_amd import _lib, ops
    lib = _lib.load()
    for B, D, H, W, C1, C2, Cout, tz in ((1, 16, 32, 64, 32, 64, 32, 4), (2, 32, 16, 64, 32, 32, 64, 8)):
        L = _layer(B, D, H, W, C1, C2, Cout)
        assert lib.vt_conv3d_up_covers(C1, C2, B, D, H, W, Cout) and _h_tz(B, D, H, W, Cout) == tz
        ph, pu = ops.conv3d_pack(L.wd, "f16x3"), ops.conv3d_pack_up(L.wd, C1)
        out, (part, nblk) = ops.conv3d_gcr(L.xd, L.ld, L.ss, None, Cout, packed_w_f16x3=ph, packed_w_up=pu)
        plain, _ = ops.conv3d_gcr(L.xd, L.ld, L.ss, None, Cout, packed_w_f16x3=ph)
        assert not torch.equal(out, plain)                            # the per-parity kernel ran (another summation order)
        assert nblk == lib.vt_conv3d_stat_blocks_f16x3(B, D, H, W, L.Cin, Cout)
        gate, tag = R.gate_f32(L.Cin), f"f16x3_up {D}x{H}x{W}"
        _check(tag, out, L.ref, L.bound, gate)
        _part_gate(part, out, (8, 8, tz), tag, nblk)


def test_final_conv_epilogue_vs_float64():
    """vt_conv3d_gcr_f16x3_final / _final_keep at 16 x 32 x 64: y_keep against the float64 layer, `out` against the float64 1x1x1 conv of
    the float64 ReLU output.  Gate of `out`: every y_c carries at most gate(27 Cin) bound_c and the 32-term pointwise sum adds
    1.5e-7 sqrt(32) of sum |W| |y_c| <= sum |W| bound_c, so |out - ref| <= (gate(27 Cin) + 1.5e-7 sqrt(32)) (|W| bound + |b|).
    Measured on the MI355X: y_keep 2.6e-7 (gate 4.4e-6), out 4.2e-8 (gate 5.3e-6)."""
    from vtaco_amd import ops
    B, D, H, W, C = 1, 16, 32, 64, 32
    L = _layer(B, D, H, W, C, 0, 32)
    assert ops.final_fusable(L.xd, 32) and _h_tz(B, D, H, W, 32) == 4
    g = torch.Generator().manual_seed(9)
    fw, fb = torch.randn(32, 32, generator=g) * 0.2, torch.randn(32, generator=g)
    ph, pf = ops.conv3d_pack(L.wd, "f16x3"), ops.conv1x1_pack_f16x3(fw.to(DEV))
    out = ops.conv3d_gcr_final(L.xd, L.ss, ph, pf, fb.to(DEV))
    y, out_k = ops.conv3d_gcr_final_keep(L.xd, L.ss, ph, pf, fb.to(DEV))
    assert torch.equal(out, out_k)
    gate = R.gate_f32(C)
    _check("final_keep y", y, L.ref, L.bound, gate)
    ref = L.ref @ fw.double().t() + fb.double()
    bound = L.bound @ fw.double().abs().t() + fb.double().abs()
    gate_out = gate + 1.5e-7 * 32 ** 0.5
    _check("final out", out, ref, bound, gate_out)


def test_flagged_blocks_scaled_inputs_and_xstats_vs_float64():
    """At 16 x 32 x 64: vt_conv3d_gcr_f16x3_skip with flags from vt_voxel_tile_flags (a small cloud: most blocks empty; its out_part per
    workgroup of the flagged tile deal, which also shows that the flagged walk served the call: the dense walk's rows miss the gate),
    vt_conv3d_gcr_f16x3_scaled with inputs at 1e-6 (without a GroupNorm table, as its callers use it: the rescale is for output
    gradients, and a shift would leave the half range with it -- the rescale combined with a table is not exercised), and vt_conv3d_gcr_f16x3_xstats (the data gradient and its (sum dxn, sum dxn x) per
    persistent workgroup) against float64.  Measured on the MI355X: _skip 6.7e-7, _scaled 5.6e-7, _xstats dxn 3.0e-7 (gate 4.4e-6 each),
    _skip's out_part per workgroup 1.6e-7 and the _xstats sums 5.3e-8 (gate 1e-5)."""
    from vtaco_amd import _lib, ops
    lib = _lib.load()
    B, D, H, W, C, Cout = 1, 16, 32, 64, 32, 32
    g = torch.Generator().manual_seed(31)
    # a cloud inside the volume, voxel ids on the 64^3 grid that contains it: the cube's flags over the volume's blocks are the volume's
    pts = (torch.rand(B, 40, 3, generator=g) * torch.tensor([20.0, 12.0, 6.0]) + torch.tensor([30.0, 10.0, 5.0])).long()       # x, y, z
    idx = (pts[..., 0] + 64 * (pts[..., 1] + 64 * pts[..., 2])).int()
    x = torch.zeros(B, D, H, W, C)
    for b in range(B):
        x[b, pts[b, :, 2], pts[b, :, 1], pts[b, :, 0]] = torch.randn(40, C, generator=g)
    cube = ops.voxel_tile_flags(SimpleNamespace(idx=idx.to(DEV).contiguous(), B=B, T=40, R=64))
    flags = cube.reshape(B, 8, 8, 8)[:, :D // 8, :H // 8, :W // 8].reshape(B, -1).contiguous()
    assert 0 < int((flags == 0).sum()) < flags.numel() // 2              # most blocks are empty
    w = torch.randn(Cout, C, 3, 3, 3, generator=g) * 0.05
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    xd, wd = x.to(DEV), w.to(DEV)
    ss = ops.gn_scale_shift(ops.channel_stats(xd), None, C, 0, B, D * H * W, gamma.to(DEV), beta.to(DEV), 8, EPS, DEV)
    _stats_gate(ss, x, None, gamma, beta, 8, "gn_scale_shift sparse grid")
    ref, bound = R.gcr64(x, None, ss, w, True)
    ph = ops.conv3d_pack(wd, "f16x3")
    assert ops.conv3d_skip_covers(xd, Cout)
    out, (part, nblk) = ops.conv3d_gcr_skip(xd, ss, ph, Cout, flags)
    dense, _ = ops.conv3d_gcr(xd, None, ss, None, Cout, packed_w_f16x3=ph)
    tz = _h_tz(B, D, H, W, Cout)
    assert tz == 4 and nblk == lib.vt_conv3d_stat_blocks_f16x3(B, D, H, W, C, Cout)
    assert float((out - dense).abs().max()) <= 2e-6 * max(1.0, float(dense.abs().max()))        # the project's bar between the two walks
    gate = R.gate_f32(C)
    _check("f16x3_skip", out, ref, bound, gate)
    # out_part per workgroup of the flagged deal; the rows of the dense walk (tiles wg, wg + wgs, ...) must NOT fit: the flags were taken
    owner = R.flagged_deal(flags, D, H, W, tz, nblk)
    assert not torch.equal(owner, (torch.arange(owner.shape[1]) % nblk).expand(B, -1))
    _part_gate(part, out, (8, 8, tz), "f16x3_skip", nblk, owner)
    dense_rows, dense_bound = R.tile_sums64(out, (8, 8, tz), nblk)
    assert _report("f16x3_skip out_part against the dense walk's rows", R.ratio(part, dense_rows, dense_bound), 1e-5) > 1e-5

    L = _layer(B, D, H, W, C, 0, Cout)
    assert lib.vt_conv3d_stat_blocks_f16x3(B, D, H, W, C, Cout) > 0          # the split-f16 kernel, which alone takes in_absmax
    tiny = (L.x * 1e-6).to(DEV)
    amax = tiny.abs().max().reshape(1)
    # (no GroupNorm table: the rescale is for output gradients, which carry none -- a shift would leave the half range with it)
    ref_s, bound_s = R.gcr64(tiny, None, None, L.w, False)
    out_s, _ = ops.conv3d_gcr(tiny, None, None, None, Cout, False, packed_w_f16x3=ops.conv3d_pack(L.wd, "f16x3"), in_absmax=amax)
    assert float(out_s.abs().max()) > 0.0
    _check("f16x3_scaled", out_s, ref_s, bound_s, gate)

    Cin = 64                                                             # the layer's input channels = the data gradient's outputs
    wl = torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.05
    gr = torch.randn(B, D, H, W, Cout, generator=g) * 1e-6 * (torch.rand(B, D, H, W, Cout, generator=g) < 0.5)
    xin = torch.randn(B, D, H, W, Cin, generator=g).relu()
    nb = lib.vt_conv3d_xstats_blocks(B, D, H, W, Cout, Cin)
    assert nb > 0
    grd, xind = gr.to(DEV), xin.to(DEV)
    got = ops.conv3d_dgrad_xstats(grd, ops.conv3d_pack_t(wl.to(DEV)), Cin, grd.abs().max().reshape(1), xind)
    assert got is not None
    dxn, (bpart, nblk) = got
    assert nblk == nb
    ref_d, bound_d = R.gcr64(gr, None, None, wl.flip(2, 3, 4).transpose(0, 1), False)
    gate_d = R.gate_f32(Cout)
    _check("f16x3_xstats dxn", dxn, ref_d, bound_d, gate_d)
    tz = _h_tz(B, D, H, W, Cin)
    assert tz == 4
    d64, x64 = dxn.double().cpu(), xin.double()
    s1, b1 = R.tile_sums64(d64, (8, 8, tz), nb)
    s2, b2 = R.tile_sums64(d64 * x64, (8, 8, tz), nb)
    want, bd = torch.stack((s1[..., 0], s2[..., 0]), -1), torch.stack((b1[..., 0], b2[..., 0]), -1)
    _check("f16x3_xstats sums", bpart, want, bd, 1e-5)


# ---- c. weight gradients ------------------------------------------------------------------------------------------------------------

WGRAD_CASES = [
    # (id, kernel, B, D, H, W, C1, C2, Cout)
    ("f32-ragged", "f32", 2, 3, 5, 7, 32, 0, 32),
    ("f32-low", "f32", 2, 6, 10, 14, 32, 64, 64),
    ("f16x3", "f16x3", 2, 6, 16, 24, 32, 0, 32),
    ("f16x3-low", "f16x3", 2, 6, 16, 24, 32, 64, 32),
    ("f16x3_up", "up", 2, 4, 16, 32, 32, 64, 32),
    ("f16x3_sparse", "sparse", 2, 8, 16, 24, 32, 0, 32),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_weight_gradients_at_non_cubic_volumes(case):
    """vt_conv3d_wgrad (ragged tiles, the virtual concat), vt_conv3d_wgrad_f16x3 (D even, H and W in eights), _up (sides in sixteens, D in
    fours) and _sparse (flags) against wgrad64 at 2e-7 sqrt(B D H W), with g at 1e-6 and g_absmax given; bit-reproducible.  Largest
    ratios measured on the MI355X: f32 1.2e-7 (gate 2.9e-6), f16x3 5.1e-8, _up 6.7e-8, _sparse 2.3e-7 (gates 1.3e-5 to 1.6e-5)."""
    from vtaco_amd import _lib, ops
    lib = _lib.load()
    name, kind, B, D, H, W, C1, C2, Cout = case
    g_ = torch.Generator().manual_seed(43)
    flags = None
    if kind == "sparse":
        x = torch.zeros(B, D, H, W, C1)
        x[:, 1:6, 2:7, 9:15] = torch.randn(B, 5, 5, 6, C1, generator=g_)      # inside block (0, 0, 1): the other five blocks are zero
        x[1] = 0                                                             # and a scene without input: the shift's share alone
        flags = torch.ones(B, (D // 8) * (H // 8) * (W // 8), dtype=torch.uint8)
        flags[0, 1] = 0
        _, low, w, gamma, beta = R.make_layer(g_, B, D, H, W, C1, C2, Cout)
    else:
        x, low, w, gamma, beta = R.make_layer(g_, B, D, H, W, C1, C2, Cout, keep=1.0)
    xd, ld = x.to(DEV), (low.to(DEV) if C2 else None)
    ss = ops.gn_scale_shift(ops.channel_stats(xd), ops.channel_stats(ld) if C2 else None, C1, C2, B, D * H * W, gamma.to(DEV), beta.to(DEV), 8, EPS, DEV)
    g = torch.randn(B, D, H, W, Cout, generator=g_) * (torch.rand(B, D, H, W, 1, generator=g_) < 0.6) * 1e-6
    gd = g.to(DEV)
    gmax = gd.abs().max().reshape(1)
    up_bytes = lib.vt_conv3d_wgrad_f16x3_up_workspace_bytes(B, D, H, W, C1, C2, Cout) if C2 else 0
    h_bytes = lib.vt_conv3d_wgrad_f16x3_workspace_bytes(B, D, H, W, C1 + C2, Cout)
    if kind == "f32":
        assert lib.vt_conv3d_wgrad_workspace_bytes(B, D, H, W, C1 + C2, Cout) > 0
        run = lambda: ops.conv3d_wgrad(xd, ld, ss, gd)
    elif kind == "f16x3":
        assert h_bytes > 0 and up_bytes == 0                                # the dense split-f16 kernel, not the per-parity one
        run = lambda: ops.conv3d_wgrad(xd, ld, ss, gd, precision="f16x3", g_absmax=gmax)
    elif kind == "up":
        assert up_bytes > 0
        run = lambda: ops.conv3d_wgrad(xd, ld, ss, gd, precision="f16x3", g_absmax=gmax)
    else:
        assert lib.vt_conv3d_wgrad_f16x3_sparse_workspace_bytes(B, D, H, W, C1, Cout) > 0
        run = lambda: ops.conv3d_wgrad_sparse(xd, ss, gd, flags.to(DEV), g_absmax=gmax)
    dw, again = run(), run()
    assert dw is not None and torch.equal(dw, again)
    ref, bound = R.wgrad64(x, low, ss, g)
    gate = R.gate_wgrad(B * D * H * W)
    _check(f"wgrad {name}", dw, ref, bound, gate)


# ---- d. the other layer types -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 6, 10, 14, 32), (2, 5, 7, 9, 32)], ids=["even", "odd"])
def test_maxpool_family_at_non_cubic_volumes(shape):
    """vt_maxpool3d_cl, _stats, _bwd and _bwd_fork at 6 x 10 x 14 and at the odd 5 x 7 x 9: bit for bit F.max_pool3d / its autograd (floor
    semantics, first maximum; ties among the ReLU zeros), or a VT_ERR_* refusal -- never silent garbage."""
    from vtaco_amd import ops
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(71)
    x = torch.randn(B, D, H, W, C, generator=g).relu()
    x[:, 0] = x[:, 1]                                                    # equal positive maxima inside the first windows along z
    xr = x.permute(0, 4, 1, 2, 3).clone().requires_grad_()
    want = F.max_pool3d(xr, 2)
    dy = torch.randn(want.shape, generator=g) * 1e-3
    (want * dy).sum().backward()
    want_cl = want.detach().permute(0, 2, 3, 4, 1).contiguous()
    xd, dyd = x.to(DEV), dy.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    got = ops.maxpool3d_cl(xd)
    assert torch.equal(got.cpu(), want_cl)
    got_s, (part, nblk) = ops.maxpool3d_cl_stats(xd)
    assert torch.equal(got_s, got)
    ref_part, ref_n = ops.channel_stats(got)
    assert nblk == ref_n and torch.equal(part, ref_part)
    odd = (D | H | W) & 1
    dskip = (torch.randn(B, D, H, W, C, generator=g) * 1e-3).to(DEV)
    if odd:
        with pytest.raises(ops.VtError):
            ops.maxpool3d_cl_bwd(xd, dyd)
        with pytest.raises(ops.VtError):
            ops.maxpool3d_cl_bwd_fork(xd, dskip, dyd)
        return
    dx = ops.maxpool3d_cl_bwd(xd, dyd)
    assert torch.equal(dx.cpu(), xr.grad.permute(0, 2, 3, 4, 1))
    fork, fmax = ops.maxpool3d_cl_bwd_fork(xd, dskip, dyd)
    want_f = torch.where(x > 0, dskip.cpu() + xr.grad.permute(0, 2, 3, 4, 1), torch.zeros(()))
    assert torch.equal(fork.cpu(), want_f) and float(fmax) == float(want_f.abs().max())


def test_channel_stats_with_uneven_blocks():
    """vt_channel_stats where the voxel count is no multiple of the block count (block blk holds voxels [V blk / n, V (blk + 1) / n)):
    each block's (sum, sumsq) against float64 at 1e-5 of sum |x| / sum x^2.  Largest ratio measured on the MI355X: 2.1e-7."""
    from vtaco_amd import ops
    for B, D, H, W, C in ((2, 3, 5, 7, 64), (1, 5, 7, 9, 32)):
        V = D * H * W
        x = torch.randn(B, D, H, W, C, generator=torch.Generator().manual_seed(V))
        part, n = ops.channel_stats(x.to(DEV))
        assert n == ops.stat_blocks(V) and V % n
        flat = x.double().reshape(B, V, C)
        rows = [flat[:, V * k // n:V * (k + 1) // n] for k in range(n)]
        want = torch.stack([torch.stack((r.sum(1), (r * r).sum(1)), -1) for r in rows], 1)
        bound = torch.stack([torch.stack((r.abs().sum(1), (r * r).sum(1)), -1) for r in rows], 1)
        _check(f"channel_stats V={V}", part, want, bound, 1e-5)


@pytest.mark.parametrize("groups", [1, 8])
def test_masked_groupnorm_backward_at_a_non_cubic_volume(groups):
    """vt_gn_bwd_masked and vt_gn_bwd_from_part at 6 x 10 x 14 with `low` at 3 x 5 x 7, both mask bits set, against float64 autograd of
    group_norm(cat(x, upsample(low))) on the kernel's dxn: dskip, dlow (masked by x > 0 / low > 0), dgamma, dbeta and the two absmax
    scalars, each at 1e-5 of the reference's largest entry.  Largest ratio measured on the MI355X: 1.4e-7 (dgamma, 8 groups)."""
    from vtaco_amd import ops
    B, D, H, W, C1, C2 = 2, 6, 10, 14, 32, 64
    g = torch.Generator().manual_seed(83 + groups)
    x = torch.randn(B, D, H, W, C1, generator=g).relu()
    low = torch.randn(B, D // 2, H // 2, W // 2, C2, generator=g).relu()
    dxn = torch.randn(B, D, H, W, C1 + C2, generator=g) * 1e-4
    gamma = 1 + 0.2 * torch.randn(C1 + C2, generator=g)
    x64, l64, g64 = (t.double().requires_grad_() for t in (x, low, gamma))
    b64 = torch.zeros(C1 + C2, dtype=torch.float64, requires_grad=True)
    cat = torch.cat((x64.permute(0, 4, 1, 2, 3), F.interpolate(l64.permute(0, 4, 1, 2, 3), scale_factor=2, mode="nearest")), 1)
    (F.group_norm(cat, groups, g64, b64, EPS) * dxn.double().permute(0, 4, 1, 2, 3)).sum().backward()
    want = {"dskip": x64.grad * (x > 0), "dlow": l64.grad * (low > 0), "dgamma": g64.grad, "dbeta": b64.grad}
    want["absmax_skip"], want["absmax_low"] = want["dskip"].abs().max().reshape(1), want["dlow"].abs().max().reshape(1)
    xd, ld, dd, gd = x.to(DEV), low.to(DEV), dxn.to(DEV), gamma.to(DEV)
    xs, ls = ops.channel_stats(xd), ops.channel_stats(ld)
    # the two sums vt_gn_bwd_from_part reads, laid out as the statistics pass leaves them: (sum dxn, sum dxn * x_cat) per block
    cat_cl = R.virtual_cat64(x, low)
    V, nb = D * H * W, 7
    d64 = dxn.double().reshape(B, V, -1)
    c64 = cat_cl.reshape(B, V, -1)
    rows = [(d64[:, V * k // nb:V * (k + 1) // nb], c64[:, V * k // nb:V * (k + 1) // nb]) for k in range(nb)]
    bpart = torch.stack([torch.stack((d.sum(1), (d * c).sum(1)), -1) for d, c in rows], 1).float().to(DEV).contiguous()
    worst = 0.0
    for tag, kw in (("masked", {}), ("from_part", {"bpart": (bpart, nb)})):
        got = ops.gn_bwd(xd, xs, ld, ls, dd, gd, groups, EPS, mask_skip=True, mask_low=True, **kw)
        for key, t in zip(("dskip", "dlow", "dgamma", "dbeta", "absmax_skip", "absmax_low"), got):
            ref = want[key]
            err = float((t.double().cpu() - ref).abs().max()) / float(ref.abs().max())
            worst = max(worst, _report(f"gn_bwd_{tag} g{groups} {key}", err, 1e-5))
            assert err <= 1e-5, (tag, key, err)
    assert worst > 0.0


# ---- e. the whole network at a non-cubic volume -----------------------------------------------------------------------------------------

def test_whole_network_at_a_non_cubic_volume():
    """UNet3D(f_maps=32, num_levels=3) on 1 x 16 x 32 x 64: forward_channels_last_layers at f32, bf16x3 and f16x3 and the forward of
    forward_channels_last_train against the oracle evaluated in float64, at the project's bar 1e-4 max(1, largest entry).  Measured on
    the MI355X (bar 1.8e-4): f32 8.9e-6, bf16x3 6.2e-5, f16x3 1.8e-5, training forward (f16x3) 1.3e-5."""
    from oracle import vtaco_oracle as orc
    from vtaco_amd.encoder.unet3d import UNet3D
    torch.manual_seed(16)
    net = UNet3D(in_channels=32, out_channels=32, f_maps=32, num_levels=3)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if "groupnorm" in n:
                p.add_(torch.randn(p.shape, generator=g) * 0.2)
    x = torch.randn(1, 32, 16, 32, 64, generator=g) * (torch.rand(1, 1, 16, 32, 64, generator=g) < 0.05)
    ref = orc.unet3d_forward({k: v.detach().double() for k, v in net.state_dict().items()}, x.double()).permute(0, 2, 3, 4, 1)
    bar = 1e-4 * max(1.0, float(ref.abs().max()))
    net = net.to(DEV)
    x_cl = x.to(DEV).permute(0, 2, 3, 4, 1).contiguous()
    outs = {}
    with torch.no_grad():
        for prec in ("f32", "bf16x3", "f16x3"):
            net.precision = prec
            outs[prec] = net.forward_channels_last_layers(x_cl).double().cpu()
    outs["train " + net.train_precision] = net.forward_channels_last_train(x_cl.clone().requires_grad_()).detach().double().cpu()
    for prec, out in outs.items():
        err = float((out - ref).abs().max())
        _report(f"network {prec} (absolute error)", err, bar)
        assert err <= bar, (prec, err, bar)
    assert not torch.equal(outs["f32"], outs["bf16x3"]) and not torch.equal(outs["bf16x3"], outs["f16x3"])
