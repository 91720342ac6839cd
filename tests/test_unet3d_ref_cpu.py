"""CPU: the float64 references of tests/unet3d_ref.py against torch's own float64 layers, and the gates of tests/test_unet3d_shapes_gpu.py
against a stand-in kernel -- the same layer computed by torch in float32 on the CPU.  Honest float32 must pass every gate; a stand-in
with one subtle fault (a dropped tap, swapped axes, a shifted upsample, padding before the normalisation, statistics over the wrong
channels, an unwritten plane) must fail it.  A gate that lets a mutant through is too weak to spend GPU time on."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet3d_ref as R  # noqa: E402

EPS = 1e-5
NCDHW, CL = R.ncdhw, R.cl


def _torch_layer(x, low, w, gamma, beta, groups, dtype, relu=True):
    """relu(conv3d(group_norm(cat(x, upsample(low))))) by torch's own layers, channels-last in and out."""
    cat = NCDHW(x.to(dtype))
    if low is not None:
        cat = torch.cat((cat, F.interpolate(NCDHW(low.to(dtype)), scale_factor=2, mode="nearest")), 1)
    y = F.conv3d(F.group_norm(cat, groups, gamma.to(dtype), beta.to(dtype), EPS), w.to(dtype), padding=1)
    return CL(F.relu(y) if relu else y)


# ---- composition: the references are the layer ---------------------------------------------------------------------------------

@pytest.mark.parametrize("groups", [1, 4, 8, 32])
@pytest.mark.parametrize("shape", [(2, 6, 10, 14, 32, 64, 64), (2, 3, 5, 7, 32, 0, 32)], ids=["with-low", "plain"])
def test_references_compose_to_torchs_float64_layer(shape, groups):
    """gcr64 on gn_scale_shift64 = relu(conv3d(group_norm(cat))) and wgrad64 = its autograd weight gradient, in float64 to 1e-12 of the
    largest entry, with and without `low`, groups that do and do not straddle the concat boundary."""
    B, D, H, W, C1, C2, Cout = shape
    x, low, w, gamma, beta = R.make_layer(torch.Generator().manual_seed(3), B, D, H, W, C1, C2, Cout)
    ss = R.gn_scale_shift64(x, low, gamma, beta, groups, EPS)
    ref, bound = R.gcr64(x, low, ss, w, True)
    w64 = w.double().requires_grad_()
    want = _torch_layer(x, low, w64, gamma, beta, groups, torch.float64)
    want = want.detach()
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((bound >= ref.abs() - 1e-12).all())                        # the bound is one: |sum| <= sum |.|
    pre, _ = R.gcr64(x, low, ss, w, False)
    assert torch.equal(pre.clamp_min(0.0), ref) and float(pre.min()) < 0.0
    g = torch.randn(want.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (_torch_layer(x, low, w64, gamma, beta, groups, torch.float64, relu=False) * g).sum().backward()
    dw, dbound = R.wgrad64(x, low, ss, g)
    assert float((dw - w64.grad).abs().max()) <= 1e-12 * float(w64.grad.abs().max())
    assert bool((dbound >= dw.abs() - 1e-12).all())


def test_plan_mirror_is_the_librarys():
    """conv_plan's tile count = vt_conv3d_stat_blocks and its route the one the case table names.  The query is a host function of the
    built library: no GPU is needed, but the library must have been built (as for the other CPU tests that load it)."""
    from vtaco_amd import _lib
    lib = _lib.load()
    seen = set()
    for name, B, D, H, W, C1, C2, Cout, relu, groups, route, tile in R.F32_CASES:
        kind, what, got_tile, n = R.conv_plan(B, D, H, W, C1 + C2, Cout)
        assert (kind, what) == route and got_tile == tile, name
        assert n == lib.vt_conv3d_stat_blocks(B, D, H, W, C1 + C2, Cout), name
        assert len({D, H, W}) == 3 and (W % tile[0] or H % tile[1] or D % tile[2]), name
        seen.add(route)
    assert seen == {("ksplit", 2), ("ksplit", 4)} | {("launch", p) for p in ((1, 1), (1, 2), (1, 4), (1, 8), (2, 8), (4, 8))}


# ---- the stand-in kernel and its mutants -------------------------------------------------------------------------------------------

def _standin(x, low, ss, w, relu, mutant=None):
    """The layer as a float32 kernel would compute it, from the (scale, shift) table it is given; ``mutant`` plants one fault."""
    cat = NCDHW(x)
    if low is not None:
        up = F.interpolate(NCDHW(low), scale_factor=2, mode="nearest")
        if mutant == "upsample-shift":
            up = torch.cat((up[..., :1], up[..., :-1]), -1)                  # x >> 1 read as (x - 1) >> 1
        cat = torch.cat((cat, up), 1)
    sc, sh = ss[:, :, 0].float()[:, :, None, None, None], ss[:, :, 1].float()[:, :, None, None, None]
    w = w.clone()
    if mutant == "tap-dropped":
        w[w.shape[0] // 2, :, 0, 2, 1] = 0.0
    if mutant == "hw-swapped":
        w = w.transpose(3, 4).contiguous()
    if mutant == "pad-before-norm":
        y = F.conv3d(F.pad(cat, (1,) * 6) * sc + sh, w)
    else:
        y = F.conv3d(cat * sc + sh, w, padding=1)
    y = CL(F.relu(y) if relu else y)
    if mutant == "w-plane-unwritten":
        y[:, :, :, -1] = 0.0
    return y


def _standin_stats(x, low, gamma, beta, groups, mutant=None):
    """vt_gn_scale_shift as a float32 kernel would compute it; the mutant takes the second group's statistics one channel too far."""
    cat = R.virtual_cat64(x, low).float()
    B, C = cat.shape[0], cat.shape[-1]
    cg = C // groups
    flat = cat.reshape(B, -1, C)
    out = torch.empty(B, C, 2)
    for g in range(groups):
        lo = g * cg + (1 if mutant == "group-range" and g == min(1, groups - 1) else 0)
        sel = flat[:, :, lo:lo + cg]
        mean, var = sel.mean((1, 2)), sel.var((1, 2), unbiased=False)
        scale = (var + EPS).rsqrt()[:, None] * gamma[None, g * cg:(g + 1) * cg]
        out[:, g * cg:(g + 1) * cg, 0] = scale
        out[:, g * cg:(g + 1) * cg, 1] = beta[None, g * cg:(g + 1) * cg] - mean[:, None] * scale
    return out


@pytest.mark.parametrize("case", R.F32_CASES, ids=[c[0] for c in R.F32_CASES])
def test_honest_float32_passes_the_gates(case):
    """Every shape of the case table: torch's float32 layer passes the conv gate 1.5e-7 sqrt(K), the statistics gate 1e-5 and the per-tile partial-sum gate 1e-5; torch's float32 weight gradient passes
    2e-7 sqrt(B D H W)."""
    name, B, D, H, W, C1, C2, Cout, relu, groups, route, tile = case
    gen = torch.Generator().manual_seed(17)
    x, low, w, gamma, beta = R.make_layer(gen, B, D, H, W, C1, C2, Cout)
    ss = _standin_stats(x, low, gamma, beta, groups)
    r_scale, r_shift = R.stats_ratios(ss, R.gn_scale_shift64(x, low, gamma, beta, groups, EPS), beta)
    assert r_scale <= 1e-5 and r_shift <= 1e-5, (r_scale, r_shift)
    ref, bound = R.gcr64(x, low, ss, w, relu)
    got = _standin(x, low, ss, w, relu)
    worst = R.assert_within(got, ref, bound, R.gate_f32(C1 + C2), name)
    assert worst > 0.0
    sums, sbound = R.tile_sums64(got, tile)
    part32 = torch.stack((R.tile_reduce64(got, tile), R.tile_reduce64(got * got, tile)), -1)          # summed in float32
    assert sums.shape[1] == R.conv_plan(B, D, H, W, C1 + C2, Cout)[3]
    R.assert_within(part32, sums, sbound, 1e-5, name + " part")
    g = (torch.randn(B, D, H, W, Cout, generator=gen) * (torch.rand(B, D, H, W, 1, generator=gen) < 0.6) * 1e-6)
    dw, dbound = R.wgrad64(x, low, ss, g)
    sc, sh = ss[:, None, None, None, :, 0], ss[:, None, None, None, :, 1]
    xn32 = NCDHW(R.virtual_cat64(x, low).float() * sc + sh).contiguous()
    dw32 = torch.nn.grad.conv3d_weight(xn32, tuple(dw.shape), NCDHW(g).contiguous(), padding=1)
    R.assert_within(dw32, dw, dbound, R.gate_wgrad(B * D * H * W), name + " wgrad")


MUTANT_CASES = [c for c in R.F32_CASES if c[0] in ("tx4-ragged", "ksplit2-straddle", "tx32-ragged")]


MUTANTS = [(c, m) for c in MUTANT_CASES for m in ("tap-dropped", "hw-swapped", "upsample-shift", "pad-before-norm", "w-plane-unwritten")
           if c[6] or m != "upsample-shift"]                     # (a case without `low` has no upsample to shift)


@pytest.mark.parametrize("case,mutant", MUTANTS, ids=[f"{c[0]}-{m}" for c, m in MUTANTS])
def test_the_conv_gate_rejects_subtle_faults(case, mutant):
    name, B, D, H, W, C1, C2, Cout, relu, groups, route, tile = case
    x, low, w, gamma, beta = R.make_layer(torch.Generator().manual_seed(17), B, D, H, W, C1, C2, Cout)
    ss = _standin_stats(x, low, gamma, beta, groups)
    ref, bound = R.gcr64(x, low, ss, w, relu)
    with pytest.raises(AssertionError, match="over the gate"):
        R.assert_within(_standin(x, low, ss, w, relu, mutant), ref, bound, R.gate_f32(C1 + C2), mutant)
    # the same fault in the weight gradient's input view fails the weight-gradient gate
    if mutant in ("upsample-shift", "pad-before-norm"):
        g = torch.randn(B, D, H, W, Cout, generator=torch.Generator().manual_seed(5)) * 1e-6
        dw, dbound = R.wgrad64(x, low, ss, g)
        cat = NCDHW(x)
        if low is not None:
            up = F.interpolate(NCDHW(low), scale_factor=2, mode="nearest")
            cat = torch.cat((cat, torch.cat((up[..., :1], up[..., :-1]), -1) if mutant == "upsample-shift" else up), 1)
        sc, sh = ss[:, :, 0, None, None, None], ss[:, :, 1, None, None, None]
        if mutant == "pad-before-norm":
            xn = (F.pad(cat, (1,) * 6) * sc + sh)
            bad = torch.nn.grad.conv3d_weight(xn, tuple(dw.shape), NCDHW(g).contiguous(), padding=0)
        else:
            bad = torch.nn.grad.conv3d_weight((cat * sc + sh).contiguous(), tuple(dw.shape), NCDHW(g).contiguous(), padding=1)
        with pytest.raises(AssertionError, match="over the gate"):
            R.assert_within(bad, dw, dbound, R.gate_wgrad(B * D * H * W), mutant + " wgrad")


@pytest.mark.parametrize("groups", [4, 8, 32])
def test_the_statistics_gate_rejects_a_wrong_channel_range(groups):
    """One group's statistics taken one channel off: caught by the statistics gate (the conv gate is fed the kernel's own table and
    holds the convolution alone), and by the composed layer against torch's float64 GroupNorm."""
    name, B, D, H, W, C1, C2, Cout, relu, _, route, tile = MUTANT_CASES[1]
    x, low, w, gamma, beta = R.make_layer(torch.Generator().manual_seed(17), B, D, H, W, C1, C2, Cout)
    ref_ss = R.gn_scale_shift64(x, low, gamma, beta, groups, EPS)
    good = R.stats_ratios(_standin_stats(x, low, gamma, beta, groups), ref_ss, beta)
    bad_ss = _standin_stats(x, low, gamma, beta, groups, mutant="group-range")
    bad = R.stats_ratios(bad_ss, ref_ss, beta)
    assert max(good) <= 1e-5 < max(bad), (good, bad)
    ref, bound = R.gcr64(x, low, ref_ss, w, relu)
    with pytest.raises(AssertionError, match="over the gate"):
        R.assert_within(_standin(x, low, bad_ss, w, relu), ref, bound, R.gate_f32(C1 + C2), "group-range")


def test_the_partial_sum_gate_rejects_a_tile_that_misses_its_ragged_tail():
    """out_part per block: a block sum that counts the voxels past the volume's edge (or drops the ragged tail) fails 1e-5."""
    name, B, D, H, W, C1, C2, Cout, relu, groups, route, tile = MUTANT_CASES[0]
    y = torch.randn(B, D, H, W, Cout, generator=torch.Generator().manual_seed(2), dtype=torch.float64).relu()
    sums, sbound = R.tile_sums64(y, tile)
    assert float((sums[..., 0].sum(1) - y.sum((1, 2, 3))).abs().max()) <= 1e-9           # the tiles partition the volume
    bad = y.clone()
    bad[:, :, :, -1] = 0.0
    with pytest.raises(AssertionError, match="over the gate"):
        R.assert_within(R.tile_sums64(bad, tile)[0].float(), sums, sbound, 1e-5, "tail dropped")


def test_flagged_deal_mirror():
    """flagged_deal: without flags it is the dense walk (tile t to workgroup t % wgs); with flags the tiles that keep their taps fill the
    workgroups from the front in tile order, the flagged ones from the back, and a depth-4 tile reads the flag of the 8^3 block it lies in."""
    D, H, W, tz, wgs = 16, 16, 24, 4, 5
    nblk, ntile = (D // 8) * (H // 8) * (W // 8), (D // tz) * (H // 8) * (W // 8)
    none = R.flagged_deal(torch.zeros(2, nblk, dtype=torch.uint8), D, H, W, tz, wgs)
    assert torch.equal(none, (torch.arange(ntile) % wgs).expand(2, -1))
    flags = torch.zeros(1, nblk, dtype=torch.uint8)
    flags[0, 1], flags[0, 6 + 2] = 1, 3                                  # block (0, 0, 1) and block (1, 0, 2)
    own = R.flagged_deal(flags, D, H, W, tz, wgs)[0]
    flagged = [1, 7, 12 + 2, 18 + 2]                                     # z tiles 0, 1 of the first block, z tiles 2, 3 of the second
    assert own[flagged].tolist() == [4, 3, 2, 1]
    rest = [t for t in range(ntile) if t not in flagged]
    assert own[rest].tolist() == [r % wgs for r in range(len(rest))]
