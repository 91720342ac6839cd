"""Float64 references of the UNet3D layer family (csrc/unet3d.hip) and the elementwise comparator the GPU tests gate with.

Everything here is CPU torch in float64 on channels-last tensors [B, D, H, W, C], the kernels' layout.  A layer reads the virtual concat
cat(x, nearest_upsample2(low)) (``low`` [B, D/2, H/2, W/2, C2] or None), normalises it per channel with a [B, C, 2] (scale, shift) table,
pads with zeros AFTER the normalisation and convolves with a [Cout, Cin, 3, 3, 3] weight.  Every reference comes with the bound its
error is measured against: the same sum with every term replaced by its absolute value, so the gate |got - ref| <= tol * bound is a
relative error per output element, blind to nothing (a max-norm gate scaled by the largest entry does not see a wrong border voxel)."""
import torch
import torch.nn.functional as F

TINY = 1e-30


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def virtual_cat64(x, low):
    """cat(x, nearest_upsample2(low)) in float64, channels-last."""
    x = x.detach().double().cpu()
    if low is None:
        return x
    up = low.detach().double().cpu().repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert up.shape[:4] == x.shape[:4], (tuple(up.shape), tuple(x.shape))
    return torch.cat((x, up), -1)


def gn_scale_shift64(x, low, gamma, beta, groups, eps):
    """GroupNorm's (scale, shift) per scene and channel over the virtual concat: [B, C1 + C2, 2] with xn = x * scale + shift.  Every value
    of ``low`` counts 8 times (its eight upsampled copies); a group may straddle the x / low boundary."""
    x = x.detach().double().cpu()
    B, V, C1 = x.shape[0], x.shape[1] * x.shape[2] * x.shape[3], x.shape[4]
    s1, s2 = x.reshape(B, V, C1).sum(1), (x * x).reshape(B, V, C1).sum(1)
    if low is not None:
        lo = low.detach().double().cpu()
        assert 8 * lo.shape[1] * lo.shape[2] * lo.shape[3] == V
        lo = lo.reshape(B, -1, lo.shape[-1])
        s1, s2 = torch.cat((s1, 8 * lo.sum(1)), 1), torch.cat((s2, 8 * (lo * lo).sum(1)), 1)
    C = s1.shape[1]
    assert C % groups == 0
    n = V * (C // groups)
    mean = s1.reshape(B, groups, -1).sum(2) / n
    var = s2.reshape(B, groups, -1).sum(2) / n - mean * mean                       # biased, as torch.nn.GroupNorm
    rstd = (var + eps).rsqrt()
    rep = lambda t: t.repeat_interleave(C // groups, 1)
    scale = rep(rstd) * gamma.detach().double().cpu()[None]
    shift = beta.detach().double().cpu()[None] - rep(mean) * scale
    return torch.stack((scale, shift), -1)


def _normalised(x, low, scale_shift):
    cat = virtual_cat64(x, low)
    if scale_shift is None:
        return cat, cat.abs()
    ss = scale_shift.detach().double().cpu()
    sc, sh = ss[:, None, None, None, :, 0], ss[:, None, None, None, :, 1]
    return cat * sc + sh, cat.abs() * sc.abs() + sh.abs()


def gcr64(x, low, scale_shift, w, relu):
    """(ref, bound) of relu?(conv3d(xn, w, padding=1)) with xn = cat * scale + shift, zero padding after the normalisation;
    bound = conv3d(|cat| |scale| + |shift|, |w|, padding=1).  ``scale_shift`` is taken as given (the GPU tests hand over the kernel's own
    table, so that the gate holds the convolution's arithmetic alone); None: no normalisation.  Channels-last in and out."""
    xn, xa = _normalised(x, low, scale_shift)
    w = w.detach().double().cpu()
    ref = F.conv3d(ncdhw(xn), w, padding=1)
    if relu:
        ref = ref.clamp_min(0.0)                                                     # 1-Lipschitz: the bound of the pre-activation holds
    return cl(ref), cl(F.conv3d(ncdhw(xa), w.abs(), padding=1))


def wgrad64(x, low, scale_shift, g):
    """(dW, bound) [Cout, Cin, 3, 3, 3] of the same conv: dW[co, ci, tap] = sum_v g[v, co] xn[v + tap, ci] (zero outside the volume),
    the bound from |g| and |cat| |scale| + |shift|."""
    xn, xa = _normalised(x, low, scale_shift)
    g = g.detach().double().cpu()
    shape = (g.shape[-1], xn.shape[-1], 3, 3, 3)
    dw = torch.nn.grad.conv3d_weight(ncdhw(xn).contiguous(), shape, ncdhw(g).contiguous(), padding=1)
    bound = torch.nn.grad.conv3d_weight(ncdhw(xa).contiguous(), shape, ncdhw(g.abs()).contiguous(), padding=1)
    return dw, bound


def ratio(got, ref, bound):
    """max |got - ref| / max(bound, tiny) (inf where ``got`` is not finite)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == bound.shape, (tuple(got.shape), tuple(ref.shape), tuple(bound.shape))
    r = (got - ref).abs() / bound.clamp_min(TINY)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max())


def assert_within(got, ref, bound, tol, tag=""):
    """Elementwise |got - ref| <= tol * max(bound, tiny); returns the largest ratio of the error to the bound."""
    worst = ratio(got, ref, bound)
    if not worst <= tol:
        got = got.detach().double().cpu()
        r = (got - ref).abs() / bound.clamp_min(TINY)
        r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
        at = tuple(int(i) for i in torch.unravel_index(r.argmax(), r.shape))
        raise AssertionError(f"{tag}: ratio {worst:.3e} > gate {tol:.3e} at {at}: got {float(got[at])!r}, ref {float(ref[at])!r}, "
                             f"bound {float(bound[at])!r}; {int((r > tol).sum())} of {r.numel()} entries over the gate")
    return worst


# ---- the gates (see the tests' module docstrings for where the constants come from) -------------------------------------------------

def gate_f32(cin):
    """Exact-f32, split-f16 and IEEE-half-pair kernels: two f32-accumulating kernels differ by 1.5e-7 sqrt(K), K = 27 Cin."""
    return 1.5e-7 * (27 * cin) ** 0.5


def gate_bf16x3(cin):
    """Split-bf16 kernels: 2^-16 per product (the dropped lo x lo term) on top of the f32 accumulation."""
    return 2.0 ** -16 + gate_f32(cin)


def gate_wgrad(nvox):
    """Weight gradients: K = B D H W products per entry."""
    return 2e-7 * nvox ** 0.5


def make_layer(gen, B, D, H, W, C1, C2, Cout, keep=0.3, x_scale=1.0):
    """The project's test inputs for one layer, drawn on the CPU: randn activations under a sparsity mask, w ~ 0.05 randn,
    gamma = 1 + 0.2 randn, beta = 0.2 randn.  Returns (x, low or None, w, gamma, beta), float32, channels-last."""
    x = torch.randn(B, D, H, W, C1, generator=gen) * (torch.rand(B, D, H, W, 1, generator=gen) < keep) * x_scale
    low = torch.randn(B, D // 2, H // 2, W // 2, C2, generator=gen) * x_scale if C2 else None
    w = torch.randn(Cout, C1 + C2, 3, 3, 3, generator=gen) * 0.05
    gamma = 1 + 0.2 * torch.randn(C1 + C2, generator=gen)
    beta = 0.2 * torch.randn(C1 + C2, generator=gen)
    return x, low, w, gamma, beta


# ---- the host-side plans of csrc/unet3d.hip, mirrored (the tests assert the mirror against the library's own queries) ---------------

def conv_tile(D, H, W, waves):
    """conv_tile: the exact-f32 kernel's block tile (TX, TY, TZ) of 32 * waves voxels and the number of (ragged) tiles per scene."""
    TX = 32 if W >= 32 else 16 if W >= 16 else 8 if W >= 8 else 4
    rows = waves * (32 // TX)
    TY = min(rows, H)
    while rows % TY:
        TY -= 1
    TZ = rows // TY
    return (TX, TY, TZ), -(-W // TX) * -(-H // TY) * -(-D // TZ)


def conv_plan(B, D, H, W, Cin, Cout):
    """vt_conv3d_gcr's route: ("ksplit", width, tile, tiles) -- conv_use_ksplit, widths 2 and 4 -- or ("launch", (NCO, WAVES), tile, tiles)
    -- conv_waves and the cout blocks per workgroup -- with tiles = vt_conv3d_stat_blocks."""
    nco, ncib = Cout // 32, Cin // 32
    tile, n1 = conv_tile(D, H, W, 1)
    if ncib >= 2 and n1 * B * nco < 1024:
        return "ksplit", (4 if ncib >= 4 else 2), tile, n1
    waves = next((wv for wv in (8, 4, 2) if conv_tile(D, H, W, wv)[1] * B * nco >= 512), 1)
    tile, n = conv_tile(D, H, W, waves)
    per = 1
    if waves == 8:
        per = nco
        while per > 1 and (per > 4 or n * B * (nco // per) < 512 or nco % per):
            per >>= 1
    return "launch", (per, waves), tile, n


def tile_reduce64(t, tile):
    """Sums of a channels-last float64 tensor over ragged (TX, TY, TZ) tiles in the kernels' block order (x fastest, then y, then z):
    [B, tiles, C]."""
    TX, TY, TZ = tile
    B, D, H, W, C = t.shape
    pad = F.pad(t, (0, 0, 0, -W % TX, 0, -H % TY, 0, -D % TZ))
    t = pad.reshape(B, pad.shape[1] // TZ, TZ, pad.shape[2] // TY, TY, pad.shape[3] // TX, TX, C).permute(0, 1, 3, 5, 2, 4, 6, 7)
    return t.reshape(B, -1, TZ * TY * TX, C).sum(2)


def tile_sums64(y, tile, wgs=0, owner=None):
    """What a conv kernel's out_part holds, from its own output: (sum y, sum y^2) per block, and the bound (sum |y|, sum y^2) the gate
    scales by -- two tensors [B, blocks, C, 2].  A block is a tile, or with ``wgs`` the tiles of persistent workgroup wg (the split-f16
    kernels): wg, wg + wgs, ... or, with ``owner`` [B, tiles], the tiles whose entry is wg (flagged_deal)."""
    y = y.detach().double().cpu()
    sq = tile_reduce64(y * y, tile)
    sums, bound = torch.stack((tile_reduce64(y, tile), sq), -1), torch.stack((tile_reduce64(y.abs(), tile), sq), -1)
    if wgs:
        if owner is None:
            owner = (torch.arange(sums.shape[1]) % wgs).expand(sums.shape[0], -1)
        fold = lambda t: torch.stack([torch.zeros(wgs, *t.shape[2:], dtype=t.dtype).index_add_(0, owner[b], t[b]) for b in range(t.shape[0])])
        sums, bound = fold(sums), fold(bound)
    return sums, bound


def flagged_deal(flags, D, H, W, tz, wgs):
    """The tile walk of vt_conv3d_gcr_f16x3_skip (conv3d_gcr_hw_kernel's prologue): per scene, the 8 x 8 x tz tiles that need their taps
    go in tile order to workgroups 0, 1, ... (rank % wgs), the tiles of flagged 8^3 blocks -- flag byte at block ((z tile * tz) >> 3, y
    tile, x tile) non-zero -- in tile order to workgroups wgs - 1, wgs - 2, ... (wgs - 1 - rank % wgs).  ``flags`` [B, (D/8)(H/8)(W/8)]
    uint8; returns the owning workgroup of every tile, [B, tiles]."""
    tx, ty = W // 8, H // 8
    t = torch.arange((D // tz) * ty * tx)
    blk = (((t // (tx * ty)) * tz) >> 3) * ty * tx + ((t // tx) % ty) * tx + t % tx
    skip = flags.cpu()[:, blk] != 0
    rank_ne, rank_e = (~skip).long().cumsum(1) - 1, skip.long().cumsum(1) - 1
    return torch.where(skip, wgs - 1 - rank_e % wgs, rank_ne % wgs)


def stats_ratios(ss, ref, beta):
    """The statistics gate's two ratios for a (scale, shift) table [B, C, 2] against gn_scale_shift64's: |scale - ref| / |ref| and
    |shift - ref| / (|beta| + |mean * scale|), with mean * scale = beta - shift of the reference.  Both are gated at 1e-5."""
    ss, beta = ss.detach().double().cpu(), beta.detach().double().cpu()
    r_scale = float(((ss[..., 0] - ref[..., 0]).abs() / ref[..., 0].abs()).max())
    r_shift = float(((ss[..., 1] - ref[..., 1]).abs() / (beta.abs()[None] + (beta[None] - ref[..., 1]).abs()).clamp_min(TINY)).max())
    return r_scale, r_shift


# ---- the exact-f32 case table: the smallest volumes with three different sides that reach each route of vt_conv3d_gcr ---------------
# (id, B, D, H, W, C1, C2, Cout, relu, groups, route, tile): every volume has a side that is no multiple of its tile.  The batch is two
# wherever the route admits one.
F32_CASES = [
    ("tx4-ragged", 2, 3, 5, 7, 32, 0, 32, True, 8, ("launch", (1, 1)), (4, 4, 2)),
    ("tx4-norelu", 2, 3, 5, 7, 32, 0, 32, False, 8, ("launch", (1, 1)), (4, 4, 2)),
    ("tx4-groups1", 2, 3, 5, 7, 32, 0, 32, True, 1, ("launch", (1, 1)), (4, 4, 2)),
    ("tx4-groups4", 2, 3, 5, 7, 32, 0, 32, True, 4, ("launch", (1, 1)), (4, 4, 2)),
    ("tx4-groups32", 2, 3, 5, 7, 32, 0, 32, True, 32, ("launch", (1, 1)), (4, 4, 2)),
    ("ksplit2-straddle", 2, 6, 10, 14, 32, 64, 64, True, 8, ("ksplit", 2), (8, 4, 1)),      # groups of 12 channels: one straddles x | low
    ("ksplit4", 2, 6, 10, 14, 64, 64, 32, True, 8, ("ksplit", 4), (8, 4, 1)),
    ("tx32-ragged", 2, 20, 12, 40, 32, 0, 32, True, 8, ("launch", (1, 1)), (32, 1, 1)),
    ("launch-1-2", 2, 68, 5, 18, 32, 0, 32, True, 8, ("launch", (1, 2)), (16, 4, 1)),
    ("launch-1-4", 2, 68, 9, 18, 32, 0, 32, True, 8, ("launch", (1, 4)), (16, 8, 1)),
    ("launch-1-8", 2, 68, 9, 34, 32, 0, 32, True, 8, ("launch", (1, 8)), (32, 8, 1)),
    ("launch-2-8", 2, 68, 9, 34, 32, 0, 64, True, 8, ("launch", (2, 8)), (32, 8, 1)),
    ("launch-4-8", 2, 68, 9, 34, 32, 0, 128, True, 8, ("launch", (4, 8)), (32, 8, 1)),
]
