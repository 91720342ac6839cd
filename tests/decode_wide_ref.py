"""A plain reference of the wide LocalDecoder (CPU, torch only): tests/decode_train_ref.py generalised to hidden_size H and c_dim C (any
widths), n_blocks nb <= 8, ``leaky`` heads, sample_mode 'nearest', the tactile concat, the contact head and features given directly --
the forward with the tensors the kernels save, and the backward written out layer by layer from those saves, in float64 (the reference),
in float32 (the yardstick e32) and over absolute values (the magnitude sums behind the rounding floor of the gate).

The module (LocalDecoder.forward / forward_img / forward_contact):

    c      = trilinear(grid, p)  or  grid[voxel(p)] with 'nearest'
    x      = fc_p([p | c_img])
    per block i:  x = x + fc_c_i(c);  a0_i = relu(x);  a1_i = relu(fc_0_i(a0_i));  x = x + fc_1_i(a1_i)
    af     = actvn(x)            relu, or leaky_relu(0.2) with ``leaky`` (the blocks' activations are ReLU whatever ``leaky`` says)
    logits = fc_out(af),  contact logits = fc_out_contact(af)

Saved tensors, in the order of the kernels' save buffer (decode_wide.hip wide_save_layout), as a list of [B,N,.] tensors:
    c [C] | a0_0, a1_0, a0_1, a1_1, ... [H] | af [H]  (af keeps the negative leaky values)

'nearest': the voxel is rint (halves to even) of the FLOAT32 grid coordinate (decode_train_cases.grid_coord32) in every precision: it
is the module's own float32 index arithmetic -- F.grid_sample(mode='nearest', padding_mode='border', align_corners=True) -- and
nothing to differentiate.  It is carried as eight "corners" at that voxel with the weights 1, 0, ..., 0, so that sample / scatter of
decode_train_ref serve both modes (adding exact zeros changes no bit)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_train_cases as cases
import decode_train_ref as ref
import decode_lattice_ref as lat
from decode_train_ref import gate_ratio                    # noqa: F401  (the gates of the callers)
from decode_lattice_ref import e_split, gate_ratio_floor   # noqa: F401

LEAKY_SLOPE = 0.2


def n_blocks(sd):
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("fc_c."))


def nearest_voxel(pts, R, padding=0.1):
    """[B,N] flattened voxel index (z slowest) of sample_mode 'nearest': rint of the float32 grid coordinate per axis."""
    f = np.rint(cases.grid_coord32(pts.detach().float().numpy(), R, padding)).astype(np.int64)
    return torch.from_numpy((f[..., 2] * R + f[..., 1]) * R + f[..., 0])


def corners(pts, R, padding=0.1, dtype=torch.float64, nearest=False):
    """(idx, w) [B,N,8] as decode_train_ref.trilinear gives them; with ``nearest`` the one voxel with weight 1 and seven zeros."""
    if not nearest:
        return ref.trilinear(pts, R, padding, dtype)
    idx = nearest_voxel(pts, R, padding).unsqueeze(-1).expand(-1, -1, 8).contiguous()
    w = torch.zeros(idx.shape, dtype=dtype)
    w[..., 0] = 1.0
    return idx, w


def _params(sd, img, dtype, absolute=False):
    def t(name):
        v = sd[name].to(dtype)
        return v.abs() if absolute else v
    nb = n_blocks(sd)
    first = "fc_p_img" if img else "fc_p"
    P = {"nb": nb, "Wp": t(first + ".weight"), "bp": t(first + ".bias"), "Wo": t("fc_out.weight"), "bo": t("fc_out.bias")}
    P["Wc"] = [t(f"fc_c.{i}.weight") for i in range(nb)]
    P["bc"] = [t(f"fc_c.{i}.bias") for i in range(nb)]
    P["W0"] = [t(f"blocks.{i}.fc_0.weight") for i in range(nb)]
    P["b0"] = [t(f"blocks.{i}.fc_0.bias") for i in range(nb)]
    P["W1"] = [t(f"blocks.{i}.fc_1.weight") for i in range(nb)]
    P["b1"] = [t(f"blocks.{i}.fc_1.bias") for i in range(nb)]
    if "fc_out_contact.weight" in sd:
        P["Wo2"], P["bo2"] = t("fc_out_contact.weight"), t("fc_out_contact.bias")
    return P


def actvn(x, leaky):
    return torch.where(x > 0, x, LEAKY_SLOPE * x) if leaky else torch.relu(x)


def _mlp(P, pf, c, c_img, contact, leaky):
    relu = torch.relu
    nb = P["nb"]
    x = pf @ P["Wp"][:, :3].t() + P["bp"]
    if c_img is not None:
        x = x + c_img @ P["Wp"][:, 3:].t()
    x = x + c @ P["Wc"][0].t() + P["bc"][0]
    saves = [c]
    for i in range(nb):
        a0 = relu(x)
        a1 = relu(a0 @ P["W0"][i].t() + P["b0"][i])
        x = x + a1 @ P["W1"][i].t() + P["b1"][i]
        if i + 1 < nb:
            x = x + c @ P["Wc"][i + 1].t() + P["bc"][i + 1]
        saves += [a0, a1]
    af = actvn(x, leaky)
    saves.append(af)
    out = (af @ P["Wo"].t() + P["bo"]).squeeze(-1)
    if contact:
        return (out, (af @ P["Wo2"].t() + P["bo2"]).squeeze(-1)), saves
    return out, saves


def forward(sd, pts, grid, c_img=None, contact=False, c=None, padding=0.1, dtype=torch.float64, leaky=False, nearest=False):
    """(logits, saves): logits [B,N] -- a pair (occupancy, contact) with ``contact`` -- and the 2 nb + 2 saved tensors.  ``c``: the
    features given directly instead of a grid (the decode_mlp form).  Nothing is detached: float64 leaves that require a gradient
    get one (tests/test_decode_wide_ref_cpu.py checks :func:`backward` that way)."""
    pf = pts.detach().float().to(dtype)
    if c is None:
        idx, w = corners(pts, grid.shape[2], padding, dtype, nearest)
        c = ref.sample(grid.to(dtype), idx, w)
    else:
        c = c.to(dtype)
    ci = c_img.to(dtype) if c_img is not None else None
    return _mlp(_params(sd, c_img is not None, dtype), pf, c, ci, contact, leaky)


def forward64(sd, pts, grid, c_img=None, contact=False, c=None, padding=0.1, leaky=False, nearest=False):
    with torch.no_grad():
        return forward(sd, pts, grid, c_img, contact, c, padding, torch.float64, leaky, nearest)


def forward32(sd, pts, grid, c_img=None, contact=False, c=None, padding=0.1, leaky=False, nearest=False):
    with torch.no_grad():
        return forward(sd, pts, grid, c_img, contact, c, padding, torch.float32, leaky, nearest)


@torch.no_grad()
def forward_bound(sd, pts, grid, c_img=None, contact=False, c=None, padding=0.1, leaky=False, nearest=False, cb=None):
    """The magnitude sums of :func:`forward64`'s results, in its layout, one per tensor as decode_train_ref.forward_bound defines them:
    sum_k |w_k grid_k| for c, sum |W| a0 + |b| for the fc_0 outputs, and for the residual stream every term added to it so far (one
    accumulator in the kernels) -- which bounds a0_i and af (a leaky negative value is 0.2 of the stream, and so is its sum).  Nothing is
    propagated through a second matrix."""
    dt = torch.float64
    img = c_img is not None
    P, A = _params(sd, img, dt), _params(sd, img, dt, absolute=True)
    nb = P["nb"]
    pf = pts.detach().float().to(dt)
    if c is None:
        idx, w = corners(pts, grid.shape[2], padding, dt, nearest)
        c, cb = ref.sample(grid.to(dt), idx, w), ref.sample(grid.to(dt).abs(), idx, w)
    else:
        c = c.to(dt)
        cb = c.abs() if cb is None else cb.to(dt)
    x = pf @ P["Wp"][:, :3].t() + P["bp"] + c @ P["Wc"][0].t() + P["bc"][0]
    bx = pf.abs() @ A["Wp"][:, :3].t() + A["bp"] + cb @ A["Wc"][0].t() + A["bc"][0]
    if img:
        ci = c_img.to(dt)
        x, bx = x + ci @ P["Wp"][:, 3:].t(), bx + ci.abs() @ A["Wp"][:, 3:].t()
    bounds = [cb]
    for i in range(nb):
        a0 = torch.relu(x)
        a1 = torch.relu(a0 @ P["W0"][i].t() + P["b0"][i])
        bounds += [bx, a0 @ A["W0"][i].t() + A["b0"][i]]
        x, bx = x + a1 @ P["W1"][i].t() + P["b1"][i], bx + a1 @ A["W1"][i].t() + A["b1"][i]
        if i + 1 < nb:
            x, bx = x + c @ P["Wc"][i + 1].t() + P["bc"][i + 1], bx + cb @ A["Wc"][i + 1].t() + A["bc"][i + 1]
    af = actvn(x, leaky).abs()
    bounds.append(torch.where(x > 0, bx, LEAKY_SLOPE * bx) if leaky else bx)
    out = (af @ A["Wo"].t() + A["bo"]).squeeze(-1)
    if contact:
        return (out, (af @ A["Wo2"].t() + A["bo2"]).squeeze(-1)), bounds
    return out, bounds


@torch.no_grad()
def forward_split64(sd, pts, grid, kind="f16", c_img=None, contact=False, c=None, padding=0.1, leaky=False, nearest=False):
    """forward64 with every dense layer in the split arithmetic of the streaming split-f16 kernel (decode_wide.hip wideh_gemm):
    W_hi x_hi + W_hi x_lo + W_lo x_hi with hi the IEEE half toward zero (cvt_pkrtz, wideh_split2) and lo the half of the rest, the parts
    held exactly and summed in float64 -- fc_p on [p | c_img] too, which that kernel also runs on the matrix core; the biases, the
    residual stream and the heads are float64.  Logits only.  A yardstick of what the operand rounding costs, not a bit model."""
    fmt = {"f16": "f16x3", "bf16": "bf16x3"}[kind]
    dt = torch.float64
    P = _params(sd, c_img is not None, dt)
    nb = P["nb"]
    pf = pts.detach().float().to(dt)
    if c is None:
        idx, w = corners(pts, grid.shape[2], padding, dt, nearest)
        c = ref.sample(grid.to(dt), idx, w)
    cs = lat.split(c.to(dt), fmt)
    xin = pf if c_img is None else torch.cat((pf, c_img.to(dt)), -1)
    x = lat.split_linear(xin, P["Wp"], fmt) + P["bp"]
    x = x + lat.split_linear(cs, P["Wc"][0], fmt) + P["bc"][0]
    for i in range(nb):
        h = lat.split_linear(torch.relu(x), P["W0"][i], fmt) + P["b0"][i]
        x = x + lat.split_linear(torch.relu(h), P["W1"][i], fmt) + P["b1"][i]
        if i + 1 < nb:
            x = x + lat.split_linear(cs, P["Wc"][i + 1], fmt) + P["bc"][i + 1]
    af = actvn(x, leaky)
    out = (af @ P["Wo"].t() + P["bo"]).squeeze(-1)
    if contact:
        return out, (af @ P["Wo2"].t() + P["bo2"]).squeeze(-1)
    return out


@torch.no_grad()
def backward(sd, pts, grid_shape, saves, grad_out, grad_out2=None, c_img=None, padding=0.1, dtype=torch.float64, absolute=False,
             leaky=False, nearest=False):
    """The backward given the saved activations ``saves`` (the list of :func:`forward`, e.g. the kernel's own save buffer through
    :func:`unpack_saves`): their values are the layer inputs of the weight gradients, their signs the masks (a > 0) and the head's
    slope (af > 0 ? 1 : 0.2 with ``leaky``, 0 without).  Returns a dict keyed like ops.decode_bwd_wide's: "grad_grid" [B,R,R,R,C]
    (None without a ``grid_shape``), "grad_c" [B,N,C], "grad_c_img" (with ``c_img``), the parameter gradients (per-block ones stacked
    [nb, ...]; "fc_p.*" is fc_p_img's with ``c_img``; "fc_out_contact.*" with ``grad_out2``) and the rows of wide_gws_layout:
    "rows.dN" [nb + 1, B, N, H] (the gradient of the residual stream in front of block i; [nb]: behind the last) and "rows.dH" [nb, B, N, H]
    (the gradient of fc_0_i's output)."""
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)
    img = c_img is not None
    P = _params(sd, img, dtype, absolute)
    nb = P["nb"]
    S = [s.detach().to(dtype) for s in saves]
    assert len(S) == 2 * nb + 2
    M = [s > 0 for s in S]
    X = [ab(s) for s in S]
    B, N = grad_out.shape
    C = S[0].shape[-1]
    go = ab(grad_out.detach().to(dtype)).unsqueeze(-1)
    flat = lambda v: v.reshape(B * N, -1)
    wg = lambda G, x: flat(G).t() @ flat(x)                       # nn.Linear layout [out][in]
    bg = lambda G: flat(G).sum(0)
    g = {k: [None] * nb for k in ("fc_c.weight", "fc_c.bias", "fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias")}
    g["fc_out.weight"], g["fc_out.bias"] = wg(go, X[-1]), bg(go)
    G = go * P["Wo"]
    if grad_out2 is not None:
        go2 = ab(grad_out2.detach().to(dtype)).unsqueeze(-1)
        g["fc_out_contact.weight"], g["fc_out_contact.bias"] = wg(go2, X[-1]), bg(go2)
        G = G + go2 * P["Wo2"]
    if leaky:
        G = G * torch.where(M[-1], torch.ones((), dtype=dtype), torch.full((), LEAKY_SLOPE, dtype=dtype))
    else:
        G = G * M[-1]                                             # d net_final
    dN, dH = [None] * (nb + 1), [None] * nb
    dN[nb] = G
    dc = torch.zeros(B, N, C, dtype=dtype)
    for i in range(nb - 1, -1, -1):                               # G = d (output of block i)
        g["fc_1.weight"][i], g["fc_1.bias"][i] = wg(G, X[2 + 2 * i]), bg(G)
        if i + 1 < nb:
            g["fc_c.weight"][i + 1], g["fc_c.bias"][i + 1] = wg(G, X[0]), bg(G)
            dc = dc + G @ P["Wc"][i + 1]
        t = (G @ P["W1"][i]) * M[2 + 2 * i]                       # d h_i
        g["fc_0.weight"][i], g["fc_0.bias"][i] = wg(t, X[1 + 2 * i]), bg(t)
        G = G + (t @ P["W0"][i]) * M[1 + 2 * i]                   # d x_i
        dH[i], dN[i] = t, G
    g["fc_c.weight"][0], g["fc_c.bias"][0] = wg(G, X[0]), bg(G)
    dc = dc + G @ P["Wc"][0]
    pin = ab(pts.detach().float().to(dtype))
    if img:
        pin = torch.cat((pin, ab(c_img.detach().to(dtype))), -1)
        g["grad_c_img"] = G @ P["Wp"][:, 3:]
    g["fc_p.weight"], g["fc_p.bias"] = wg(G, pin), bg(G)
    for k in list(g):
        if isinstance(g[k], list):
            g[k] = torch.stack(g[k])
    g["rows.dN"], g["rows.dH"] = torch.stack(dN), torch.stack(dH)
    g["grad_c"] = dc
    g["grad_grid"] = None
    if grid_shape is not None:
        idx, w = corners(pts, grid_shape[2], padding, dtype, nearest)
        g["grad_grid"] = ref.scatter(dc, idx, ab(w), grid_shape[2])
    return g


def backward64(sd, pts, grid_shape, saves, grad_out, grad_out2=None, c_img=None, padding=0.1, leaky=False, nearest=False):
    """(gradients, bounds) in float64: ``bounds`` holds, under the same keys, the same sums run over |W|, |G|, |X| and |w|."""
    args = (sd, pts, grid_shape, saves, grad_out, grad_out2, c_img, padding, torch.float64)
    return backward(*args, leaky=leaky, nearest=nearest), backward(*args, absolute=True, leaky=leaky, nearest=nearest)


def backward32(sd, pts, grid_shape, saves, grad_out, grad_out2=None, c_img=None, padding=0.1, leaky=False, nearest=False):
    return backward(sd, pts, grid_shape, saves, grad_out, grad_out2, c_img, padding, torch.float32, leaky=leaky, nearest=nearest)


def unpack_saves(save, B, N, H, C, nb):
    """The kernels' flat save buffer (wide_save_layout: c [P][C] | nb x (a0, a1) [P][H] | af [P][H]) -> the list of :func:`forward`."""
    P = B * N
    save = save.detach().cpu()
    assert save.numel() == P * C + (2 * nb + 1) * P * H
    out = [save[:P * C].view(B, N, C)]
    blk = save[P * C:P * C + 2 * nb * P * H].view(2 * nb, B, N, H)
    out += [blk[k] for k in range(2 * nb)]
    out.append(save[P * C + 2 * nb * P * H:].view(B, N, H))
    return out
