"""A plain reference of the decoder on plane features (CPU, torch only): ``sample_plane_feature`` (reference decoder.py:55-60) as the
explicit four-pixel formula, the sum ``grid, xz, xy, yz`` in the reference's order whatever order the dict has (:137-146), and the
conditioned MLP, on top of the oracle's ``normalize_coordinate``, ``_sample`` and ``decoder_mlp`` -- in float64 (the reference), in
float32 (the yardstick e32 of the gate) and over absolute values (the magnitude sums behind the gate's rounding floor).

The gate is tests/decode_train_ref.py's: |got - ref64| <= 8 max(e32, 2^-24 bound), elementwise (``gate_ratio``).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import vtaco_oracle as orc  # noqa: E402
from decode_train_ref import gate_ratio  # noqa: E402,F401

ORDER = ("xz", "xy", "yz")


def corners(pts, R, plane, padding=0.1, mode="bilinear", dtype=torch.float64):
    """Pixel indices [B,N,4] into a flattened R x R plane (row = the second projected axis, column = the first) and their weights
    [B,N,4] in ``dtype``.  Pixel k: bit 0 = column + 1, bit 1 = row + 1; 'nearest': pixel 0 alone, rounded half to even."""
    q = orc.normalize_coordinate(pts.detach().float().to(dtype), padding, plane)
    f = ((((2 * q - 1) + 1) / 2) * (R - 1)).clamp(0, R - 1)
    if mode == "nearest":
        i = torch.round(f).long()
        idx = (i[..., 1] * R + i[..., 0]).unsqueeze(-1).expand(-1, -1, 4)
        w = torch.zeros(*idx.shape, dtype=dtype)
        w[..., 0] = 1
        return idx, w
    f0 = f.floor()
    i0 = f0.long()
    i1 = (i0 + 1).clamp(max=R - 1)
    w0 = (f0 + 1) - f
    w1 = torch.where(i0 + 1 <= R - 1, f - f0, torch.zeros_like(f))
    idx, w = [], []
    for k in range(4):
        sx, sy = k & 1, (k >> 1) & 1
        idx.append((i1 if sy else i0)[..., 1] * R + (i1 if sx else i0)[..., 0])
        w.append((w1 if sx else w0)[..., 0] * (w1 if sy else w0)[..., 1])
    return torch.stack(idx, -1), torch.stack(w, -1)


def sample_plane(plane, idx, w):
    """sum_k w_k plane[pixel_k]: plane [B,C,R,R] -> [B,N,C] in the dtype of ``w`` (differentiable in ``plane``)."""
    B, C = plane.shape[:2]
    cl = plane.reshape(B, C, -1).permute(0, 2, 1).to(w.dtype)
    out = 0
    for k in range(4):
        out = out + w[..., k:k + 1] * torch.gather(cl, 1, idx[..., k:k + 1].expand(-1, -1, C))
    return out


def features(c_plane, pts, padding=0.1, mode="bilinear", dtype=torch.float64, base=None, absolute=False):
    """c [B,N,C] = base? + grid? + xz? + xy? + yz? in that order; ``absolute``: the same sums over magnitudes."""
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)
    c = 0 if base is None else ab(base.to(dtype))
    if "grid" in c_plane:
        g = c_plane["grid"].to(dtype)
        if absolute:
            g = g.abs()
        c = c + orc._sample(g, pts.detach().float().to(dtype), padding, mode).to(dtype)
    for k in ORDER:
        if k in c_plane:
            idx, w = corners(pts, c_plane[k].shape[-1], k, padding, mode, dtype)
            c = c + sample_plane(ab(c_plane[k].to(dtype)), idx, ab(w))
    return c


def scatter(grad_feat, pts, R, plane, padding=0.1, mode="bilinear", dtype=torch.float64, absolute=False):
    """The transpose of sample_plane: grad_feat [B,N,C] -> grad plane [B,C,R,R]."""
    idx, w = corners(pts, R, plane, padding, mode, dtype)
    g = grad_feat.detach().to(dtype)
    if absolute:
        g, w = g.abs(), w.abs()
    B, N, C = g.shape
    out = torch.zeros(B, R * R, C, dtype=dtype)
    for k in range(4):
        out.scatter_add_(1, idx[..., k:k + 1].expand(-1, -1, C), w[..., k:k + 1] * g)
    return out.permute(0, 2, 1).reshape(B, C, R, R)


def forward(sd, pts, c_plane, padding=0.1, leaky=False, mode="bilinear", dtype=torch.float64, c=None):
    """LocalDecoder.forward's logits [B,N] (decoder.py:135-161) in ``dtype``; ``c``: features given instead of sampled."""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    if c is None:
        c = features(c_plane, pts, padding, mode, dtype)
    net = orc.decoder_mlp(sdd, orc._lin(sdd, "fc_p", pts.detach().float().to(dtype)), c.to(dtype))
    return orc._lin(sdd, "fc_out", orc._head_actvn(net, leaky)).squeeze(-1)


def grads(sd, pts, c_plane, padding=0.1, leaky=False, mode="bilinear", dtype=torch.float64):
    """(logits, {feature key: d sum(logits) / d feature}, {parameter name: gradient}) under autograd in ``dtype``."""
    feats = {k: v.detach().to(dtype).requires_grad_(True) for k, v in c_plane.items()}
    prm = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if not k.startswith("fc_p_img")}
    logits = forward(prm, pts, feats, padding, leaky, mode, dtype)
    logits.sum().backward()
    return logits.detach(), {k: v.grad for k, v in feats.items()}, {k: v.grad for k, v in prm.items() if v.grad is not None}


def _nb(sd):
    return orc._n_blocks(sd)


def mlp_saves(sd, pts, c, leaky=False, dtype=torch.float64):
    """(rx, rh, af) of the conditioned MLP on features ``c``: per block the inputs of fc_0 (relu(net + fc_c_i(c))) and of fc_1
    (relu(fc_0(.))), stacked [nb,B,N,H], and the head's input actvn(net_final) [B,N,H] -- what the training forwards keep."""
    P = {k: v.detach().to(dtype) for k, v in sd.items()}
    c = c.detach().to(dtype)
    net = orc._lin(P, "fc_p", pts.detach().float().to(dtype))
    rxs, rhs = [], []
    for i in range(_nb(P)):
        net = net + orc._lin(P, f"fc_c.{i}", c)
        rx = torch.relu(net)
        rh = torch.relu(orc._lin(P, f"blocks.{i}.fc_0", rx))
        net = net + orc._lin(P, f"blocks.{i}.fc_1", rh)
        rxs.append(rx)
        rhs.append(rh)
    return torch.stack(rxs), torch.stack(rhs), orc._head_actvn(net, leaky)


def mlp_backward(sd, pts, c, rx, rh, af, grad_out, leaky=False, dtype=torch.float64, absolute=False):
    """The MLP's backward written out layer by layer from the saved layer inputs (their values are the X operands of the weight
    gradients, their signs the activation masks -- tests/decode_train_ref.py's treatment of ReLU flips, at any hidden size and with
    the `leaky` head): {"grad_c": [B,N,C], state-dict name: gradient}.  ``absolute``: the same sums over |W|, |G|, |X|."""
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)
    P = {k: ab(v.detach().to(dtype)) for k, v in sd.items()}
    nb = _nb(P)
    rx, rh, af = rx.detach().to(dtype), rh.detach().to(dtype), af.detach().to(dtype)
    c = c.detach().to(dtype)
    B, N = grad_out.shape
    flat = lambda v: v.reshape(B * N, -1)
    wg = lambda G, x: flat(G).t() @ flat(ab(x))
    bg = lambda G: flat(G).sum(0)
    go = ab(grad_out.detach().to(dtype)).unsqueeze(-1)
    g = {"fc_out.weight": wg(go, af), "fc_out.bias": bg(go)}
    slope = torch.where(af > 0, torch.ones_like(af), torch.full_like(af, 0.2 if leaky else 0.0))
    G = (go * P["fc_out.weight"]) * slope                          # d net_final
    dc = torch.zeros(B, N, c.shape[-1], dtype=dtype)
    for i in range(nb - 1, -1, -1):
        g[f"blocks.{i}.fc_1.weight"], g[f"blocks.{i}.fc_1.bias"] = wg(G, rh[i]), bg(G)
        t = (G @ P[f"blocks.{i}.fc_1.weight"]) * (rh[i] > 0)        # d fc_0's output
        g[f"blocks.{i}.fc_0.weight"], g[f"blocks.{i}.fc_0.bias"] = wg(t, rx[i]), bg(t)
        G = G + (t @ P[f"blocks.{i}.fc_0.weight"]) * (rx[i] > 0)    # d (net + fc_c_i(c)), which is d net in front of the block too
        g[f"fc_c.{i}.weight"], g[f"fc_c.{i}.bias"] = wg(G, c), bg(G)
        dc = dc + G @ P[f"fc_c.{i}.weight"]
    g["fc_p.weight"], g["fc_p.bias"] = wg(G, pts.detach().float().to(dtype)), bg(G)
    g["grad_c"] = dc
    return g


def feature_grads(c_plane, pts, dc, padding=0.1, mode="bilinear", dtype=torch.float64, absolute=False):
    """d features from d c [B,N,C]: the transpose of every sampler of ``c_plane`` ('grid': [B,C,R,R,R])."""
    out = {}
    for k, v in c_plane.items():
        if k == "grid":
            # the transpose of the oracle's own sampler (its corner weights are >= 0: over magnitudes it is the same map on |d c|)
            z = torch.zeros(v.shape, dtype=dtype, requires_grad=True)
            cot = dc.detach().to(dtype)
            orc._sample(z, pts.detach().float().to(dtype), padding, mode).backward(cot.abs() if absolute else cot)
            out[k] = z.grad
        else:
            out[k] = scatter(dc, pts, v.shape[-1], k, padding, mode, dtype, absolute)
    return out
