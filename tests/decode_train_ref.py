"""A plain reference of the 32/32 LocalDecoder's training path (CPU, torch only): the forward with the twelve tensors the kernel
saves, and the backward written out layer by layer -- in float64 (the reference), in float32 (the yardstick e32) and over absolute
values (the magnitude sums behind the rounding floor of the gate).

The module (LocalDecoder.forward / forward_img / forward_contact, 5 blocks, hidden = c_dim = 32):

    c      = trilinear(grid, p)                       align-corners, border; p normalised by divisor = float32(1 + padding + 10e-4),
                                                      q = p / divisor + 0.5, q >= 1 -> 0.999, q < 0 -> 0, f = q (R - 1)
    x_0    = fc_p([p | c_img]) + fc_c_0(c)
    h_i    = fc_0_i(relu(x_i))
    x_i+1  = x_i + fc_1_i(relu(h_i)) + fc_c_i+1(c)    (no fc_c term after the last block: x_5 = net_5)
    logits = fc_out(relu(net_5)),  contact logits = fc_out_contact(relu(net_5))

Saved tensors, in the order of the kernel's save buffer [12][B*N][32]:
    slot 0 c | slots 1..5 relu(x_i) | slots 6..10 relu(h_i) | slot 11 relu(net_5)

The point coordinates are float32 values; the normalisation and the trilinear weights are evaluated in the working precision from
them.  The constants 0.999 and the divisor are the module's float32 constants in every precision.
"""
import numpy as np
import torch

NB = 5
Q_HI = float(np.float32(0.999))


def divisor(padding=0.1):
    return float(np.float32(1.0 + padding + 10e-4))


def trilinear(pts, R, padding=0.1, dtype=torch.float64):
    """Corner indices [B,N,8] into a flattened R^3 volume (z slowest, x fastest) and their weights [B,N,8] in ``dtype``.
    Corner k: bit 0 = x + 1, bit 1 = y + 1, bit 2 = z + 1.  A +1 corner past the border is clamped to R - 1 with weight 0."""
    p = pts.detach().float().to(dtype)
    q = p / divisor(padding) + 0.5
    q = torch.where(q >= 1, torch.full_like(q, Q_HI), q)
    q = torch.where(q < 0, torch.zeros_like(q), q)
    f = ((((2 * q - 1) + 1) / 2) * (R - 1)).clamp(0, R - 1)
    f0 = f.floor()
    i0 = f0.long()
    i1 = (i0 + 1).clamp(max=R - 1)
    w0 = (f0 + 1) - f
    w1 = torch.where(i0 + 1 <= R - 1, f - f0, torch.zeros_like(f))
    idx, w = [], []
    for k in range(8):
        sx, sy, sz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        xi, yi, zi = (i1 if sx else i0)[..., 0], (i1 if sy else i0)[..., 1], (i1 if sz else i0)[..., 2]
        idx.append((zi * R + yi) * R + xi)
        w.append(((w1 if sx else w0)[..., 0] * (w1 if sy else w0)[..., 1]) * (w1 if sz else w0)[..., 2])
    return torch.stack(idx, -1), torch.stack(w, -1)


def sample(grid, idx, w):
    """sum_k w_k grid[corner_k]: grid [B,C,R,R,R] -> [B,N,C] in the dtype of ``w``."""
    B, C = grid.shape[:2]
    gcl = grid.permute(0, 2, 3, 4, 1).reshape(B, -1, C).to(w.dtype)
    out = torch.zeros(B, idx.shape[1], C, dtype=w.dtype)
    for k in range(8):
        out = out + w[..., k:k + 1] * torch.gather(gcl, 1, idx[..., k:k + 1].expand(-1, -1, C))
    return out


def scatter(dc, idx, w, R):
    """The transpose of :func:`sample`: d c [B,N,C] -> d grid [B,R,R,R,C]."""
    B, N, C = dc.shape
    out = torch.zeros(B, R ** 3, C, dtype=dc.dtype)
    for k in range(8):
        out.scatter_add_(1, idx[..., k:k + 1].expand(-1, -1, C), w[..., k:k + 1] * dc)
    return out.view(B, R, R, R, C)


def scatter64(pts, grad_feat, R, padding=0.1, dtype=torch.float64):
    """Backward of the trilinear sampling alone, any channel count: (d grid [B,R,R,R,C], its magnitude sum)."""
    idx, w = trilinear(pts, R, padding, dtype)
    g = grad_feat.detach().to(dtype)
    return scatter(g, idx, w, R), scatter(g.abs(), idx, w.abs(), R)


def _params(sd, img, dtype, absolute=False):
    def t(name):
        v = sd[name].detach().to(dtype)
        return v.abs() if absolute else v
    first = "fc_p_img" if img else "fc_p"
    P = {"Wp": t(first + ".weight"), "bp": t(first + ".bias"), "Wo": t("fc_out.weight"), "bo": t("fc_out.bias")}
    P["Wc"] = [t(f"fc_c.{i}.weight") for i in range(NB)]
    P["bc"] = [t(f"fc_c.{i}.bias") for i in range(NB)]
    P["W0"] = [t(f"blocks.{i}.fc_0.weight") for i in range(NB)]
    P["b0"] = [t(f"blocks.{i}.fc_0.bias") for i in range(NB)]
    P["W1"] = [t(f"blocks.{i}.fc_1.weight") for i in range(NB)]
    P["b1"] = [t(f"blocks.{i}.fc_1.bias") for i in range(NB)]
    if "fc_out_contact.weight" in sd:
        P["Wo2"], P["bo2"] = t("fc_out_contact.weight"), t("fc_out_contact.bias")
    return P


def _mlp(P, pf, c, c_img, contact):
    relu = torch.relu
    x = pf @ P["Wp"][:, :3].t() + P["bp"]
    if c_img is not None:
        x = x + c_img @ P["Wp"][:, 3:].t()
    x = x + c @ P["Wc"][0].t() + P["bc"][0]
    rxs, rhs = [], []
    for i in range(NB):
        rx = relu(x)
        rh = relu(rx @ P["W0"][i].t() + P["b0"][i])
        x = x + rh @ P["W1"][i].t() + P["b1"][i]
        if i + 1 < NB:
            x = x + c @ P["Wc"][i + 1].t() + P["bc"][i + 1]
        rxs.append(rx)
        rhs.append(rh)
    a = relu(x)
    out = (a @ P["Wo"].t() + P["bo"]).squeeze(-1)
    saves = [c] + rxs + rhs + [a]
    if contact:
        return (out, (a @ P["Wo2"].t() + P["bo2"]).squeeze(-1)), saves
    return out, saves


def forward(sd, pts, grid, c_img=None, contact=False, c=None, padding=0.1, dtype=torch.float64):
    """(logits, saves): logits [B,N] -- a pair (occupancy, contact) with ``contact`` -- and the twelve saved tensors [B,N,32].
    ``c``: the features given directly instead of a grid (the decode_mlp form)."""
    pf = pts.detach().float().to(dtype)
    if c is None:
        idx, w = trilinear(pts, grid.shape[2], padding, dtype)
        c = sample(grid.detach().to(dtype), idx, w)
    else:
        c = c.detach().to(dtype)
    ci = c_img.detach().to(dtype) if c_img is not None else None
    return _mlp(_params(sd, c_img is not None, dtype), pf, c, ci, contact)


def forward64(sd, pts, grid, c_img=None, contact=False, c=None, padding=0.1):
    return forward(sd, pts, grid, c_img, contact, c, padding, torch.float64)


def forward32(sd, pts, grid, c_img=None, contact=False, c=None, padding=0.1):
    return forward(sd, pts, grid, c_img, contact, c, padding, torch.float32)


def forward_bound(sd, pts, grid, c_img=None, contact=False, c=None, padding=0.1, cb=None):
    """The magnitude sums of :func:`forward64`'s results, in its layout.  Each is the sum of |terms| of the ONE sum that makes the tensor
    from the float64 values of its inputs: sum_k |w_k grid_k| for c, sum |W| relu(x) + |b| for h_i, and for the residual stream x_i every
    term added to it so far (fc_p, the fc_c's, the fc_1's and the biases; the kernels keep it in one accumulator).  Nothing is propagated
    through a second matrix: a bound run through all five blocks over |W| grows by orders of magnitude and would gate nothing.
    ``cb`` with ``c``: the magnitude sum of the sampling that made ``c``, where the caller kept it (|c| otherwise)."""
    dt = torch.float64
    img = c_img is not None
    P, A = _params(sd, img, dt), _params(sd, img, dt, absolute=True)
    pf = pts.detach().float().to(dt)
    if c is None:
        idx, w = trilinear(pts, grid.shape[2], padding, dt)
        c, cb = sample(grid.detach().to(dt), idx, w), sample(grid.detach().to(dt).abs(), idx, w)
    else:
        c = c.detach().to(dt)
        cb = c.abs() if cb is None else cb.detach().to(dt)
    x = pf @ P["Wp"][:, :3].t() + P["bp"] + c @ P["Wc"][0].t() + P["bc"][0]
    bx = pf.abs() @ A["Wp"][:, :3].t() + A["bp"] + cb @ A["Wc"][0].t() + A["bc"][0]
    if img:
        ci = c_img.detach().to(dt)
        x, bx = x + ci @ P["Wp"][:, 3:].t(), bx + ci.abs() @ A["Wp"][:, 3:].t()
    bxs, bhs = [], []
    for i in range(NB):
        rx = torch.relu(x)
        rh = torch.relu(rx @ P["W0"][i].t() + P["b0"][i])
        bxs.append(bx)
        bhs.append(rx @ A["W0"][i].t() + A["b0"][i])
        x, bx = x + rh @ P["W1"][i].t() + P["b1"][i], bx + rh @ A["W1"][i].t() + A["b1"][i]
        if i + 1 < NB:
            x, bx = x + c @ P["Wc"][i + 1].t() + P["bc"][i + 1], bx + cb @ A["Wc"][i + 1].t() + A["bc"][i + 1]
    a = torch.relu(x)
    out = (a @ A["Wo"].t() + A["bo"]).squeeze(-1)
    bounds = [cb] + bxs + bhs + [bx]
    if contact:
        return (out, (a @ A["Wo2"].t() + A["bo2"]).squeeze(-1)), bounds
    return out, bounds


def backward(sd, pts, grid_shape, saves, grad_out, grad_out2=None, c_img=None, padding=0.1, dtype=torch.float64, absolute=False):
    """The backward given the saved activations ``saves`` (twelve [B,N,32] tensors, or one [12,B,N,32]): their values are the layer
    inputs of the weight gradients, their signs (> 0) the ReLU masks.  Returns a dict: "grad_grid" [B,R,R,R,C] (None without a
    ``grid_shape``), "grad_c" [B,N,32], "grad_c_img" (with ``c_img``) and the parameter gradients keyed like
    ops.split_decoder_grads ("fc_p.*" is fc_p_img's with ``c_img``; "fc_out_contact.*" with ``grad_out2``)."""
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)
    img = c_img is not None
    P = _params(sd, img, dtype, absolute)
    S = [s.detach().to(dtype) for s in saves]
    M = [s > 0 for s in S]
    X = [ab(s) for s in S]
    B, N = grad_out.shape
    go = ab(grad_out.detach().to(dtype)).unsqueeze(-1)
    flat = lambda v: v.reshape(B * N, -1)
    wg = lambda G, x: flat(G).t() @ flat(x)                       # nn.Linear layout [out][in]
    bg = lambda G: flat(G).sum(0)
    g = {k: [None] * NB for k in ("fc_c.weight", "fc_c.bias", "fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias")}
    g["fc_out.weight"], g["fc_out.bias"] = wg(go, X[11]), bg(go)
    G = go * P["Wo"]
    if grad_out2 is not None:
        go2 = ab(grad_out2.detach().to(dtype)).unsqueeze(-1)
        g["fc_out_contact.weight"], g["fc_out_contact.bias"] = wg(go2, X[11]), bg(go2)
        G = G + go2 * P["Wo2"]
    G = G * M[11]                                                 # d net_5
    dc = torch.zeros(B, N, 32, dtype=dtype)
    for i in range(NB - 1, -1, -1):                               # G = d (output of block i)
        g["fc_1.weight"][i], g["fc_1.bias"][i] = wg(G, X[6 + i]), bg(G)
        if i + 1 < NB:
            g["fc_c.weight"][i + 1], g["fc_c.bias"][i + 1] = wg(G, X[0]), bg(G)
            dc = dc + G @ P["Wc"][i + 1]
        t = (G @ P["W1"][i]) * M[6 + i]                           # d h_i
        g["fc_0.weight"][i], g["fc_0.bias"][i] = wg(t, X[1 + i]), bg(t)
        G = G + (t @ P["W0"][i]) * M[1 + i]                       # d x_i
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
    g["grad_c"] = dc
    g["grad_grid"] = None
    if grid_shape is not None:
        idx, w = trilinear(pts, grid_shape[2], padding, dtype)
        g["grad_grid"] = scatter(dc, idx, ab(w), grid_shape[2])
    return g


def backward64(sd, pts, grid_shape, saves, grad_out, grad_out2=None, c_img=None, padding=0.1):
    """(gradients, bounds) in float64: ``bounds`` holds, under the same keys, the same sums run over |W|, |G|, |X| and |w|."""
    return (backward(sd, pts, grid_shape, saves, grad_out, grad_out2, c_img, padding, torch.float64),
            backward(sd, pts, grid_shape, saves, grad_out, grad_out2, c_img, padding, torch.float64, absolute=True))


def backward32(sd, pts, grid_shape, saves, grad_out, grad_out2=None, c_img=None, padding=0.1):
    return backward(sd, pts, grid_shape, saves, grad_out, grad_out2, c_img, padding, torch.float32)


def gate_ratio(got, ref64, ref32, bound):
    """max over the elements of |got - ref64| / max(e32, 2^-24 bound), e32 = max |ref32 - ref64| over the tensor (a scalar); the
    tests assert it is <= 8.  An element whose base is 0 (nothing contributes to it, in any precision) must be exactly 0."""
    ref64 = ref64.double()
    err = (got.detach().double().cpu().reshape(ref64.shape) - ref64).abs()
    e32 = float((ref32.double().reshape(ref64.shape) - ref64).abs().max()) if ref64.numel() else 0.0
    base = torch.clamp(bound.double().reshape(ref64.shape) * 2.0 ** -24, min=e32)
    ratio = torch.where(base > 0, err / base.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return (float(ratio.max()) if ratio.numel() else 0.0), e32
