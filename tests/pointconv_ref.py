"""A plain reference of the PointConv baseline (CPU, torch only): the five operations behind ops.points and the two modules
(PointNetPlusPlus, LocalPointDecoder) written out from the reference's formulas, in float64 (the reference), in float32 (the
yardstick e32 of decode_train_ref.gate_ratio) and, with ``absolute=True``, over absolute values (the gate's magnitude sums).

Coordinates are float32 values; every distance is evaluated from them in the working precision as ((dx dx + dy dy) + dz dz).
The sampler is the shifted form (the query's largest exponent subtracted before the exponential); ``sample_unshifted`` is the
reference's own form (decoder.py:468-485), which is 0 / 0 once the nearest cloud point is far.  Test infrastructure.
"""
import torch
import torch.nn.functional as F

from seeded_fill import seeded_fill

EPS = 10e-6


def d2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ---- the sampler -------------------------------------------------------------------------------------------------------------
def weights(q, p, mode, gaussian_val, dtype=torch.float64, shifted=True):
    """Un-normalised weights [B,M,N] and their sums [B,M,1] for queries q [B,M,3] and cloud p [B,N,3]."""
    dist = torch.sqrt(d2(p.float().to(dtype)[:, None, :, :], q.float().to(dtype)[:, :, None, :])) + EPS
    if mode == 'gaussian':
        var = gaussian_val ** 2
        if dtype == torch.float32:
            var = float(torch.tensor(var, dtype=torch.float32))
        e = -(dist ** 2) / var
        if shifted:
            e = e - e.max(dim=2, keepdim=True)[0]
        w = e.exp()
    else:
        w = 1.0 / dist
    return w, w.sum(dim=2, keepdim=True)


def sample(q, p, fea, mode='gaussian', gaussian_val=None, dtype=torch.float64, absolute=False):
    """c [B,M,C] = sum_n w fea_n / sum_n w; ``absolute``: the same sum over |fea|."""
    w, s = weights(q, p, mode, gaussian_val, dtype)
    f = fea.detach().to(dtype)
    return (w / s) @ (f.abs() if absolute else f)


def sample_unshifted(q, p, fea, mode='gaussian', gaussian_val=None, dtype=torch.float32):
    """(c, sums) in the reference's form: NaN where the sum underflows to 0."""
    w, s = weights(q, p, mode, gaussian_val, dtype, shifted=False)
    return (w / s) @ fea.detach().to(dtype), s.squeeze(-1)


def sample_bwd(q, p, grad_c, mode='gaussian', gaussian_val=None, dtype=torch.float64, absolute=False):
    """grad_fea [B,N,C] = sum_m (w / sum) grad_c_m."""
    w, s = weights(q, p, mode, gaussian_val, dtype)
    g = grad_c.detach().to(dtype)
    return (w / s).transpose(1, 2) @ (g.abs() if absolute else g)


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def fps(xyz, npoint, start, dtype=torch.float64):
    """(indices [B,npoint], the smallest relative gap between the maximum and the runner-up over all steps): the reference's
    loop (pointnetpp.py:188-209), the lowest index among equal maxima."""
    x = xyz.float().to(dtype)
    B, N, _ = x.shape
    out = torch.zeros(B, npoint, dtype=torch.long)
    distance = torch.full((B, N), 1e10, dtype=dtype)
    far = start.clone().long()
    batch = torch.arange(B)
    gap = float("inf")
    for i in range(npoint):
        out[:, i] = far
        distance = torch.minimum(distance, d2(x, x[batch, far, :].view(B, 1, 3)))
        top = distance.max(dim=1, keepdim=True)[0]
        far = (distance == top).long().argmax(dim=1)                     # the first index that reaches the maximum
        if i + 1 < npoint and N > 1:
            two = distance.topk(2, dim=1)[0]
            rel = (two[:, 0] - two[:, 1]) / two[:, 0].clamp(min=1e-300)
            gap = min(gap, float(rel.min()))
    return out, gap


def ball_query(xyz, centres, radius, nsample, dtype=torch.float64):
    """(rows [B,S,nsample], the smallest |d^2 - radius^2| over all pairs): pointnetpp.py:212-232; a row with nothing in range is 0."""
    x, c = xyz.float().to(dtype), centres.float().to(dtype)
    B, N, _ = x.shape
    S = c.shape[1]
    sq = d2(x[:, None, :, :], c[:, :, None, :])
    group = torch.arange(N).view(1, 1, N).repeat(B, S, 1)
    group[sq > radius ** 2] = N
    group = group.sort(dim=-1)[0]
    if N < nsample:
        group = torch.cat([group, group.new_full((B, S, nsample - N), N)], dim=2)
    group = group[:, :, :nsample]
    group = torch.where(group == N, group[:, :, :1].expand(-1, -1, nsample), group)
    group = torch.where(group == N, torch.zeros_like(group), group)
    return group, float((sq - radius ** 2).abs().min())


def three_nn(tgt, src, dtype=torch.float64):
    """(idx [B,N,k], weight [B,N,k], the smallest relative gap between the k-th and the (k+1)-th distance), k = min(3, S)."""
    dist = d2(tgt.float().to(dtype)[:, :, None, :], src.float().to(dtype)[:, None, :, :])
    k = min(3, dist.shape[2])
    ds, idx = dist.sort(dim=-1, stable=True)
    gap = float("inf")
    if dist.shape[2] > k:
        gap = float(((ds[:, :, k] - ds[:, :, k - 1]) / ds[:, :, k].clamp(min=1e-300)).min())
    recip = 1.0 / (ds[:, :, :k] + 1e-8)
    return idx[:, :, :k], recip / recip.sum(dim=2, keepdim=True), gap


def index_points(points, idx):
    B = points.shape[0]
    return points[torch.arange(B).view(B, *([1] * (idx.dim() - 1))), idx, :]


def interpolate(points2, idx, weight, absolute=False):
    """sum_k weight_k points2[idx_k]: [B,N,D]."""
    f = points2.abs() if absolute else points2
    return torch.sum(index_points(f.to(weight.dtype), idx) * weight.unsqueeze(-1), dim=2)


# ---- the modules -------------------------------------------------------------------------------------------------------------
def fill(module, seed):
    """tests/seeded_fill.py, then the BatchNorm scales at 1 + 0.1 r (seeded_fill leaves them at 0.1 r: its rule knows other names)."""
    seeded_fill(module, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if "mlp_bns" in name and name.endswith(".weight"):
                t.copy_(1.0 + 0.1 * torch.randn(t.shape, generator=g))
    return module


def _mlp(sd, prefix, n, x, train, dtype):
    """n x relu(bn(conv1x1(x))) on x [B,C,...] from the state dict entries ``prefix``.mlp_convs.i / .mlp_bns.i."""
    for i in range(n):
        w = sd[f"{prefix}.mlp_convs.{i}.weight"].to(dtype)
        w = w.reshape(w.shape[0], w.shape[1])
        b = sd[f"{prefix}.mlp_convs.{i}.bias"].to(dtype)
        x = torch.einsum("oc,bc...->bo...", w, x) + b.view(1, -1, *([1] * (x.dim() - 2)))
        bn = f"{prefix}.mlp_bns.{i}."
        x = F.batch_norm(x, None if train else sd[bn + "running_mean"].to(dtype), None if train else sd[bn + "running_var"].to(dtype),
                         sd[bn + "weight"].to(dtype), sd[bn + "bias"].to(dtype), training=train, eps=1e-5)
        x = torch.relu(x)
    return x


def _sa(sd, prefix, xyz, points, npoint, radius, nsample, start, train, dtype, trace):
    """One set abstraction on xyz [B,N,3], points [B,N,D]: (centres [B,S,3], features [B,S,D'])."""
    B = xyz.shape[0]
    idx_c, _ = fps(xyz, npoint, start, dtype)
    new_xyz = index_points(xyz, idx_c)
    idx, _ = ball_query(xyz, new_xyz, radius, nsample, dtype)
    trace += [idx_c, idx]
    grouped = torch.cat([index_points(xyz, idx) - new_xyz.view(B, npoint, 1, 3), index_points(points, idx)], dim=-1)
    x = _mlp(sd, prefix, 3, grouped.permute(0, 3, 2, 1), train, dtype)
    return new_xyz, x.max(dim=2)[0].permute(0, 2, 1)


def encoder(sd, cloud, starts, train=False, dtype=torch.float64):
    """PointNetPlusPlus.forward (pointnetpp.py:116-129) from its state dict: (features [B,N,c_dim], [fps1, ball1, fps2, ball2, nn
    indices ...]).  ``starts``: the two [B] start-index draws of sa1 and sa2."""
    sd = {k: v.detach() for k, v in sd.items()}
    xyz = cloud.float().to(dtype)
    trace = []
    l1_xyz, l1 = _sa(sd, "sa1", xyz, xyz, 512, 0.2, 32, starts[0], train, dtype, trace)
    l2_xyz, l2 = _sa(sd, "sa2", l1_xyz, l1, 128, 0.4, 64, starts[1], train, dtype, trace)
    B, S2, _ = l2_xyz.shape
    g3 = torch.cat([l2_xyz, l2], dim=-1).view(B, 1, S2, -1).permute(0, 3, 2, 1)
    l3 = _mlp(sd, "sa3", 3, g3, train, dtype).max(dim=2)[0].permute(0, 2, 1)                       # [B,1,1024]

    def fp(prefix, n, xyz1, xyz2, points1, points2):
        idx, w, _ = three_nn(xyz1, xyz2, dtype)
        trace.append(idx)
        x = interpolate(points2, idx, w)
        if points1 is not None:
            x = torch.cat([points1, x], dim=-1)
        return _mlp(sd, prefix, n, x.permute(0, 2, 1), train, dtype).permute(0, 2, 1)
    l2 = fp("fp3", 2, l2_xyz, torch.zeros(B, 1, 3, dtype=dtype), l2, l3)
    l1 = fp("fp2", 2, l1_xyz, l2_xyz, l1, l2)
    return fp("fp1", 3, xyz, l1_xyz, None, l1), trace


def named_grads(sd, g):
    """decode_train_ref.backward's gradient dict under the module's parameter names."""
    out = {}
    for name in sd:
        parts = name.split('.')
        if parts[0] == 'fc_c':
            out[name] = g[f'fc_c.{parts[2]}'][int(parts[1])]
        elif parts[0] == 'blocks':
            out[name] = g[f'{parts[2]}.{parts[3]}'][int(parts[1])]
        else:
            out[name] = g[name]
        out[name] = out[name].reshape(sd[name].shape)
    return out


def decoder(sd, q, cloud, fea, occ, mode, gaussian_val=None, dtype=torch.float64):
    """LocalPointDecoder.forward (decoder.py:487-515) and the backward of F.l1_loss(logits, occ), hidden = c_dim = 32: a dict with
    'c', 'logits', 'grad_out', 'grad_c', 'grad_fea', 'grads' (by parameter name); in float64 also 'bound.*', the magnitude sums of
    the gate for 'c', 'logits', 'grad_fea' and 'grads'."""
    import decode_train_ref as D
    c = sample(q, cloud, fea, mode, gaussian_val, dtype)
    logits, saves = D.forward(sd, q, None, c=c, dtype=dtype)
    go = torch.sign(logits - occ.to(dtype)) / logits.numel()
    g = D.backward(sd, q, None, saves, go, dtype=dtype)
    out = {'c': c, 'logits': logits, 'grad_out': go, 'grad_c': g['grad_c'], 'grads': named_grads(sd, g),
           'grad_fea': sample_bwd(q, cloud, g['grad_c'], mode, gaussian_val, dtype)}
    if dtype == torch.float64:
        out['bound.c'] = sample(q, cloud, fea, mode, gaussian_val, dtype, absolute=True)
        out['bound.logits'] = D.forward_bound(sd, q, None, c=c)[0]
        out['bound.grad_fea'] = sample_bwd(q, cloud, g['grad_c'], mode, gaussian_val, dtype, absolute=True)
        out['bound.grads'] = named_grads(sd, D.backward(sd, q, None, saves, go, dtype=dtype, absolute=True))
    return out


MODES = (("gaussian", dict(sample_mode="gaussian", gaussian_val=0.1)), ("inverse", dict(sample_mode="inverse")))
SEED_ENC, SEED_DEC = 2601, 2602
MARGIN = 4.0        # a golden (or a kernel) and the float32 restatement are two float32 evaluations: 2 e32 apart at worst, times 2


def golden():
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_pointconv.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fi" else list(z[k])) for k in z.files}
