"""A plain reference of the PointNet encoder's training path (CPU, torch only): the row-wise linear layer, ResnetBlockFC on the virtual
concat [x1 | x2] with its data and weight gradients, and the segment pools and scatter-means over cell ids -- each in float64 (the
reference), in float32 (the yardstick e32) and over absolute values (the magnitude sums behind the rounding floor of the gate,
tests/decode_train_ref.py gate_ratio).  ``forms(fn, ...)`` returns the three.

Layouts are the kernels': rows [N, C], nn.Linear weights [out][in], features [B, T, C], cell ids [B, T] (any integers: equal id = same
cell).  A bound is the same sum run over |inputs|; where a tensor is made from an intermediate of the same call (d x from d h) the
intermediate's bound is carried on, as the decoder's backward reference does within a block."""
import torch

F64, F32 = torch.float64, torch.float32


def forms(fn, *args, **kw):
    """(float64, float32, magnitude bound) of ``fn``."""
    return fn(*args, dtype=F64, **kw), fn(*args, dtype=F32, **kw), fn(*args, dtype=F64, absolute=True, **kw)


def _t(v, dtype, absolute=False):
    v = v.detach().cpu().to(dtype)
    return v.abs() if absolute else v


def _cat(x1, x2, dtype):
    x = _t(x1, dtype)
    return x if x2 is None else torch.cat([x, _t(x2, dtype)], -1)


def stray(got, bound):
    """The number of elements of ``got`` that are not exactly 0 although nothing contributes to them (their magnitude bound is 0)."""
    b = bound.detach().double().cpu()
    return int(((got.detach().double().cpu().reshape(b.shape) != 0) & (b == 0)).sum())


# ---- dense layers ------------------------------------------------------------------------------------------------------------------
def linear_rows(x, w, b=None, dtype=F64, absolute=False):
    """out[n][j] = b[j] + sum_k w[j][k] x[n][k]."""
    out = _t(x, dtype, absolute) @ _t(w, dtype, absolute).t()
    return out if b is None else out + _t(b, dtype, absolute)


def resblock_hidden(x1, x2, w0, b0, dtype=F64, absolute=False):
    """h = b0 + W0 relu([x1 | x2])  [N, H] (relu(h) is the kernels' ``act``); the bound: |b0| + |W0| relu(x)."""
    rx = torch.relu(_cat(x1, x2, dtype))
    return rx @ _t(w0, dtype, absolute).t() + _t(b0, dtype, absolute)


def resblock_act(x1, x2, w0, b0, dtype=F64, absolute=False):
    h = resblock_hidden(x1, x2, w0, b0, dtype, absolute)
    return h if absolute else torch.relu(h)


def resblock_fwd(x1, x2, w0, b0, w1, b1, ws, dtype=F64, absolute=False, swap=False):
    """out = b1 + W1 relu(h) + (Ws x, or x without a shortcut layer), x = [x1 | x2] (``swap``: [x2 | x1], a perturbation for the
    bite checks).  The bound takes relu(h) at its float64 value: |b1| + |W1| relu(h) + |Ws| |x|."""
    x = _cat(x2, x1, dtype) if swap else _cat(x1, x2, dtype)
    a = torch.relu(torch.relu(x) @ _t(w0, dtype).t() + _t(b0, dtype))
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)
    out = a @ _t(w1, dtype, absolute).t() + _t(b1, dtype, absolute)
    return out + (ab(x) @ _t(ws, dtype, absolute).t() if ws is not None else ab(x))


def resblock_bwd(x1, x2, w0, w1, ws, dout, mask_h, dtype=F64, absolute=False):
    """Data gradient given d out [N, O] and the mask [h > 0] ([N, H] bool; the GPU test passes the kernel's own act > 0):
    d h = (d out W1) . mask_h;  d x = (d h W0) . [x > 0] + d out Ws (or + d out).  Returns (dx1, dx2 or None, dh)."""
    x = _cat(x1, x2, dtype)
    C1 = x1.shape[-1]
    go = _t(dout, dtype, absolute)
    m = mask_h.detach().cpu()
    dh = (go @ _t(w1, dtype, absolute)) * m
    dx = (dh @ _t(w0, dtype, absolute)) * (x > 0) + (go @ _t(ws, dtype, absolute) if ws is not None else go)
    return dx[..., :C1], (dx[..., C1:] if x2 is not None else None), dh


def rows_wgrad(g, x1, x2=None, relu_x=False, dtype=F64, absolute=False, rows=None):
    """(dW [M, K], db [M]) of a linear layer over the rows: dW = g^T [x1 | x2] (x relu'd with ``relu_x``), db = column sums of g.
    ``rows``: only the first ``rows`` rows (a perturbation for the bite checks)."""
    x = _cat(x1, x2, dtype)
    x = torch.relu(x) if relu_x else (x.abs() if absolute else x)
    G = _t(g, dtype, absolute)
    G, x = G.reshape(-1, G.shape[-1])[:rows], x.reshape(-1, x.shape[-1])[:rows]
    return G.t() @ x, G.sum(0)


# ---- cells ---------------------------------------------------------------------------------------------------------------------------
def _segments(idx_b):
    """(inverse [T] -> dense cell number, counts per cell) of one scene's cell ids."""
    _, inv, cnt = torch.unique(idx_b.detach().cpu().long(), return_inverse=True, return_counts=True)
    return inv, cnt


def segment_sum(v, idx, dtype=F64, absolute=False):
    """Per point, the sum of ``v`` over the points of its cell, added in point order; and the cell's count [B, T]."""
    v = _t(v, dtype, absolute)
    out, n = torch.empty_like(v), torch.empty(v.shape[:2], dtype=torch.long)
    for b in range(v.shape[0]):
        inv, cnt = _segments(idx[b])
        out[b] = torch.zeros(cnt.numel(), v.shape[2], dtype=dtype).index_add_(0, inv, v[b])[inv]
        n[b] = cnt[inv]
    return out, n


def pool_max(feat, idx, last=False):
    """(out [B,T,C], arg [B,T,C]): per cell and channel the maximum, gathered back, and the point index of its FIRST occurrence in
    point order (``last``: of the last, a perturbation).  Exact in any precision: the values are the inputs'."""
    f = feat.detach().cpu()
    B, T, C = f.shape
    out, arg = torch.empty_like(f), torch.empty(B, T, C, dtype=torch.long)
    for b in range(B):
        inv, cnt = _segments(idx[b])
        for s in range(cnt.numel()):
            mem = torch.nonzero(inv == s).view(-1)                  # ascending point indices
            fs = f[b, mem]
            m = fs.max(0).values
            hit = (fs == m)
            if last:
                pos = fs.shape[0] - 1 - hit.flip(0).int().argmax(0)
            else:
                pos = hit.int().argmax(0)                           # the first maximal value
            out[b, mem] = m
            arg[b, mem] = mem[pos]
    return out, arg


def pool_max_bwd(grad_out, arg, idx, dtype=F64, absolute=False):
    """grad_feat[b][t][c] = [arg[b][t][c] == t] * sum of grad_out[b][.][c] over t's cell."""
    tot, _ = segment_sum(grad_out, idx, dtype, absolute)
    T = tot.shape[1]
    own = arg.detach().cpu().long() == torch.arange(T).view(1, T, 1)
    return tot * own


def pool_max_sum(feat, idxs, dtype=F64, absolute=False):
    """sum_k pool_max(feat, idxs[k]) in partition order."""
    out = None
    for idx in idxs:
        m = _t(pool_max(feat, idx)[0], dtype, absolute)
        out = m if out is None else out + m
    return out


def pool_max_sum_bwd(grad_out, args, idxs, dtype=F64, absolute=False):
    out = None
    for arg, idx in zip(args, idxs):
        g = pool_max_bwd(grad_out, arg, idx, dtype, absolute)
        out = g if out is None else out + g
    return out


def pool_mean(feat, idx, dtype=F64, absolute=False, long_div=None):
    """Per point, the mean of its cell (self-adjoint: the backward is the same map).  ``long_div``: cells of more than 32 points divide
    by it instead of their count (a perturbation)."""
    tot, n = segment_sum(feat, idx, dtype, absolute)
    div = n.to(dtype)
    if long_div is not None:
        div = torch.where(n > 32, torch.full_like(div, float(long_div)), div)
    return tot / div.unsqueeze(-1)


def scatter_mean(feat, idx, V, dtype=F64, absolute=False, channels_last=False, long_div=None):
    """Cell means into a zero-filled grid of V cells: [B, C, V], or [B, V, C] with ``channels_last``."""
    mean = pool_mean(feat, idx, dtype, absolute, long_div)
    B, T, C = mean.shape
    grid = torch.zeros(B, V, C, dtype=dtype)
    ix = idx.detach().cpu().long().unsqueeze(-1).expand(-1, -1, C)
    grid.scatter_(1, ix, mean)                                      # every member of a cell writes the same mean
    return grid if channels_last else grid.permute(0, 2, 1).contiguous()


def scatter_mean_bwd(grad_grid, idx, dtype=F64, absolute=False, channels_last=False):
    """grad_feat[b][t][c] = grad_grid[b][c][cell(t)] / count(cell(t)); grad_grid [B, C, V] or [B, V, C]."""
    g = _t(grad_grid, dtype, absolute)
    g = g if channels_last else g.permute(0, 2, 1)
    B, V, C = g.shape
    ix = idx.detach().cpu().long()
    n = torch.stack([(lambda ic: ic[1][ic[0]])(_segments(ix[b])) for b in range(B)]).to(dtype)
    return torch.gather(g, 1, ix.unsqueeze(-1).expand(-1, -1, C)) / n.unsqueeze(-1)


def scatter_mean_multi(feat, idxs, V, dtype=F64, absolute=False):
    """The partitions' scatter-means one after the other: [n * B, C, V]."""
    return torch.cat([scatter_mean(feat, idx, V, dtype, absolute) for idx in idxs], 0)


def scatter_mean_multi_bwd(grad_planes, idxs, dtype=F64, absolute=False):
    """grad_planes [n * B, C, V] -> sum_k (partition k's scatter_mean_bwd), in partition order."""
    B = grad_planes.shape[0] // len(idxs)
    out = None
    for k, idx in enumerate(idxs):
        g = scatter_mean_bwd(grad_planes[k * B:(k + 1) * B], idx, dtype, absolute)
        out = g if out is None else out + g
    return out


# ---- the module ----------------------------------------------------------------------------------------------------------------------
class _GatherPool(torch.autograd.Function):
    """pool_max under autograd: the gradient of a cell goes to its first maximum."""

    @staticmethod
    def forward(ctx, feat, idx):
        out, arg = pool_max(feat, idx)
        ctx.arg, ctx.idx = arg, idx
        return out

    @staticmethod
    def backward(ctx, grad):
        return pool_max_bwd(grad, ctx.arg, ctx.idx, dtype=grad.dtype), None


def point_features(module, p, idxs):
    """LocalPoolPointnet.point_features (scatter_type 'max') of a CPU copy of the module in its own dtype, through its nn.Linear
    layers, the pools summed over the partitions ``idxs`` (a list of [B,T] cell ids) in order."""
    net = module.blocks[0](module.fc_pos(p))
    for blk in module.blocks[1:]:
        pooled = None
        for idx in idxs:
            m = _GatherPool.apply(net, idx)
            pooled = m if pooled is None else pooled + m
        net = blk(torch.cat([net, pooled], dim=2))
    return module.fc_c(net)
