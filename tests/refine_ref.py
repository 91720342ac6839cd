"""The definition of the field jet and of one mesh-refinement iteration (CPU, torch only; float64 unless a dtype is passed).

The module is the 32 / 32 / 5 LocalDecoder of tests/decode_train_ref.py: f(p) = MLP(p, c(p)), c the trilinear sample of the grid at the
normalised point.  The normalisation is written as the reference writes it (in-place masked assignments: q >= 1 -> 0.999, q < 0 -> 0), so
autograd gives a clamped axis zero derivatives.

  field           the logit, from differentiable torch ops.  ``sampler='grid_sample'`` takes F.grid_sample (forward and first
                  derivative only: torch has no double backward for it -- ``derivative for aten::grid_sampler_3d_backward is not
                  implemented``); ``sampler='index'`` (the default) gathers the 8 corners by index and weights them with
                  (x0 + 1 - f), (f - x0): the same function, twice differentiable.  tests/test_refine_ref_cpu.py checks that the two
                  agree in value and gradient.
  jet_autograd    (f, f_x, f_y, f_z, f_xy, f_xz, f_yz) and the whole Hessian: autograd.grad(create_graph=True), then one grad per row.
  jet_closed      the same 7 numbers by the closed form: forward, one vector-Jacobian walk with cotangent 1 through the ReLU masks of
                  that forward (a = df/dc, b = df/dp along fc_p), phi_k = a . corner_k, derivatives of the trilinear interpolant of phi
                  times (R - 1) / divisor per free axis.  ``magnitude=True`` returns the sums over magnitudes behind each number.
  refine_loss     upstream's refine_mesh loss given eps: (target term per face, normal term per face, per-face-corner gradient [F,3,3],
                  vertex gradient [V,3]) by autograd through the gradient of sigmoid(f).
  rmsprop_step    torch.optim.RMSprop's defaults.
  refine_steps    the loop, on the CPU.
  near_kink       the running forward rounding bound of every ReLU pre-activation and grid coordinate
                  (e_out = sum |w| e_in + (n_in + 2) u sum |w| |a|, u = 2^-24); a point is near a kink when a pre-activation's
                  magnitude is at most its bound, or a grid coordinate lies within its bound of an integer or the raw normalised
                  coordinate within its bound of a clamp end (0 or 1)."""
import numpy as np
import torch
import torch.nn.functional as F

from decode_train_ref import NB, Q_HI, _params, divisor

U = 2.0 ** -24
F64 = torch.float64


def normalized(p, padding=0.1):
    q = p / divisor(padding) + 0.5
    if q.numel() and q.max() >= 1:
        q[q >= 1] = Q_HI
    if q.numel() and q.min() < 0:
        q[q < 0] = 0.0
    return q


def grid_coords(p, R, padding=0.1):
    """The continuous grid coordinate in [0, R-1] (align_corners, border clip), differentiable."""
    q = normalized(p, padding)
    return ((((2 * q - 1) + 1) / 2) * (R - 1)).clamp(0, R - 1)


def _corners(f, R):
    f0 = f.detach().floor()
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
    return torch.stack(idx, -1), torch.stack(w, -1), i0


def sample(grid, p, padding=0.1, sampler="index"):
    """c [N,C] at p [N,3] from grid [1,C,R,R,R] (already in p's dtype)."""
    R = grid.shape[2]
    if sampler == "grid_sample":
        vgrid = 2.0 * normalized(p, padding) - 1.0
        return F.grid_sample(grid, vgrid[None, :, None, None], padding_mode="border", align_corners=True,
                             mode="bilinear").squeeze(-1).squeeze(-1)[0].t()
    idx, w, _ = _corners(grid_coords(p, R, padding), R)
    gcl = grid[0].permute(1, 2, 3, 0).reshape(-1, grid.shape[1])
    return (gcl[idx] * w.unsqueeze(-1)).sum(1)


def _mlp(P, p, c):
    """(logit [N], the 11 ReLU pre-activations in the order x_0..x_4, h_0..h_4, net_5)."""
    x = F.linear(p, P["Wp"][:, :3], P["bp"]) + F.linear(c, P["Wc"][0], P["bc"][0])
    xs, hs = [], []
    for i in range(NB):
        xs.append(x)
        h = F.linear(torch.relu(x), P["W0"][i], P["b0"][i])
        hs.append(h)
        x = x + F.linear(torch.relu(h), P["W1"][i], P["b1"][i])
        if i + 1 < NB:
            x = x + F.linear(c, P["Wc"][i + 1], P["bc"][i + 1])
    return F.linear(torch.relu(x), P["Wo"], P["bo"]).squeeze(-1), xs + hs + [x]


def field(sd, grid, p, padding=0.1, sampler="index", pre=False):
    """The logit [N] at p [N,3] (p's dtype is the working precision)."""
    P = _params(sd, False, p.dtype)
    out, acts = _mlp(P, p, sample(grid.detach().to(p.dtype), p, padding, sampler))
    return (out, acts) if pre else out


def _grad(y, x):
    if not y.requires_grad:
        return torch.zeros_like(x)
    g, = torch.autograd.grad(y, x, create_graph=True, allow_unused=True)
    return torch.zeros_like(x) if g is None else g


def jet_autograd(sd, grid, pts, padding=0.1, dtype=F64):
    """(jet [N,7], hessian [N,3,3]) by autograd on the index sampler."""
    p = pts.detach().float().to(dtype).clone().requires_grad_()
    f = field(sd, grid, p, padding)
    g = _grad(f.sum(), p)
    H = torch.stack([_grad(g[:, j].sum(), p) for j in range(3)], 1).detach()
    jet = torch.cat([f.detach()[:, None], g.detach(), H[:, 0, 1:2], H[:, 0, 2:3], H[:, 1, 2:3]], 1)
    return jet, H


def jet_closed(sd, grid, pts, padding=0.1, dtype=F64, magnitude=False):
    """jet [N,7] by the closed form; with ``magnitude`` also the sum over magnitudes behind each of the 7 numbers."""
    P = _params(sd, False, dtype)
    A = _params(sd, False, dtype, absolute=True)
    p = pts.detach().float().to(dtype)
    g = grid.detach().to(dtype)
    R, C = g.shape[2], g.shape[1]
    q_raw = p / divisor(padding) + 0.5
    free = ((q_raw < 1) & (q_raw >= 0)).to(dtype)
    f = grid_coords(p.clone(), R, padding)
    idx, w, i0 = _corners(f, R)
    gcl = g[0].permute(1, 2, 3, 0).reshape(-1, C)
    rows = gcl[idx]                                                # [N,8,C]
    c = (rows * w.unsqueeze(-1)).sum(1)
    out, acts = _mlp(P, p, c)
    M = [(a > 0).to(dtype) for a in acts]                          # x_0..x_4 | h_0..h_4 | net_5
    G = P["Wo"].expand(p.shape[0], -1) * M[10]
    Gm = A["Wo"].expand(p.shape[0], -1) * M[10]
    dc = torch.zeros(p.shape[0], C, dtype=dtype)
    dcm = torch.zeros_like(dc)
    for i in range(NB - 1, -1, -1):
        if i + 1 < NB:
            dc, dcm = dc + G @ P["Wc"][i + 1], dcm + Gm @ A["Wc"][i + 1]
        t, tm = (G @ P["W1"][i]) * M[5 + i], (Gm @ A["W1"][i]) * M[5 + i]
        G, Gm = G + (t @ P["W0"][i]) * M[i], Gm + (tm @ A["W0"][i]) * M[i]
    dc, dcm = dc + G @ P["Wc"][0], dcm + Gm @ A["Wc"][0]
    b, bm = G @ P["Wp"][:, :3], G.abs() @ A["Wp"][:, :3]
    phi = (rows * dc.unsqueeze(1)).sum(-1)                         # [N,8]
    phim = (rows.abs() * dc.abs().unsqueeze(1)).sum(-1)
    f0 = i0.to(dtype)
    inside = (i0 + 1 <= R - 1).to(dtype)
    w1 = (f - f0) * inside
    w0 = (f0 + 1) - f
    s = free * ((R - 1) / divisor(padding))

    def interp(ph, sign):
        """d/d(axis set) of the trilinear interpolant of ph: corner k enters with the product over the differentiated axes of
        (+1 upper, -1 lower) -- |.| with ``sign`` False -- and the weights of the others."""
        outs = {}
        for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
            acc = torch.zeros(p.shape[0], dtype=dtype)
            for k in range(8):
                coef = torch.ones(p.shape[0], dtype=dtype)
                for ax in range(3):
                    up = (k >> ax) & 1
                    if ax in axes:
                        coef = coef * ((1.0 if up else -1.0) if sign else 1.0)
                    else:
                        coef = coef * (w1 if up else w0)[:, ax]
                acc = acc + coef * ph[:, k]
            outs[axes] = acc
        return outs
    T = interp(phi, True)
    jet = torch.stack([out, b[:, 0] + s[:, 0] * T[(0,)], b[:, 1] + s[:, 1] * T[(1,)], b[:, 2] + s[:, 2] * T[(2,)],
                       s[:, 0] * s[:, 1] * T[(0, 1)], s[:, 0] * s[:, 2] * T[(0, 2)], s[:, 1] * s[:, 2] * T[(1, 2)]], 1)
    if not magnitude:
        return jet
    Tm = interp(phim, False)
    relu_net = torch.relu(acts[10])
    fm = relu_net @ A["Wo"][0] + A["bo"].abs()
    mag = torch.stack([fm, bm[:, 0] + s[:, 0] * Tm[(0,)], bm[:, 1] + s[:, 1] * Tm[(1,)], bm[:, 2] + s[:, 2] * Tm[(2,)],
                       s[:, 0] * s[:, 1] * Tm[(0, 1)], s[:, 0] * s[:, 2] * Tm[(0, 2)], s[:, 1] * s[:, 2] * Tm[(1, 2)]], 1)
    return jet, mag


def masks_and_cells(sd, grid, pts, padding=0.1, dtype=F64):
    """(ReLU masks [N,11*32] bool, cells [N,3] int64, clamp pattern [N,3] int64) of the forward in ``dtype``."""
    p = pts.detach().float().to(dtype)
    R = grid.shape[2]
    q_raw = p / divisor(padding) + 0.5
    _, acts = field(sd, grid, p.clone(), padding, pre=True)
    cells = grid_coords(p.clone(), R, padding).floor().long()
    return torch.cat([a > 0 for a in acts], 1), cells, (q_raw >= 1).long() - (q_raw < 0).long()


def near_kink(sd, grid, pts, padding=0.1):
    """bool [N]: some ReLU pre-activation or grid coordinate of the float64 forward lies within its float32 rounding bound of a kink."""
    dt = F64
    P, A = _params(sd, False, dt), _params(sd, False, dt, absolute=True)
    p = pts.detach().float().to(dt)
    g = grid.detach().to(dt)
    R, C = g.shape[2], g.shape[1]
    d = divisor(padding)
    q_raw = p / d + 0.5
    e_q = U * (p.abs() / d) + U * q_raw.abs()                      # one rounding each, of the result: the division, the addition
    f = grid_coords(p.clone(), R, padding)
    qc = normalized(p.clone(), padding)                            # in [0, 1)
    # g = 2 q - 1 (one rounding of |g| <= 1), g + 1 (one of 2 q), the halving is exact, the scale by R - 1 (one of f); the clip is exact
    e_f = (R - 1) * (e_q + U * (2 * qc - 1).abs() / 2 + U * qc) + U * f
    # (a clamped axis sits at f = 0 or 0.999 (R - 1) in every precision and has zero derivatives: only a free axis can change cell)
    free = (q_raw < 1) & (q_raw >= 0)
    near = ((q_raw - 1).abs() <= e_q).any(1) | (q_raw.abs() <= e_q).any(1) | (free & ((f - f.round()).abs() <= e_f)).any(1)
    idx, w, i0 = _corners(f, R)
    rows = g[0].permute(1, 2, 3, 0).reshape(-1, C)[idx]            # [N,8,C]
    # a corner's weight is a product of three factors, each off by its axis' e_f (the subtraction from the integer is exact in
    # float32 to within that): e_w = sum_axis e_f[axis] prod_(other axes) factor + 2 u w
    f0 = i0.to(dt)
    fac = [(f0 + 1) - f, torch.where(i0 + 1 <= R - 1, f - f0, torch.zeros_like(f))]
    e_w = []
    for k in range(8):
        up = [(k >> ax) & 1 for ax in range(3)]
        e_w.append(e_f[:, 0] * fac[up[1]][:, 1] * fac[up[2]][:, 2] + fac[up[0]][:, 0] * e_f[:, 1] * fac[up[2]][:, 2]
                   + fac[up[0]][:, 0] * fac[up[1]][:, 1] * e_f[:, 2] + 2 * U * w[:, k])
    e_w = torch.stack(e_w, 1)                                      # [N,8]
    c = (rows * w.unsqueeze(-1)).sum(1)
    cm = (rows.abs() * w.unsqueeze(-1)).sum(1)
    e_c = (rows.abs() * e_w.unsqueeze(-1)).sum(1) + (8 + 2) * U * cm

    def lin(Aw, e_in, mag_in, bias, n_in):
        """e_out = sum |w| e_in + (n_in + 2) u (sum |w| |a| + |b|)"""
        m = mag_in @ Aw.t() + bias
        return e_in @ Aw.t() + (n_in + 2) * U * m, m
    ep, mp = lin(A["Wp"][:, :3], torch.zeros_like(p), p.abs(), A["bp"], 3)
    ec, mc = lin(A["Wc"][0], e_c, c.abs(), A["bc"][0], C)
    x = F.linear(p, P["Wp"][:, :3], P["bp"]) + F.linear(c, P["Wc"][0], P["bc"][0])
    e_x, m_x = ep + ec + 2 * U * (mp + mc), mp + mc
    for i in range(NB):
        near |= (x.abs() <= e_x).any(1)
        rx = torch.relu(x)
        h = F.linear(rx, P["W0"][i], P["b0"][i])
        e_h, _ = lin(A["W0"][i], e_x, rx, A["b0"][i], 32)
        near |= (h.abs() <= e_h).any(1)
        rh = torch.relu(h)
        e1, m1 = lin(A["W1"][i], e_h, rh, A["b1"][i], 32)
        x, e_x, m_x = x + F.linear(rh, P["W1"][i], P["b1"][i]), e_x + e1, m_x + m1
        if i + 1 < NB:
            e2, m2 = lin(A["Wc"][i + 1], e_c, c.abs(), A["bc"][i + 1], C)
            x, e_x, m_x = x + F.linear(c, P["Wc"][i + 1], P["bc"][i + 1]), e_x + e2, m_x + m2
        e_x = e_x + 2 * U * m_x                                    # the residual additions
    near |= (x.abs() <= e_x).any(1)
    return near


# ---- refinement ------------------------------------------------------------------------------------------------------------------
def face_points(verts, faces, eps):
    return (verts[faces] * eps[:, :, None]).sum(dim=1)


def refine_loss(sd, grid, verts, faces, eps, threshold, padding=0.1, weight=0.01, dtype=F64):
    """Upstream's loss at the face points ``sum_i eps_i v_i``.  Returns (target [F], normal [F], per-face-corner gradient [F,3,3],
    vertex gradient [V,3]) of L = mean(target) + weight mean(normal)."""
    faces = faces.long()
    v = verts.detach().float().to(dtype)
    fv = v[faces].clone().requires_grad_()
    e = eps.detach().float().to(dtype)
    fp = (fv * e[:, :, None]).sum(dim=1)
    v1, v2 = fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 1]
    n = torch.linalg.cross(v1, v2)
    n = n / (n.norm(dim=1, keepdim=True) + 1e-10)
    val = torch.sigmoid(field(sd, grid, fp, padding))
    nt = -_grad(val.sum(), fp)
    nt = nt / (nt.norm(dim=1, keepdim=True) + 1e-10)
    target = (val - threshold).pow(2)
    normal = (n - nt).pow(2).sum(dim=1)
    loss = target.mean() + weight * normal.mean()
    gfv, = torch.autograd.grad(loss, fv)
    gv = torch.zeros_like(v).index_add_(0, faces.reshape(-1), gfv.reshape(-1, 3))
    return target.detach(), normal.detach(), gfv, gv


def rmsprop_step(v, g, sq, lr=1e-4, alpha=0.99, eps=1e-8):
    sq = alpha * sq + (1 - alpha) * g * g
    return v - lr * g / (sq.sqrt() + eps), sq


def refine_steps(sd, grid, verts, faces, eps_steps, threshold, padding=0.1, weight=0.01, lr=1e-4):
    """The loop in float64 from float32 vertices: eps_steps [steps,F,3]."""
    v = verts.detach().float().double()
    sq = torch.zeros_like(v)
    for eps in eps_steps:
        _, _, _, g = refine_loss(sd, grid, v, faces, eps, threshold, padding, weight)
        v, sq = rmsprop_step(v, g, sq, lr)
    return v


# ---- seeded inputs shared by the CPU and GPU tests ------------------------------------------------------------------------------------
GAIN = 0.15         # tests/seeded_fill.py's weight scale for the jet tests: keeps the running bound's growth through the five blocks low
WEIGHT_SEED = 20


# every point set tests/test_field_jet_gpu.py checks against float64: (B, N, R).  N = 32 k + 5 below and above the 8 tiles a workgroup
# takes at a time, one odd grid, two scenes, a single point.
JET_CASES = [(1, 1, 5), (1, 37, 5), (2, 32 * 9 + 5, 5), (1, 32 * 70 + 5, 8), (2, 32 * 20 + 5, 8)]


def seeded_decoder(seed=WEIGHT_SEED, gain=GAIN):
    from seeded_fill import seeded_fill
    from vtaco_amd.conv_onet.models import decoder_dict
    return seeded_fill(decoder_dict["simple_local"](dim=3, c_dim=32, hidden_size=32), seed, gain)


def jet_points(B, N, R, seed=0, padding=0.1):
    """float32 [B,N,3]: uniform over +-0.6 (a tenth of them beyond the box on one axis, both directions), plus -- from N >= 64 -- six
    points pushed out along each axis and direction and six in the last cell (q just under 1)."""
    rng = np.random.RandomState(7919 * R + 31 * B + N + seed)
    d = divisor(padding)
    pts = ((rng.rand(B, N, 3) - 0.5) * 1.2).astype(np.float32)
    if N >= 64:
        for b in range(B):
            for j in range(6):
                pts[b, j, j % 3] = np.float32((1 if j < 3 else -1) * (0.5 * d + 0.01 + 0.1 * rng.rand()))
                pts[b, 6 + j] = np.float32(0.5 * d * (1 - 1e-3 * (1 + rng.rand(3))))
                pts[b, 6 + j, (j + 1) % 3] = np.float32((rng.rand() - 0.5))
    return torch.from_numpy(pts)


def jet_grid(B, R, seed=0):
    return torch.randn(B, 32, R, R, R, generator=torch.Generator().manual_seed(4001 * R + B + seed))
