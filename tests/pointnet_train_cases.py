"""Seeded inputs of the PointNet training-path tests (CPU only): the widths and row counts of the dense kernels with a restatement of
which kernel a width takes and of their LDS needs, weights whose pre-activations are negative about half of the time, rows with every
7th gradient row zero, the constructed point sets of the pool and scatter kernels (known counts of points in chosen cells), a float32
restatement of the kernels' cell ids, and the module-level cases with the seeds the float64 reference chose.
tests/test_pointnet_train_ref_cpu.py asserts what these hold."""
import copy
import functools

import numpy as np
import torch

import pointnet_train_ref as ref

F32 = np.float32
LDS_LIMIT = 64 * 1024

# (C1, C2, H, O, shortcut layer)
WIDTHS = [(64, 0, 32, 32, True), (32, 32, 32, 32, True), (32, 0, 32, 32, False),          # the MFMA backward
          (24, 24, 24, 24, True),          # FMA backward, K = 48 straddles a 32-wide tile, 16 idle threads in the forward
          (40, 40, 40, 40, True),          # three rows per workgroup in the backward (six in the forward)
          (25, 25, 25, 25, True), (3, 0, 17, 9, True),          # scalar transpose, the dot product's tail loop, K = 3
          (47, 47, 47, 47, True),          # the widest the FMA backward holds
          (48, 0, 24, 48, False)]          # identity shortcut off the MFMA path
LINEAR = [(3, 64), (32, 48), (47, 3), (64, 256)]
POOL_CHANNELS = (8, 24, 40, 96, 128, 256, 320, 512)
SMALL_ROWS = (1, 31, 33, 127, 129, 255, 257, 1023, 1025)
TEN_CHUNKS = 9 * 1024 + 37


# ---- which kernel, how many rows, how much LDS (pointnet.hip restated) -----------------------------------------------------------
def takes_mfma(C1, C2, H, O):
    return H == 32 and O == 32 and C1 + C2 in (32, 64) and C1 % 32 == 0 and C2 % 32 == 0


def fwd_rows(H, O):
    """Rows per workgroup of vt_resblock_fc (and of vt_linear_rows with H = O = Cout)."""
    return 256 // max(H, O)


def bwd_rows(C1, C2, H, O):
    return 128 if takes_mfma(C1, C2, H, O) else 256 // max(C1 + C2, H, O)


def fwd_cap(cus, H, O):
    return 4 * cus * fwd_rows(H, O)


def bwd_cap(cus, C1, C2, H, O):
    return cus * 128 if takes_mfma(C1, C2, H, O) else 4 * cus * bwd_rows(C1, C2, H, O)


def fwd_lds_bytes(C, H, O, shortcut):
    return 4 * (C * (H | 1) + H * (O | 1) + (C * (O | 1) if shortcut else 0) + fwd_rows(H, O) * (C + H))


def bwd_fma_lds_bytes(C, H, O, shortcut):
    pts = 256 // max(C, H, O)
    return 4 * (C * (H | 1) + H * (C | 1) + O * (H | 1) + (O * (C | 1) if shortcut else 0) + pts * (C + O + 2 * H))


def hidden_fits(h):
    """What LocalPoolPointnet._fused_mlp_fits() must answer for hidden_dim h: forward, the backward the width takes and the weight
    gradient (any width) all launch at C = 2 h, H = O = h."""
    if h < 1 or 2 * h > 256 or fwd_lds_bytes(2 * h, h, h, True) > LDS_LIMIT:
        return False
    return takes_mfma(2 * h, 0, h, h) or bwd_fma_lds_bytes(2 * h, h, h, True) <= LDS_LIMIT


HIDDEN_BOUND = max(h for h in range(1, 129) if hidden_fits(h))


def with_bound_width():
    h = HIDDEN_BOUND
    w = (h, h, h, h, True)
    return WIDTHS + ([w] if w not in WIDTHS else [])


def row_counts(width, cus):
    """The row counts of a width: 1, the tile edges, one either side of a workgroup's rows (forward and backward), ten weight-gradient
    chunks, and one grid-stride round past each kernel's cap."""
    C1, C2, H, O, _ = width
    ns = set(SMALL_ROWS) | {TEN_CHUNKS}
    for r in (fwd_rows(H, O), bwd_rows(C1, C2, H, O)):
        ns |= {max(r - 1, 1), r + 1}
    ns |= {fwd_cap(cus, H, O) + 69, bwd_cap(cus, C1, C2, H, O) + 69}
    return sorted(ns)


def linear_row_counts(Cout, cus):
    r = 256 // Cout
    return sorted(set(SMALL_ROWS) | {max(r - 1, 1), r + 1, TEN_CHUNKS, 4 * cus * r + 69})


# ---- dense inputs -----------------------------------------------------------------------------------------------------------------
def block_weights(width, seed=0):
    C1, C2, H, O, short = width
    C = C1 + C2
    g = torch.Generator().manual_seed(7919 * seed + 101 * C + 11 * H + O)
    w = {"w0": torch.randn(H, C, generator=g) / C ** 0.5, "b0": 0.1 * torch.randn(H, generator=g),
         "w1": torch.randn(O, H, generator=g) / H ** 0.5, "b1": 0.1 * torch.randn(O, generator=g),
         "ws": torch.randn(O, C, generator=g) / C ** 0.5 if short else None}
    return w


def block_rows(N, width, seed=0):
    """x1 [N,C1], x2 [N,C2] or None, dout [N,O] with every 7th row zero."""
    C1, C2, H, O, _ = width
    g = torch.Generator().manual_seed(104729 * seed + 13 * N + C1 + 3 * C2)
    x1 = torch.randn(N, C1, generator=g)
    x2 = torch.randn(N, C2, generator=g) if C2 else None
    dout = torch.randn(N, O, generator=g)
    dout[::7] = 0.0
    return x1, x2, dout


def linear_case(N, Cin, Cout):
    g = torch.Generator().manual_seed(31 * N + 7 * Cin + Cout)
    x = torch.randn(N, Cin, generator=g)
    w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    b = 0.1 * torch.randn(Cout, generator=g)
    return x, w, b


# ---- cells --------------------------------------------------------------------------------------------------------------------------
PLANE_AXES = {"xz": (0, 2), "xy": (0, 1), "yz": (1, 2)}
PLANES = ("xz", "xy", "yz")


def _consts(padding, plane):
    if plane is None:
        return F32(1.0 + padding + 10e-4), F32(0.999)
    return F32(1.0 + padding + 10e-6), F32(1.0 - 10e-6)


def cell_ids32(pts, R, padding=0.1, plane=None):
    """voxel.hip's cell ids in float32 numpy: the volume (plane None: x + R (y + R z)) or a canonical plane (a0 + R a1).  int64 [B,T]."""
    p = np.asarray(pts, F32)
    d, hi = _consts(padding, plane)

    def coord(v):
        q = (v / d + F32(0.5)).astype(F32)
        q = np.where(q >= F32(1), hi, q).astype(F32)
        q = np.where(q < F32(0), F32(0), q).astype(F32)
        return (q * F32(R)).astype(F32).astype(np.int64)
    if plane is None:
        return torch.from_numpy(coord(p[..., 0]) + R * (coord(p[..., 1]) + R * coord(p[..., 2])))
    a0, a1 = PLANE_AXES[plane]
    return torch.from_numpy(coord(p[..., a0]) + R * coord(p[..., a1]))


def cell_centre(cell, R, padding=0.1):
    """float32 [3]: the centre of volume cell ``cell`` (a centre's plane cells are centres too)."""
    ijk = np.array([cell % R, (cell // R) % R, cell // (R * R)], np.float64)
    return (((ijk + 0.5) / R - 0.5) * (1.0 + padding)).astype(F32)


POOL_R = 8
# scene 0, in sorted (cell id) order: the lengths 1, 2, 31, 32, 33, 64, 65; a filler up to position 256; a long segment from the aligned
# position 256; fillers up to 415 = 384 + 31; a long segment from there; a long segment that ends the scene at T = 525 (T % 32 = 13)
SCENE0_LENGTHS = (1, 2, 31, 32, 33, 64, 65, 28, 100, 30, 29, 70, 40)
SCENE0_CELLS = tuple(7 + 37 * k for k in range(len(SCENE0_LENGTHS)))
SCENE1_CELL = 300
POOL_T = sum(SCENE0_LENGTHS)
ALIGNED_LONG, OFFSET31_LONG, LAST_LONG = 8, 11, 12          # positions in SCENE0_LENGTHS


@functools.lru_cache(maxsize=None)
def pool_points():
    """(pts float32 [2,T,3], volume cell ids [2,T] by construction): scene 0 holds SCENE0_LENGTHS[k] points at the centre of cell
    SCENE0_CELLS[k], in a seeded shuffle; every point of scene 1 sits in SCENE1_CELL."""
    rng = np.random.RandomState(525)
    ids0 = np.repeat(np.array(SCENE0_CELLS), np.array(SCENE0_LENGTHS))[rng.permutation(POOL_T)]
    ids = np.stack([ids0, np.full(POOL_T, SCENE1_CELL)])
    pts = np.stack([np.stack([cell_centre(c, POOL_R) for c in row]) for row in ids])
    return torch.from_numpy(pts), torch.from_numpy(ids.astype(np.int64))


def tie_rows(ids):
    """Per scene, pairs (or a triple) of point indices that share a cell and get the same feature row: in the cells of 2, 31 (short) and
    33, 100 (long) points of scene 0, and three points of scene 1's single cell."""
    groups = [[], []]
    for cell in (SCENE0_CELLS[1], SCENE0_CELLS[2], SCENE0_CELLS[4], SCENE0_CELLS[ALIGNED_LONG]):
        mem = torch.nonzero(ids[0] == cell).view(-1)
        groups[0].append([int(mem[len(mem) // 2]), int(mem[-1])] if len(mem) > 2 else [int(mem[0]), int(mem[1])])
    groups[1].append([5, 77, 500])
    return groups


def pool_features(C, seed=0):
    """feat [2,T,C] with the tie rows duplicated and raised (the duplicates are their cell's maximum in nearly every channel), and a
    gradient [2,T,C] with every 7th row zero."""
    _, ids = pool_points()
    g = torch.Generator().manual_seed(1000 * C + seed)
    feat = torch.randn(2, POOL_T, C, generator=g)
    for b, groups in enumerate(tie_rows(ids)):
        for grp in groups:
            feat[b, grp] = feat[b, grp[0]] + 6.0
    grad = torch.randn(2, POOL_T, C, generator=g)
    grad.view(-1, C)[::7] = 0.0
    return feat, grad


# ---- the module ----------------------------------------------------------------------------------------------------------------------
MODULE_B, MODULE_T, GRID_R, PLANE_R = 2, 301, 4, 3
# The seeds: a module case is only a test of arithmetic while no ReLU or max-pool decision of the float64 reference sits within f32
# roundoff of a tie.  Of the seeds 0..39 the one whose float64 forward keeps min(smallest |pre-ReLU value|, smallest max-pool gap)
# largest was taken (module_gaps below; tests/test_pointnet_train_ref_cpu.py repeats the search for one case) -- a choice by the
# reference alone, recorded here before any kernel ran on these inputs.
#   (hidden_dim, index): (seed, smallest |pre-ReLU|, smallest pool gap)
MODULE_SEEDS = {
    (24, "grid"): (10, 1.03e-06, 5.65e-07),
    (24, "planes"): (27, 8.79e-06, 4.18e-06),
    (32, "grid"): (33, 1.07e-06, 8.27e-07),
    (32, "planes"): (22, 3.27e-06, 2.15e-06),
    (47, "grid"): (8, 5.18e-07, 5.61e-07),          # HIDDEN_BOUND
    (48, "grid"): (19, 7.80e-07, 2.94e-07),         # HIDDEN_BOUND + 1: the nn.Linear path
}


def module_case(hidden, seed, c_dim=32):
    """(CPU float32 LocalPoolPointnet with seeded weights -- fc_1 given something to do --, points [B,T,3], output weights [B,T,c_dim])."""
    from vtaco_amd.encoder.pointnet import LocalPoolPointnet
    torch.manual_seed(1000 * hidden + seed)
    net = LocalPoolPointnet(c_dim=c_dim, dim=3, hidden_dim=hidden, grid_resolution=GRID_R, plane_type='grid')
    g = torch.Generator().manual_seed(77 * hidden + seed)
    with torch.no_grad():
        for blk in net.blocks:
            blk.fc_1.weight.copy_(torch.randn(blk.fc_1.weight.shape, generator=g) * (0.5 / hidden ** 0.5))
    p = (torch.rand(MODULE_B, MODULE_T, 3, generator=g) - 0.5) * 1.0
    wgt = torch.randn(MODULE_B, MODULE_T, c_dim, generator=g)
    return net, p, wgt


def module_indices(p, kind):
    """The cell ids of the module cases: [volume at GRID_R] or the three planes at PLANE_R."""
    if kind == "grid":
        return [cell_ids32(p.numpy(), GRID_R)]
    return [cell_ids32(p.numpy(), PLANE_R, plane=k) for k in PLANES]


def module_step(net, p, wgt, idxs, dtype):
    """One step of a CPU copy of the module in ``dtype`` through the reference pools: {"out", "grad:<name>"}."""
    m = copy.deepcopy(net).to(dtype)
    out = ref.point_features(m, p.to(dtype), idxs)
    (out * wgt.to(dtype)).sum().backward()
    res = {"out": out.detach()}
    res.update({"grad:" + n: q.grad for n, q in m.named_parameters() if q.grad is not None})
    return res


def module_gaps(net, p, idxs):
    """(smallest |pre-ReLU value|, smallest gap between a cell's two largest values) of the float64 forward."""
    m = copy.deepcopy(net).double()
    x = m.fc_pos(p.double())
    pre, gap = float("inf"), float("inf")
    with torch.no_grad():
        for i, blk in enumerate(m.blocks):
            if i:
                pooled = None
                for idx in idxs:
                    for b in range(x.shape[0]):
                        for cell in torch.unique(idx[b]):
                            mem = x[b, idx[b] == cell]
                            if mem.shape[0] > 1:
                                top = mem.topk(2, dim=0).values
                                gap = min(gap, float((top[0] - top[1]).min()))
                    pm = ref.pool_max(x, idx)[0]
                    pooled = pm if pooled is None else pooled + pm
                x = torch.cat([x, pooled], dim=2)
            h = blk.fc_0(torch.relu(x))
            pre = min(pre, float(x.abs().min()), float(h.abs().min()))
            x = blk(x)
    return pre, gap


def rel_err(t, t64):
    """|| t - t64 ||_2 / || t64 ||_2 (tests/resnet_train_util.py's L2 form)."""
    return float((t.detach().double().cpu() - t64).norm() / t64.norm())
