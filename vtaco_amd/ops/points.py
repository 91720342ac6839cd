"""The PointConv baseline's kernels: the point-feature sampler (vt_point_sample_fwd / _bwd) and the PointNet++ geometry (vt_fps,
vt_ball_query, vt_three_nn).  Reached as ``ops.points.name``: the module adds no name to ``vtaco_amd.ops`` itself."""
import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c

I64 = torch.int64


def _mode(sample_mode, gaussian_val):
    """(gaussian flag, gaussian_val) of a decoder's sample_mode: 'gaussian', or anything else = inverse distance (decoder.py:473-478)."""
    if sample_mode == 'gaussian':
        if gaussian_val is None or not float(gaussian_val) > 0:
            raise VtError(f"point_sample: sample_mode 'gaussian' needs gaussian_val > 0 (got {gaussian_val!r})")
        return 1, float(gaussian_val)
    return 0, 0.0


def _cloud(cloud, fea, what):
    cloud, fea = _c(cloud.float()), _c(fea.float())
    if cloud.dim() != 3 or cloud.shape[2] != 3 or fea.dim() != 3 or fea.shape[:2] != cloud.shape[:2]:
        raise VtError(f"{what}: cloud [B,N,3] and features [B,N,C] (got {tuple(cloud.shape)}, {tuple(fea.shape)})")
    return cloud, fea


def point_sample(cloud, fea, pts=None, lattice=None, sample_mode='gaussian', gaussian_val=None, want_saved=False):
    """c [B,M,C]: the normalised kernel-weighted sum of ``fea`` [B,N,C] over ``cloud`` [B,N,3] at the queries ``pts`` [B,M,3], or with
    ``lattice=(nx, box, first, count)`` at ``box * make_3d_grid(...)[first:first+count]`` generated in the kernel -- bit for bit the
    point form's result on those points.  ``want_saved``: also the per-query (shift, sum) [B,M] the backward needs."""
    if (pts is None) == (lattice is None):
        raise VtError("point_sample: give the queries as pts [B,M,3] or as lattice=(nx, box, first, count), one of the two")
    cloud, fea = _cloud(cloud, fea, "point_sample")
    B, N, C = fea.shape
    gaussian, gval = _mode(sample_mode, gaussian_val)
    if pts is not None:
        pts = _c(pts.float())
        if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] != 3:
            raise VtError(f"point_sample: pts must be [B,M,3] with B={B} (got {tuple(pts.shape)})")
        M, nx, box, first = pts.shape[1], 0, 0.0, 0
    else:
        nx, box, first, M = lattice
        if nx < 2 or first < 0 or M < 0 or first + M > nx ** 3:
            raise VtError(f"point_sample: slab [{first}, {first + M}) outside the {nx}^3 lattice")
    out = torch.empty((B, M, C), dtype=torch.float32, device=fea.device)
    shift = torch.empty((B, M), dtype=torch.float32, device=fea.device)
    total = torch.empty((B, M), dtype=torch.float32, device=fea.device)
    if M == 0:
        return (out, shift, total) if want_saved else out
    check(_lib.load().vt_point_sample_fwd(dev_ptr(pts, "pts"), int(M), int(nx), float(box), int(first), dev_ptr(cloud, "cloud"),
                                          dev_ptr(fea, "fea"), B, N, C, gaussian, gval, dev_ptr(out, "out"), dev_ptr(shift, "shift"),
                                          dev_ptr(total, "sum"), stream_ptr()), "vt_point_sample_fwd")
    return (out, shift, total) if want_saved else out


def point_sample_bwd(cloud, pts, shift, total, grad_c, sample_mode='gaussian', gaussian_val=None):
    """grad_fea [B,N,C] of point_sample from ``grad_c`` [B,M,C] and the forward's saved (shift, sum); the same bits every run."""
    cloud, pts, grad_c = _c(cloud.float()), _c(pts.float()), _c(grad_c.float())
    B, N = cloud.shape[:2]
    M, C = grad_c.shape[1], grad_c.shape[2]
    if tuple(pts.shape) != (B, M, 3) or grad_c.shape[0] != B or tuple(shift.shape) != (B, M) or tuple(total.shape) != (B, M):
        raise VtError(f"point_sample_bwd: pts [B,M,3], grad_c [B,M,C], shift and sum [B,M] with B={B} (got {tuple(pts.shape)}, "
                      f"{tuple(grad_c.shape)}, {tuple(shift.shape)}, {tuple(total.shape)})")
    gaussian, gval = _mode(sample_mode, gaussian_val)
    lib = _lib.load()
    grad_fea = torch.empty((B, N, C), dtype=torch.float32, device=grad_c.device)
    wsb = lib.vt_point_sample_bwd_workspace_bytes(B, M, N, C)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=grad_c.device)
    check(lib.vt_point_sample_bwd(dev_ptr(pts, "pts"), M, dev_ptr(cloud, "cloud"), B, N, C, gaussian, gval, dev_ptr(_c(shift), "shift"),
                                  dev_ptr(_c(total), "sum"), dev_ptr(grad_c, "grad_c"), dev_ptr(grad_fea, "grad_fea"),
                                  dev_ptr(ws, "workspace", torch.uint8), ws.numel(), stream_ptr()), "vt_point_sample_bwd")
    return grad_fea


def _xyz(t, what):
    t = _c(t.float())
    if t.dim() != 3 or t.shape[2] != 3:
        raise VtError(f"{what} must be [B,N,3] (got {tuple(t.shape)})")
    return t


def fps(xyz, npoint, start):
    """Farthest-point sampling (vt_fps): indices int64 [B,npoint] beginning at ``start`` [B] (int64; a CPU tensor is checked
    against the cloud and copied over)."""
    xyz = _xyz(xyz, "fps: xyz")
    B, N = xyz.shape[:2]
    if tuple(start.shape) != (B,):
        raise VtError(f"fps: start must be [B]=({B},) (got {tuple(start.shape)})")
    if not start.is_cuda:
        if N and (int(start.min()) < 0 or int(start.max()) >= N):
            raise VtError(f"fps: start indices must lie in [0, {N})")
        start = start.to(xyz.device)
    start = _c(start.to(I64))
    out = torch.empty((B, int(npoint)), dtype=I64, device=xyz.device)
    dist = torch.empty((B, max(N, 1)), dtype=torch.float32, device=xyz.device)
    check(_lib.load().vt_fps(dev_ptr(xyz, "xyz"), B, N, int(npoint), dev_ptr(start, "start", I64), dev_ptr(dist, "dist"),
                             dev_ptr(out, "out", I64), stream_ptr()), "vt_fps")
    return out


def ball_query(xyz, centres, radius, nsample):
    """Ball query (vt_ball_query): int64 [B,S,nsample], per centre the lowest ``nsample`` indices within ``radius`` in ascending
    order, a short row padded with its first entry."""
    xyz, centres = _xyz(xyz, "ball_query: xyz"), _xyz(centres, "ball_query: centres")
    B, N = xyz.shape[:2]
    S = centres.shape[1]
    if centres.shape[0] != B:
        raise VtError(f"ball_query: xyz and centres share B (got {B}, {centres.shape[0]})")
    out = torch.empty((B, S, int(nsample)), dtype=I64, device=xyz.device)
    check(_lib.load().vt_ball_query(dev_ptr(xyz, "xyz"), B, N, dev_ptr(centres, "centres"), S, float(radius), int(nsample),
                                    dev_ptr(out, "out", I64), stream_ptr()), "vt_ball_query")
    return out


def three_nn(tgt, src):
    """(idx int64 [B,N,k], weight [B,N,k]) with k = min(3, S): every target's nearest sources and their normalised inverse squared
    distance weights (vt_three_nn)."""
    tgt, src = _xyz(tgt, "three_nn: tgt"), _xyz(src, "three_nn: src")
    B, N = tgt.shape[:2]
    S = src.shape[1]
    if src.shape[0] != B:
        raise VtError(f"three_nn: tgt and src share B (got {B}, {src.shape[0]})")
    k = min(3, S)
    idx = torch.empty((B, N, k), dtype=I64, device=tgt.device)
    weight = torch.empty((B, N, k), dtype=torch.float32, device=tgt.device)
    check(_lib.load().vt_three_nn(dev_ptr(tgt, "tgt"), B, N, dev_ptr(src, "src"), S, dev_ptr(idx, "idx", I64), dev_ptr(weight, "weight"),
                                  stream_ptr()), "vt_three_nn")
    return idx, weight
