"""Multiresolution isosurface extraction: one refinement step (mise.hip; driven by vtaco_amd/mise.py)."""
import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, U8, _c


MISE_MAX_N = 513                    # VT_MISE_MAX_N


def mise_lattice(n, box, device, want_ids=True):
    """(ids int32 [n^3] or None, pts f32 [n^3,3]) of the whole n^3 lattice, coordinates as the decode kernels' lattice computes them
    (vt_mise_lattice)."""
    n = int(n)
    if not 2 <= n <= MISE_MAX_N:
        raise VtError(f"mise_lattice: n must be in [2, {MISE_MAX_N}] (got {n})")
    pts = torch.empty((n ** 3, 3), dtype=torch.float32, device=device)
    ids = torch.empty(n ** 3, dtype=I32, device=device) if want_ids else None
    check(_lib.load().vt_mise_lattice(n, float(box), dev_ptr(ids, "ids", I32), dev_ptr(pts, "pts"), stream_ptr()), "vt_mise_lattice")
    return ids, pts


def mise_refine(coarse, level, box, capacity, coarse_known=None, fine=None, known=None, qids=None, qpts=None, count=None, active=None):
    """One refinement step (vt_mise_refine) of the coarse value grid [nc]^3 whose known points ``coarse_known`` (u8 [nc]^3; None: all)
    marks: the fine grid [nf]^3 (nf = 2 nc - 1) holding the nearest-coarse fill, its known mask (u8: the even points whose coarse
    point was known; None when ``known=False``), and the query list
    (ids int32 [capacity], pts [capacity,3]) with its length in the device word ``count`` (int32 [1]; may exceed ``capacity``, in
    which case only the first ``capacity`` entries were written).  Asynchronous: nothing is read back."""
    if coarse.dim() != 3 or not (coarse.shape[0] == coarse.shape[1] == coarse.shape[2]) or not coarse.is_contiguous():
        raise VtError("mise_refine: the coarse grid must be a contiguous cube [nc,nc,nc]")
    nc = int(coarse.shape[0])
    nf = 2 * nc - 1
    if not 2 <= nc or nf > MISE_MAX_N:
        raise VtError(f"mise_refine: the fine grid {nf}^3 is outside [3, {MISE_MAX_N}]^3")
    dev = coarse.device
    capacity = int(capacity)
    fine = torch.empty((nf, nf, nf), dtype=torch.float32, device=dev) if fine is None else fine
    if known is None:
        known = torch.empty((nf, nf, nf), dtype=U8, device=dev)
    elif known is False:
        known = None
    qids = torch.empty(max(capacity, 1), dtype=I32, device=dev) if qids is None else qids
    qpts = torch.empty((max(capacity, 1), 3), dtype=torch.float32, device=dev) if qpts is None else qpts
    count = torch.empty(1, dtype=I32, device=dev) if count is None else count
    active = torch.empty((nc - 1) ** 3, dtype=U8, device=dev) if active is None else active
    if (fine.numel() != nf ** 3 or (known is not None and known.numel() != nf ** 3) or qids.numel() < capacity
            or qpts.numel() < 3 * capacity or active.numel() < (nc - 1) ** 3 or count.numel() < 1):
        raise VtError("mise_refine: an output buffer is smaller than the step needs")
    if coarse_known is not None and (coarse_known.numel() != nc ** 3 or not coarse_known.is_contiguous()):
        raise VtError("mise_refine: coarse_known must be a contiguous u8 [nc,nc,nc]")
    check(_lib.load().vt_mise_refine(dev_ptr(coarse, "coarse"), dev_ptr(coarse_known, "coarse_known", U8), nc, float(level), float(box), dev_ptr(active, "active", U8),
                                     dev_ptr(fine, "fine"), dev_ptr(known, "known", U8), dev_ptr(qids, "qids", I32), dev_ptr(qpts, "qpts"),
                                     capacity, dev_ptr(count, "count", I32), stream_ptr()), "vt_mise_refine")
    return fine, known, qids, qpts, count


def mise_scatter(fine, ids, vals, known=None):
    """fine[ids[i]] = vals[i] (and known[ids[i]] = 1) for every entry of the list (vt_mise_scatter)."""
    m = int(ids.numel())
    if int(vals.numel()) != m:
        raise VtError(f"mise_scatter: {m} ids but {int(vals.numel())} values")
    vals = _c(vals.detach().float().reshape(-1))
    check(_lib.load().vt_mise_scatter(dev_ptr(_c(ids.reshape(-1)), "ids", I32), dev_ptr(vals, "vals"), m, dev_ptr(fine, "fine"),
                                      int(fine.numel()), dev_ptr(known, "known", U8), stream_ptr()), "vt_mise_scatter")
    return fine
