"""Touch session: one touch merged into the id lattice an object keeps (touch.hip; driven by conv_onet/inferencing.py)."""
import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, U8, _c
from .mise import MISE_MAX_N


TOUCH_MAX_ROWS = 254                # rows of a session's feature table: one byte per lattice point, 255 = no row


def touch_workspace(nx, device):
    """The int32 workspace of touch_merge for an nx^3 lattice (vt_touch_workspace_bytes)."""
    nbytes = int(_lib.load().vt_touch_workspace_bytes(int(nx)))
    if nbytes == 0:
        raise VtError(f"touch_workspace: nx must be in [2, {MISE_MAX_N}] (got {nx})")
    return torch.empty(nbytes // 4, dtype=I32, device=device)


def touch_merge(ids, anchors, success, mode, radius, nx, box, row_base, capacity, count=None, changed_ids=None, changed_pts=None,
                n_changed=None, workspace=None):
    """One touch merged into the session's id lattice ``ids`` (u8 [nx^3], in place): where vt_tactile_assign's rule names finger f,
    ``ids[g] = row_base + f``; every other entry is left alone (vt_touch_merge).  Returns (changed_ids int32 [capacity], changed_pts
    f32 [capacity,3], n_changed int32 [1] on the device): the merged points in ascending lattice order; the length may exceed
    ``capacity``, in which case only the first ``capacity`` entries were written.  ``row_base + F > TOUCH_MAX_ROWS`` is refused by
    the entry point before any launch (VtError).  Asynchronous: nothing is read back."""
    anchors = _c(anchors.float())
    F, K = anchors.shape[0], anchors.shape[1]
    dev = anchors.device
    nx, capacity, row_base = int(nx), int(capacity), int(row_base)
    if ids.dtype != U8 or ids.numel() != nx ** 3 or not ids.is_contiguous():
        raise VtError(f"touch_merge: ids must be a contiguous u8 lattice of {nx}^3 points")
    count = torch.full((F,), K, dtype=I32, device=dev) if count is None else _c(count.to(I32))
    success = _c(success.to(U8))
    changed_ids = torch.empty(max(capacity, 1), dtype=I32, device=dev) if changed_ids is None else changed_ids
    changed_pts = torch.empty((max(capacity, 1), 3), dtype=torch.float32, device=dev) if changed_pts is None else changed_pts
    n_changed = torch.empty(1, dtype=I32, device=dev) if n_changed is None else n_changed
    workspace = touch_workspace(nx, dev) if workspace is None else workspace
    if changed_ids.numel() < capacity or changed_pts.numel() < 3 * capacity or n_changed.numel() < 1:
        raise VtError("touch_merge: an output buffer is smaller than the capacity")
    check(_lib.load().vt_touch_merge(dev_ptr(anchors, "anchors"), dev_ptr(count, "count", I32), dev_ptr(success, "success", U8), F, K,
                                     {"nearest": 0, "within": 1}[mode], float(radius), nx, float(box), row_base, dev_ptr(ids, "ids", U8),
                                     dev_ptr(changed_ids, "changed_ids", I32), dev_ptr(changed_pts, "changed_pts"), capacity,
                                     dev_ptr(n_changed, "n_changed", I32), dev_ptr(workspace, "workspace", I32),
                                     workspace.numel() * 4, stream_ptr()), "vt_touch_merge")
    return changed_ids, changed_pts, n_changed
