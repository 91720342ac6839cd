"""Marching cubes on the device (vt_mc_*)."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c

# what ``from .mc import *`` hands to ``vtaco_amd.ops``; ``mc_emit_normals`` and ``marching_cubes_normals`` are reached as ``ops.mc.*``
__all__ = ["mc_count", "mc_count_notify", "mc_echo_slot", "mc_echo_release", "mc_count_echo", "mc_echo_arm", "mc_emit", "marching_cubes"]


_mc_ws_cache = {}


def _mc_workspace(vol):
    lib = _lib.load()
    n0, n1, n2 = vol.shape
    nbytes = lib.vt_mc_workspace_bytes(n0, n1, n2)
    if nbytes == 0:
        raise ValueError("Input array must be at least 2x2x2.")
    key = (vol.device, nbytes)
    ws = _mc_ws_cache.get(key)
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
        _mc_ws_cache.clear()
        _mc_ws_cache[key] = ws
    return ws, nbytes


def mc_count(vol, level=None):
    """Phase 1 of marching cubes (vt_mc_count): classify + scan into the workspace.  Asynchronous
    and graph-capturable; returns the workspace tensor."""
    if vol.dim() != 3:
        raise VtError("marching_cubes: volume must be [n0,n1,n2]")
    if not vol.is_contiguous():
        raise VtError("marching_cubes: volume must be contiguous")
    ws, nbytes = _mc_workspace(vol)
    n0, n1, n2 = vol.shape
    check(_lib.load().vt_mc_count(dev_ptr(vol, "vol"), n0, n1, n2, 0.0 if level is None else float(level), int(level is None),
                                  ctypes.c_void_p(ws.data_ptr()), nbytes, stream_ptr()), "vt_mc_count")
    return ws


def mc_count_notify(vol, level=None):
    """``mc_count`` whose scan kernel also writes the counts into a page-locked host slot (vt_mc_count_notify): returns
    (workspace, token); hand the token to ``mc_emit`` -- the count read then needs no copy command between the count and the emit
    kernels.  Not for graph capture: the slot's sequence number is baked into the scan kernel's arguments, so a replay would write
    a number nobody waits for; captured scenes use ``mc_count``."""
    if vol.dim() != 3 or not vol.is_contiguous():
        raise VtError("marching_cubes: volume must be a contiguous [n0,n1,n2] tensor")
    ws, nbytes = _mc_workspace(vol)
    n0, n1, n2 = vol.shape
    tok = ctypes.c_int()
    check(_lib.load().vt_mc_count_notify(dev_ptr(vol, "vol"), n0, n1, n2, 0.0 if level is None else float(level), int(level is None),
                                         ctypes.c_void_p(ws.data_ptr()), nbytes, stream_ptr(), ctypes.byref(tok)), "vt_mc_count_notify")
    return ws, tok.value


def mc_echo_slot():
    """A page-locked slot for the counts of a CAPTURED scene (vt_mc_echo_slot): make it outside the capture, hand it to
    ``mc_count_echo`` inside, ``mc_echo_arm`` it before every replay and pass it to ``mc_emit(echo=...)``."""
    tok = ctypes.c_int()
    check(_lib.load().vt_mc_echo_slot(ctypes.byref(tok)), "vt_mc_echo_slot")
    return tok.value


def mc_echo_release(slot):
    """Hand a slot back (vt_mc_echo_release) once the graph that echoes into it is gone; the next ``mc_echo_slot`` reuses it."""
    check(_lib.load().vt_mc_echo_release(int(slot)), "vt_mc_echo_release")


def mc_count_echo(vol, level, slot):
    """``mc_count`` for graph capture whose scan kernel echoes the slot's current number behind the counts into the slot's page-locked
    header (vt_mc_count_echo): the replayed scene needs no copy command between the count and the emit kernels."""
    if vol.dim() != 3 or not vol.is_contiguous():
        raise VtError("marching_cubes: volume must be a contiguous [n0,n1,n2] tensor")
    ws, nbytes = _mc_workspace(vol)
    n0, n1, n2 = vol.shape
    check(_lib.load().vt_mc_count_echo(dev_ptr(vol, "vol"), n0, n1, n2, 0.0 if level is None else float(level), int(level is None),
                                       ctypes.c_void_p(ws.data_ptr()), nbytes, stream_ptr(), int(slot)), "vt_mc_count_echo")
    return ws


def mc_echo_arm(slot):
    """A fresh number into the slot (vt_mc_echo_arm): before every replay of the graph that holds ``mc_count_echo``."""
    check(_lib.load().vt_mc_echo_arm(int(slot)), "vt_mc_echo_arm")


_mc_guess = {}          # volume shape -> (vertex, face) capacity that covered the last extraction there


def mc_emit(vol, ws, rescale=None, capacity=None, token=None, echo=None):
    """Phase 2 (vt_mc_emit + vt_mc_read_counts).  With ``capacity=(V,F)`` nothing is read back
    (no stream sync; the counts stay in the workspace).  Otherwise the outputs are sized by the
    counts, which costs one host read: after the first extraction of a shape the emit kernels are
    launched SPECULATIVELY into buffers 25 % larger than the previous result before that read, so
    the read is the only synchronisation of the call; if the surface outgrew the guess the emit is
    repeated at the exact size (the kernels never write past their capacity)."""
    lib = _lib.load()
    if capacity is not None and (token is not None or echo is not None):
        raise VtError("mc_emit: a token (mc_count_notify) is handed back by reading the counts; with capacity= nothing is read -- "
                      "use mc_count for fixed-capacity extraction")
    n0, n1, n2 = vol.shape
    st = stream_ptr()
    wp = ctypes.c_void_p(ws.data_ptr())
    shift, scale = rescale if rescale is not None else (0.0, 1.0)

    def emit(cap_v, cap_f):
        verts = torch.empty((cap_v, 3), dtype=torch.float32, device=vol.device)
        faces = torch.empty((cap_f, 3), dtype=torch.int32, device=vol.device)
        check(lib.vt_mc_emit(dev_ptr(vol, "vol"), n0, n1, n2, wp, dev_ptr(verts, "verts"), cap_v,
                             dev_ptr(faces, "faces", torch.int32), cap_f, int(rescale is not None), shift, scale, st),
              "vt_mc_emit")
        return verts, faces

    if capacity is not None:
        verts, faces = emit(*capacity)
        return verts, faces, ws          # counts stay on the device: ws[8:16] = (nverts, nfaces) int32
    key = (vol.device.index, n0, n1, n2)
    guess = _mc_guess.get(key)
    # the copy of the counts is queued FIRST (it needs the classify / scan launches only) and waited for by its own event, so
    # the speculative emit kernels run under that wait instead of in front of the copy
    tok = ctypes.c_int(-1 if token is None else token)
    if token is None and echo is None:
        check(lib.vt_mc_read_counts_begin(wp, st, ctypes.byref(tok)), "vt_mc_read_counts_begin")
    nv, nf, lvl = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    try:
        spec = emit(*guess) if guess is not None else None
    finally:                             # the token is handed back whatever the emit did (sixteen exist)
        if echo is not None:             # (a captured scene's slot, armed before the replay: the scan kernel echoes its number)
            rc = lib.vt_mc_echo_wait(int(echo), st, ctypes.byref(nv), ctypes.byref(nf), ctypes.byref(lvl))
        else:
            rc = lib.vt_mc_read_counts_end(tok.value, ctypes.byref(nv), ctypes.byref(nf), ctypes.byref(lvl))
    check(rc, "vt_mc_read_counts_end")
    if nv.value == 0:
        raise RuntimeError("No surface found at the given iso value.")
    _mc_guess[key] = (nv.value + nv.value // 4 + 1024, nf.value + nf.value // 4 + 1024)
    if spec is not None and nv.value <= guess[0] and nf.value <= guess[1]:
        return spec[0][:nv.value], spec[1][:nf.value], lvl.value
    verts, faces = emit(nv.value, nf.value)
    return verts, faces, lvl.value


def marching_cubes(vol, level=None, rescale=None, capacity=None):
    """Lewiner marching cubes of a device volume [n0,n1,n2] (vt_mc_count/emit).

    Returns (verts f32 [V,3] in array-axis order, faces i32 [F,3], level) as device
    tensors, numbered exactly as skimage.measure.marching_cubes(vol,
    gradient_direction='ascent') numbers them.  ``rescale=(shift, scale)`` fuses the
    reference's `v -= shift; v *= scale` (generation.py:271-272).  ``capacity=(V,F)``
    skips the host read of the counts (no stream sync); otherwise the counts are read
    back once to size the outputs.  Raises RuntimeError('No surface found ...') like
    skimage when the level misses the data.
    """
    if vol.dim() != 3:
        raise VtError("marching_cubes: volume must be [n0,n1,n2]")
    vol = _c(vol)
    if capacity is not None or torch.cuda.is_current_stream_capturing():
        return mc_emit(vol, mc_count(vol, level), rescale, capacity)
    ws, tok = mc_count_notify(vol, level)            # the counts arrive in a page-locked slot: no copy between count and emit
    return mc_emit(vol, ws, rescale, None, token=tok)


def mc_emit_normals(vol, ws, n_verts):
    """The normals [V,3] and values [V] of the vertices ``mc_emit`` numbered (vt_mc_emit_normals): one asynchronous launch behind
    ``mc_count`` / ``mc_emit`` on the same volume and workspace.  ``n_verts``: the rows to write (the vertex count or a capacity)."""
    n0, n1, n2 = vol.shape
    n_verts = int(n_verts)
    normals = torch.empty((n_verts, 3), dtype=torch.float32, device=vol.device)
    values = torch.empty(n_verts, dtype=torch.float32, device=vol.device)
    check(_lib.load().vt_mc_emit_normals(dev_ptr(vol, "vol"), n0, n1, n2, ctypes.c_void_p(ws.data_ptr()), dev_ptr(normals, "normals"),
                                         dev_ptr(values, "values"), n_verts, stream_ptr()), "vt_mc_emit_normals")
    return normals, values


def marching_cubes_normals(vol, level=None, rescale=None):
    """``marching_cubes`` with the other half of scikit-image's result: (verts, faces, normals f32 [V,3], values f32 [V], level), as
    ``measure.marching_cubes(vol, level, gradient_direction='ascent')`` returns them (reference generation.py:270).  The normals are
    unit, in array-axis order like the vertices, (0,0,0) where scikit-image's sum is zero or not finite; ``rescale`` is a uniform scale
    and leaves them as they are.  One extra launch behind the emit; the count is read back once, as in ``marching_cubes``."""
    if vol.dim() != 3:
        raise VtError("marching_cubes: volume must be [n0,n1,n2]")
    vol = _c(vol)
    if torch.cuda.is_current_stream_capturing():
        raise VtError("marching_cubes_normals: reads the vertex count back; inside a capture use mc_count / mc_emit with a capacity "
                      "and mc_emit_normals")
    ws, tok = mc_count_notify(vol, level)
    verts, faces, lvl = mc_emit(vol, ws, rescale, None, token=tok)
    normals, values = mc_emit_normals(vol, ws, verts.shape[0])
    return verts, faces, normals, values, lvl
