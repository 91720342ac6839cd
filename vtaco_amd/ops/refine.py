"""The decoder's second-order field jet (vt_decode_jet, vt_decode_jet_composed: csrc/field_jet.hip) and mesh refinement on it
(vt_refine_sample, vt_refine_face_grad, vt_refine_step, vt_refine: csrc/refine.hip) -- the Convolutional Occupancy Networks
generator's ``refine_mesh``.  The 32 / 32 / 5 plain decoder on a feature volume only.  faces are int32 [F,3], vertices float32 [V,3]."""
import ctypes

import numpy as np
import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, I32, _c
from .decode import _cl_storage
from .mesh import _faces, _ws

__all__ = ["JET_FORMS", "decode_jet", "refine_sample", "refine_face_grad", "refine_step", "refine", "refine_accum", "refine_blobs", "refine_check"]

JET_FORMS = ("fused", "composed")
# the form ``refine`` and ``decode_jet`` take unless told: the one tools/bench_refine.py measured faster (profiles/refine_bench.json)
JET_FORM = "fused"


def _form(form):
    form = JET_FORM if form is None else form
    if form not in JET_FORMS:
        raise VtError(f"jet form must be one of {JET_FORMS} (got {form!r})")
    return form


def refine_check(decoder):
    """VtError unless the jet kernels cover ``decoder``: LocalDecoder at hidden 32, c_dim 32, 5 ReLU blocks, bilinear.  Touches no device."""
    if hasattr(decoder, "fuser"):
        raise VtError("refine: the attention decoder is not covered (TransformerFusion couples the points of a chunk: the field at the "
                      "face points is not a function of each point alone)")
    if type(decoder).__name__ == "LocalPointDecoder":
        raise VtError("refine: the PointConv baseline is not covered (its features are sampled from a point cloud, not a volume)")
    shape = (getattr(decoder, "hidden_size", None), getattr(decoder, "c_dim", None), getattr(decoder, "n_blocks", None))
    if shape != (32, 32, 5) or getattr(decoder, "_wide", True):
        raise VtError(f"refine: the field jet is built for hidden_size 32, c_dim 32, 5 ReLU blocks, bilinear sampling (got hidden_size / "
                      f"c_dim / n_blocks = {shape}, leaky = {getattr(decoder, 'leaky', None)}, sample_mode = {getattr(decoder, 'sample_mode', None)!r})")


def refine_blobs(decoder):
    """(blob, blob_t) of a decoder ``refine_check`` accepts."""
    refine_check(decoder)
    with torch.no_grad():
        return decoder._blob(), decoder._blob_t()


def _grid(what, grid):
    B, C, D, H, W = grid.shape
    if not (D == H == W):
        raise VtError(f"{what}: the feature grid must be cubic (got {tuple(grid.shape)})")
    return _cl_storage(grid) + (B, C, D)


def decode_jet(grid, blob, blob_t, pts, padding=0.1, form=None):
    """jet [B,N,8] float32 = (f, f_x, f_y, f_z, f_xy, f_xz, f_yz, 0) of the decoder's logit at pts [B,N,3]."""
    lib = _lib.load()
    form = _form(form)
    keep, gptr, B, C, R = _grid("decode_jet", grid)
    pts = _c(pts.float())
    if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] != 3:
        raise VtError(f"decode_jet: pts must be [B,N,3] with B={B} (got {tuple(pts.shape)})")
    N = pts.shape[1]
    jet = torch.empty((B, N, 8), dtype=torch.float32, device=grid.device)
    if N == 0:
        return jet
    if form == "fused":
        check(lib.vt_decode_jet(gptr, B, R, C, dev_ptr(pts, "pts"), N, dev_ptr(blob, "blob"), dev_ptr(blob_t, "blob_t"), float(padding),
                                dev_ptr(jet, "jet"), stream_ptr()), "vt_decode_jet")
    else:
        wsb = lib.vt_decode_jet_composed_workspace_bytes(B, N)
        ws = _ws(wsb, grid.device)
        check(lib.vt_decode_jet_composed(gptr, B, R, C, dev_ptr(pts, "pts"), N, dev_ptr(blob, "blob"), dev_ptr(blob_t, "blob_t"),
                                         float(padding), dev_ptr(jet, "jet"), ctypes.c_void_p(ws.data_ptr()), wsb, stream_ptr()),
              "vt_decode_jet_composed")
    return jet


def _mesh(what, verts, faces):
    faces = _faces(what, faces, verts)
    if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise VtError(f"{what}: vertices must be float32 [V,3] with V >= 1 (got {verts.dtype} {tuple(verts.shape)})")
    return _c(verts), faces


def _eps(what, eps, F, dev):
    if eps is None:
        return None
    eps = _c(eps.to(dev).float())
    if tuple(eps.shape) != (F, 3):
        raise VtError(f"{what}: eps must be [F,3] = [{F},3] (got {tuple(eps.shape)})")
    return eps


def refine_sample(verts, faces, eps=None, seed=0, step=0):
    """(eps [F,3], pts [F,3]): one point per face, ``sum_i eps_i v_i``; eps as given, or drawn on the device as
    Dirichlet(1/2,1/2,1/2) from a counter hash of (seed, step, face) -- no state, equal bits in any launch order."""
    verts, faces = _mesh("refine_sample", verts, faces)
    F = faces.shape[0]
    given = _eps("refine_sample", eps, F, verts.device)
    out = given if given is not None else torch.empty((F, 3), dtype=torch.float32, device=verts.device)
    pts = torch.empty((F, 3), dtype=torch.float32, device=verts.device)
    check(_lib.load().vt_refine_sample(dev_ptr(verts, "verts"), verts.shape[0], dev_ptr(faces, "faces", I32), F, dev_ptr(given, "eps"),
                                       int(seed), int(step), dev_ptr(out, "eps"), dev_ptr(pts, "pts"), stream_ptr()), "vt_refine_sample")
    return out, pts


def refine_accum(V, device):
    """The zeroed fixed-point accumulator of ``refine_face_grad`` / ``refine_step`` for V vertices."""
    return torch.zeros(_lib.load().vt_refine_accum_bytes(V) // 8, dtype=torch.int64, device=device)


def refine_face_grad(verts, faces, eps, jet, threshold, normal_weight=0.01, accum=None):
    """(terms [F,2], accum): the per-face loss terms ((sigmoid(f) - threshold)^2, |n_face - n_target|^2) and the vertex gradient of
    ``mean(target) + normal_weight mean(normal)`` added into ``accum`` (``refine_accum``; made here when None) as exact fixed-point
    sums: ``refine_step`` turns them into float32."""
    verts, faces = _mesh("refine_face_grad", verts, faces)
    V, F = verts.shape[0], faces.shape[0]
    eps = _eps("refine_face_grad", eps, F, verts.device)
    jet = _c(jet.float()).reshape(-1, 8)
    if eps is None or jet.shape[0] != F:
        raise VtError(f"refine_face_grad: eps [F,3] and jet [F,8] are required (F = {F}, jet {tuple(jet.shape)})")
    if accum is None:
        accum = refine_accum(V, verts.device)
    terms = torch.empty((F, 2), dtype=torch.float32, device=verts.device)
    check(_lib.load().vt_refine_face_grad(dev_ptr(verts, "verts"), V, dev_ptr(faces, "faces", I32), F, dev_ptr(eps, "eps"), dev_ptr(jet, "jet"),
                                          float(threshold), float(normal_weight), dev_ptr(terms, "terms"),
                                          ctypes.c_void_p(accum.data_ptr()), accum.numel() * 8, stream_ptr()), "vt_refine_face_grad")
    return terms, accum


def refine_step(verts, accum, sq, lr=1e-4, alpha=0.99, eps=1e-8):
    """One RMSprop update IN PLACE on ``verts`` [V,3] and ``sq`` [V,3] from the sums in ``accum``, which it zeroes.  Returns the
    float32 gradient [V,3] it applied."""
    if verts.dtype != torch.float32 or not verts.is_contiguous() or sq.dtype != torch.float32 or not sq.is_contiguous() or sq.shape != verts.shape:
        raise VtError("refine_step: verts and sq must be contiguous float32 [V,3] tensors of one shape (they are updated in place)")
    V = verts.shape[0]
    grad = torch.empty((V, 3), dtype=torch.float32, device=verts.device)
    check(_lib.load().vt_refine_step(dev_ptr(verts, "verts"), V, ctypes.c_void_p(accum.data_ptr()), accum.numel() * 8, dev_ptr(sq, "sq"),
                                     float(lr), float(alpha), float(eps), dev_ptr(grad, "grad"), stream_ptr()), "vt_refine_step")
    return grad


def refine(verts, faces, grid, decoder, steps, threshold, padding, eps=None, seed=0, lr=1e-4, normal_weight=0.01, return_losses=False,
           sampler="device", form=None):
    """``steps`` RMSprop iterations (torch's defaults, lr ``lr``) on a copy of ``verts`` against the decoder's field on ``grid``
    [1,32,R,R,R]: sample -> jet -> face gradient -> step, enqueued in full on the current stream with no host read.

    eps      None: drawn per step -- ``sampler='device'`` by the counter hash of (seed, step, face), ``sampler='numpy'`` by
             ``np.random.dirichlet((0.5, 0.5, 0.5), size=F)`` from numpy's global generator, once per step, uploaded (as upstream).
             A tensor [steps,F,3] (or [F,3] for one step): the weights of every step.
    Returns the refined vertices [V,3] float32 -- with ``return_losses`` also the per-face loss terms [steps,F,2] of every step
    (target, normal; before that step's update)."""
    lib = _lib.load()
    form = _form(form)
    if sampler not in ("device", "numpy"):
        raise VtError(f"refine: sampler must be 'device' or 'numpy' (got {sampler!r})")
    steps = int(steps)
    if steps < 0:
        raise VtError(f"refine: steps must be >= 0 (got {steps})")
    blob, blob_t = refine_blobs(decoder)
    verts, faces = _mesh("refine", verts, faces)
    keep, gptr, B, C, R = _grid("refine", grid)
    if B != 1:
        raise VtError(f"refine: one scene at a time (got a grid batch of {B})")
    V, F = verts.shape[0], faces.shape[0]
    dev = verts.device
    out = verts.clone()
    terms = torch.empty((steps, F, 2), dtype=torch.float32, device=dev) if return_losses else None
    if steps == 0:
        return (out, terms) if return_losses else out
    if eps is not None:
        eps = eps.to(dev).float()
        eps = eps.reshape(1, F, 3) if eps.dim() == 2 else eps
        if tuple(eps.shape) != (steps, F, 3):
            raise VtError(f"refine: eps must be [steps,F,3] = [{steps},{F},3] (got {tuple(eps.shape)})")
        eps = _c(eps)
    composed = 1 if form == "composed" else 0
    wsb = lib.vt_refine_workspace_bytes(V, F, composed)
    ws = _ws(wsb, dev)
    sq = torch.zeros((V, 3), dtype=torch.float32, device=dev)
    st = stream_ptr()

    def run(n, first, given, tslice):
        check(lib.vt_refine(gptr, R, C, dev_ptr(out, "verts"), V, dev_ptr(faces, "faces", I32), F, dev_ptr(blob, "blob"),
                            dev_ptr(blob_t, "blob_t"), float(padding), float(threshold), float(normal_weight), float(lr), n, int(seed),
                            first, dev_ptr(given, "eps"), dev_ptr(sq, "sq"), composed, dev_ptr(tslice, "terms"),
                            ctypes.c_void_p(ws.data_ptr()), wsb, st), "vt_refine")

    if eps is None and sampler == "device":
        run(steps, 0, None, terms)
    else:
        for it in range(steps):
            if eps is not None:
                given = eps[it]
            else:                                                     # upstream's draw, from numpy's global generator
                given = torch.from_numpy(np.random.dirichlet((0.5, 0.5, 0.5), size=F).astype(np.float32)).to(dev)
            run(1, it, given, None if terms is None else terms[it])
    return (out, terms) if return_losses else out
