"""TransformerFusion forward and backward (vt_fusion_*)."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c


FUSION_TENSORS = tuple(n for n, _t in _lib.FusionUnit._fields_)


def _fusion_params(self_attn, cross_attn, C, keep):
    def unit(d):
        u = _lib.FusionUnit()
        for name in FUSION_TENSORS:
            t = _c(d[name].detach())
            keep.append(t)
            setattr(u, name, dev_ptr(t, name).value)
        return u
    prm = _lib.FusionParams()
    prm.d_model, prm.key_dim = C, self_attn["WK"].shape[0]
    prm.self_attn, prm.cross_attn = unit(self_attn), unit(cross_attn)
    return prm


def fusion_plan(B, N, d_model=32, train=False):
    """What a fuser call of ``B`` chunks of ``N`` points launches (vt_fusion_plan: the launchers' own rule, asked without launching
    anything; VTACO_FUSION_SCORE_TERMS counts as it does for them).  ``train``: fusion_fwd_train / fusion_bwd, otherwise fusion_fwd /
    fusion_fwd_ids.  Returns {"form": "full" | "half_pair" | "f8", "proj_tiles", "inorm": "cached" | "streamed", "fwd_row_blocks",
    "bwd_row_blocks", "strided": the names among ("scalev", "epilogue", "add", "bwd_point") of the capped grids whose workgroups
    walk the rest in a loop}; raises VtError where the launchers would refuse the shape."""
    keys = ("form", "proj_tiles", "inorm", "fwd_row_blocks", "bwd_row_blocks", "scalev", "epilogue", "add", "bwd_point")
    out = [ctypes.c_int(0) for _ in keys]
    rc = _lib.load().vt_fusion_plan(int(B), int(N), int(d_model), int(bool(train)), *[ctypes.byref(v) for v in out])
    if rc < 0:
        raise VtError(f"fusion_plan: no fuser call of B={B}, N={N}, d_model={d_model} (code {rc})")
    v = {k: int(x.value) for k, x in zip(keys, out)}
    return {"form": ("full", "half_pair", "f8")[v["form"]], "proj_tiles": v["proj_tiles"], "inorm": ("cached", "streamed")[v["inorm"]],
            "fwd_row_blocks": v["fwd_row_blocks"], "bwd_row_blocks": v["bwd_row_blocks"],
            "strided": tuple(k for k in ("scalev", "epilogue", "add", "bwd_point") if v[k])}


def fusion_fwd(c_img, c, self_attn, cross_attn):
    """TransformerFusion forward, eval mode (vt_fusion_fwd).  ``self_attn`` / ``cross_attn``:
    dicts with the ten tensors of a vt_fusion_unit.

    A chunk of ONE point (N = 1) gives zeros, here and in every other entry of this module: the InstanceNorm over the chunk sees
    z - mean = 0 and a variance of 0, as the oracle's restatement does; torch's own InstanceNorm1d refuses a single element."""
    lib = _lib.load()
    c_img, c = _c(c_img.float()), _c(c.float())
    B, N, C = c.shape
    if tuple(c_img.shape) != (B, N, C):
        raise VtError(f"fusion: c_img {tuple(c_img.shape)} and c {tuple(c.shape)} must match")
    keep = []
    prm = _fusion_params(self_attn, cross_attn, C, keep)
    nbytes = lib.vt_fusion_workspace_bytes_wide(B, N, C)              # (d_model 32, or the generic-width kernels up to 128)
    if nbytes == 0:
        raise VtError(f"fusion: d_model = {C} is not built (32, 64, 96 or 128 with key_feature_dim 64)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=c.device)
    out = torch.empty((B, N, C), dtype=torch.float32, device=c.device)
    check(lib.vt_fusion_fwd(dev_ptr(c_img, "c_img"), dev_ptr(c, "c"), B, N, ctypes.byref(prm),
                            ctypes.c_void_p(ws.data_ptr()), nbytes, dev_ptr(out, "out"), stream_ptr()), "vt_fusion_fwd")
    return out


def fusion_fwd_ids(finger_ids, finger_feats, c, self_attn, cross_attn, chunk_index=None):
    """TransformerFusion forward, eval mode, with the tactile rows by finger id (vt_fusion_fwd_ids): ``finger_ids`` uint8 [rows, N]
    (255 = none), ``finger_feats`` [F, C]; batch element b of ``c`` [B, N, C] reads ids row ``chunk_index[b]`` (int32 [B] on the
    device) or row b.  No [B, N, C] tensor of gathered features exists."""
    lib = _lib.load()
    c = _c(c.float())
    B, N, C = c.shape
    ids, feats = _c(finger_ids), _c(finger_feats.detach().float())
    if ids.dtype != torch.uint8 or ids.dim() != 2 or ids.shape[1] != N or feats.dim() != 2 or feats.shape[1] != C:
        raise VtError(f"fusion_fwd_ids: finger ids must be uint8 [rows,{N}] with a [F,{C}] table (got {tuple(ids.shape)}, {tuple(feats.shape)})")
    if chunk_index is None and ids.shape[0] != B:
        raise VtError(f"fusion_fwd_ids: {ids.shape[0]} id rows for {B} chunks and no chunk_index")
    ci = _c(chunk_index) if chunk_index is not None else None
    if ci is not None and (ci.dtype != torch.int32 or ci.numel() != B):
        raise VtError("fusion_fwd_ids: chunk_index must be int32 [B]")
    keep = []
    prm = _fusion_params(self_attn, cross_attn, C, keep)
    nbytes = lib.vt_fusion_workspace_bytes(B, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=c.device)
    out = torch.empty((B, N, C), dtype=torch.float32, device=c.device)
    check(lib.vt_fusion_fwd_ids(dev_ptr(ids, "finger_ids", torch.uint8), dev_ptr(feats, "finger_feats"), int(feats.shape[0]),
                                dev_ptr(ci, "chunk_index", torch.int32), dev_ptr(c, "c"), B, N, ctypes.byref(prm),
                                ctypes.c_void_p(ws.data_ptr()), nbytes, dev_ptr(out, "out"), stream_ptr()), "vt_fusion_fwd_ids")
    return out


def fusion_fwd_train(c_img, c, self_attn, cross_attn, p_drop=0.0, seed=0):
    """TransformerFusion forward for training (vt_fusion_fwd_train): dropout with probability ``p_drop`` (masks a function
    of ``seed``) and the O(N) state the backward needs.  Returns (out [B,N,C], saved: opaque uint8 tensor)."""
    lib = _lib.load()
    c_img, c = _c(c_img.float()), _c(c.float())
    B, N, C = c.shape
    if tuple(c_img.shape) != (B, N, C):
        raise VtError(f"fusion: c_img {tuple(c_img.shape)} and c {tuple(c.shape)} must match")
    keep = []
    prm = _fusion_params(self_attn, cross_attn, C, keep)
    nbytes, sbytes = lib.vt_fusion_workspace_bytes_wide(B, N, C), lib.vt_fusion_saved_bytes_wide(B, N, C)
    if not nbytes or not sbytes:
        raise VtError(f"fusion_fwd_train: d_model {C} is not built (32, 64, 96, 128)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=c.device)
    saved = torch.empty(sbytes, dtype=torch.uint8, device=c.device)
    out = torch.empty((B, N, C), dtype=torch.float32, device=c.device)
    check(lib.vt_fusion_fwd_train(dev_ptr(c_img, "c_img"), dev_ptr(c, "c"), B, N, ctypes.byref(prm), float(p_drop), int(seed),
                                  ctypes.c_void_p(ws.data_ptr()), nbytes, ctypes.c_void_p(saved.data_ptr()), sbytes,
                                  dev_ptr(out, "out"), stream_ptr()), "vt_fusion_fwd_train")
    return out, saved


def fusion_bwd(d_out, c_img, c, self_attn, cross_attn, saved, p_drop=0.0, seed=0):
    """Backward of ``fusion_fwd_train`` (vt_fusion_bwd).  Returns (d_c_img, d_c, grads_self, grads_cross): the last two are
    dicts name -> gradient tensor with the shapes of the unit's parameters (the self unit's: the sum of its two uses)."""
    lib = _lib.load()
    d_out, c_img, c = _c(d_out.float()), _c(c_img.float()), _c(c.float())
    B, N, C = c.shape
    keep = []
    prm = _fusion_params(self_attn, cross_attn, C, keep)
    grads = _lib.FusionGrads()
    outs = []
    for unit, src in ((grads.self_attn, self_attn), (grads.cross_attn, cross_attn)):
        g = {name: torch.empty_like(src[name], memory_format=torch.contiguous_format) for name in FUSION_TENSORS}
        for name in FUSION_TENSORS:
            setattr(unit, name, dev_ptr(g[name], "grad " + name).value)
        outs.append(g)
    d_c_img, d_c = torch.empty_like(c), torch.empty_like(c)
    nbytes = lib.vt_fusion_bwd_workspace_bytes_wide(B, N, C)
    if not nbytes:
        raise VtError(f"fusion_bwd: d_model {C} is not built (32, 64, 96, 128)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=c.device)
    check(lib.vt_fusion_bwd(dev_ptr(d_out, "d_out"), dev_ptr(c_img, "c_img"), dev_ptr(c, "c"), B, N, ctypes.byref(prm), float(p_drop),
                            int(seed), ctypes.c_void_p(saved.data_ptr()), saved.numel(), ctypes.c_void_p(ws.data_ptr()), nbytes,
                            dev_ptr(d_c_img, "d_c_img"), dev_ptr(d_c, "d_c"), ctypes.byref(grads), stream_ptr()), "vt_fusion_bwd")
    return d_c_img, d_c, outs[0], outs[1]


def fusion_dropout_mask(p_drop, seed, call, which, points, device, d_model=32):
    """The dropout factors (0 or 1/(1-p)) the fusion kernels apply: [points, 64] for which=0, [points, d_model] for which=1."""
    out = torch.empty((points, 64 if which == 0 else d_model), dtype=torch.float32, device=device)
    if d_model == 32:
        check(_lib.load().vt_fusion_dropout_mask(float(p_drop), int(seed), int(call), int(which), int(points), dev_ptr(out, "mask"),
                                                stream_ptr()), "vt_fusion_dropout_mask")
    else:
        check(_lib.load().vt_fusion_dropout_mask_wide(float(p_drop), int(seed), int(call), int(which), int(points), int(d_model),
                                                     dev_ptr(out, "mask"), stream_ptr()), "vt_fusion_dropout_mask_wide")
    return out
