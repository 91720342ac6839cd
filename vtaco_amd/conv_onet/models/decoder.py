"""Implicit occupancy decoders (drop-in for reference src/conv_onet/models/decoder.py).

Same constructor kwargs, parameter names and call signatures as the reference's
``LocalDecoder`` (decoder.py:9-161); the arithmetic -- coordinate normalisation,
trilinear sampling of the feature grid, fc_p, 5 x (fc_c + ResnetBlockFC), fc_out --
is ONE fused HIP kernel reached through the C ABI (``vt_decode_fwd``).  There is
no torch fallback: CPU tensors raise.
"""
from __future__ import annotations

import os

import torch
from torch import nn

from ... import ops
from ..._lib import VtError
from ...layers import ResnetBlockFC
from ...transformer_fusion import TransformerFusion


class _DecodeFn(torch.autograd.Function):
    """Differentiable fused decode: forward = vt_decode_fwd (saving activations), backward =
    vt_decode_bwd + vt_decode_wgrad.  Gradients flow to the feature grid, c_img and every
    decoder parameter; not to the query points (the reference never reads p.grad either,
    SURVEY.md section 8a row A14)."""

    @staticmethod
    def forward(ctx, dec, p, grid, c_img, *params):
        img = c_img is not None
        B, N = p.shape[0], p.shape[1]
        save = ops.decode_save_buffer(B * N, grid.device)
        out = ops.decode_fwd(grid, dec._blob(img=img), pts=p, c_img=c_img, padding=dec.padding, save=save)
        ctx.dec, ctx.img, ctx.save, ctx.grid_shape = dec, img, save, tuple(grid.shape)
        ctx.p, ctx.c_img = p.detach(), (c_img.detach() if img else None)
        ctx.need_grid = grid.requires_grad
        return out

    @staticmethod
    def backward(ctx, grad_out):
        dec, img = ctx.dec, ctx.img
        ggrid, gimg, flat = ops.decode_bwd(ctx.grid_shape, dec._blob_t(img=img), grad_out, ctx.save, pts=ctx.p,
                                           with_c_img=img, c_img=ctx.c_img, padding=dec.padding,
                                           want_grid_grad=ctx.need_grid)
        g = ops.split_decoder_grads(flat, 3 + dec.c_dim if img else 3)
        grads = []
        for name in dec._param_order(img):
            key, idx = name
            grads.append(g[key] if idx is None else g[key][idx])
        return (None, None, ggrid, gimg, *grads)


class _DecodeContactFn(torch.autograd.Function):
    """forward_contact, differentiable (decoder.py:105-133; training.py:896-948): the fused decode with both heads
    (vt_decode_fwd with out2 and the saved activations), backward = vt_decode_bwd_contact + vt_decode_wgrad_contact."""

    @staticmethod
    def forward(ctx, dec, p, grid, *params):
        B, N = p.shape[0], p.shape[1]
        save = ops.decode_save_buffer(B * N, grid.device)
        out, out2 = ops.decode_fwd(grid, dec._blob(contact=True), pts=p, padding=dec.padding, save=save, want_contact=True)
        ctx.dec, ctx.save, ctx.grid_shape, ctx.p, ctx.need_grid = dec, save, tuple(grid.shape), p.detach(), grid.requires_grad
        return out, out2

    @staticmethod
    def backward(ctx, grad_out, grad_out2):
        dec = ctx.dec
        ggrid, _, flat = ops.decode_bwd(ctx.grid_shape, dec._blob_t(contact=True), grad_out, ctx.save, pts=ctx.p,
                                        padding=dec.padding, want_grid_grad=ctx.need_grid, grad_out2=grad_out2)
        g = ops.split_decoder_grads(flat, 3)
        grads = [g[key] if idx is None else g[key][idx] for key, idx in dec._param_order(False)]
        return (None, None, ggrid, *grads, g["fc_out_contact.weight"], g["fc_out_contact.bias"])


class _DecodeWideFn(torch.autograd.Function):
    """The decoder at the shapes beyond 32 / 32 (hidden_size / c_dim multiples of 32 up to 256, `leaky`, 'nearest'), differentiable:
    forward = vt_decode_fwd_wide_train (keeps every layer's input), backward = vt_decode_bwd_wide (data gradients on transposed
    weight fragments, the grid gradient by atomics) + vt_rows_wgrad per layer.  Gradients to the feature grid, c_img and every
    parameter; with ``contact`` both heads (forward_contact)."""

    @staticmethod
    def forward(ctx, dec, p, grid, c_img, contact, *params):
        img = c_img is not None
        nearest = dec.sample_mode == 'nearest'
        out, out2, save = ops.decode_fwd_wide_train(grid, dec._blob(img=img, contact=contact), p, c_img, dec.hidden_size, dec.n_blocks,
                                                    dec.leaky, nearest, dec.padding, want_contact=contact)
        ctx.dec, ctx.img, ctx.contact, ctx.save, ctx.grid_shape = dec, img, contact, save, tuple(grid.shape)
        ctx.p, ctx.c_img = p.detach(), (c_img.detach() if img else None)
        ctx.need_grid = grid.requires_grad
        ctx.need_img = img and c_img.requires_grad
        return (out, out2) if contact else out

    @staticmethod
    def backward(ctx, grad_out, grad_out2=None):
        dec, img = ctx.dec, ctx.img
        first = dec.fc_p_img if img else dec.fc_p
        blob_t = ops.pack_decoder_wide_t(first.weight, [l.weight for l in dec.fc_c], [(b.fc_0.weight, b.fc_1.weight) for b in dec.blocks],
                                         dec.fc_out.weight, dec.fc_out_contact.weight if ctx.contact else None)
        if ctx.contact and grad_out2 is None:
            grad_out2 = torch.zeros_like(grad_out)
        ggrid, gimg, g = ops.decode_bwd_wide(ctx.grid_shape, blob_t, grad_out, ctx.save, ctx.p, dec.hidden_size, dec.n_blocks, dec.leaky,
                                             dec.sample_mode == 'nearest', dec.padding, c_img=ctx.c_img, want_grid_grad=ctx.need_grid,
                                             grad_out2=grad_out2 if ctx.contact else None)
        grads = [g[key] if idx is None else g[key][idx] for key, idx in dec._param_order(img)]
        if ctx.contact:
            grads += [g["fc_out_contact.weight"], g["fc_out_contact.bias"]]
        return (None, None, ggrid, gimg if ctx.need_img else None, None, *grads)


class _SampleGridFn(torch.autograd.Function):
    """Trilinear sampling alone (vt_sample_grid / vt_sample_grid_bwd), differentiable in the grid."""

    @staticmethod
    def forward(ctx, grid, p, padding):
        ctx.shape, ctx.p, ctx.padding = tuple(grid.shape), p.detach(), padding
        return ops.sample_grid(grid, p, padding)

    @staticmethod
    def backward(ctx, grad_feat):
        return ops.sample_grid_bwd(ctx.shape, ctx.p, grad_feat, ctx.padding), None, None


class _SamplePlanesFn(torch.autograd.Function):
    """The canonical planes' samples added onto ``base`` (vt_sample_planes / vt_sample_planes_bwd), differentiable in every plane and
    in ``base`` (whose gradient is the output's).  ``keys``: the planes' names, in the order the tensors follow."""

    @staticmethod
    def forward(ctx, p, padding, nearest, base, keys, *planes):
        ctx.keys, ctx.shape, ctx.p, ctx.padding, ctx.nearest = keys, tuple(planes[0].shape), p.detach(), padding, nearest
        ctx.has_base = base is not None
        # (the planes are summed onto a copy: the grid's sample stays what its own autograd node returned)
        return ops.planes.sample_planes(dict(zip(keys, planes)), p, padding, base=None if base is None else base.detach().clone(),
                                        nearest=nearest)

    @staticmethod
    def backward(ctx, grad_feat):
        grads = ops.planes.sample_planes_bwd(ctx.keys, ctx.shape, ctx.p, grad_feat, ctx.padding, ctx.nearest)
        return (None, None, None, grad_feat if ctx.has_base else None, None, *[grads[k] for k in ctx.keys])


class _DecodeMlpFn(torch.autograd.Function):
    """The conditioned MLP on given features (vt_decode_mlp_fwd_train; backward vt_decode_mlp_bwd +
    vt_decode_wgrad): gradients to the features and to every decoder parameter (fc_p form)."""

    @staticmethod
    def forward(ctx, dec, p, c, *params):
        out, save = ops.decode_mlp_fwd_train(c, dec._blob(), p)
        ctx.dec, ctx.save, ctx.p = dec, save, p.detach()
        return out

    @staticmethod
    def backward(ctx, grad_out):
        dec = ctx.dec
        grad_c, flat = ops.decode_mlp_bwd(dec._blob_t(img=False), grad_out, ctx.save, ctx.p, dec.c_dim)
        g = ops.split_decoder_grads(flat, 3)
        grads = []
        for key, idx in dec._param_order(False):
            grads.append(g[key] if idx is None else g[key][idx])
        return (None, None, grad_c, *grads)


class _DecodeMlpWideFn(torch.autograd.Function):
    """_DecodeMlpFn at the widths beyond 32 / 32 (vt_decode_mlp_fwd_wide_train; backward vt_decode_mlp_bwd_wide + vt_rows_wgrad per
    layer): gradients to the given features and to every decoder parameter (fc_p form)."""

    @staticmethod
    def forward(ctx, dec, p, c, *params):
        out, save = ops.decode_mlp_fwd_wide_train(c, dec._blob(), p, dec.hidden_size, dec.n_blocks, dec.leaky)
        ctx.dec, ctx.save, ctx.p, ctx.c = dec, save, p.detach(), c.detach()
        return out

    @staticmethod
    def backward(ctx, grad_out):
        dec = ctx.dec
        blob_t = ops.pack_decoder_wide_t(dec.fc_p.weight, [l.weight for l in dec.fc_c], [(b.fc_0.weight, b.fc_1.weight) for b in dec.blocks],
                                         dec.fc_out.weight, None)
        grad_c, g = ops.decode_mlp_bwd_wide(blob_t, grad_out, ctx.save, ctx.p, ctx.c, dec.hidden_size, dec.n_blocks, dec.leaky)
        grads = [g[key] if idx is None else g[key][idx] for key, idx in dec._param_order(False)]
        return (None, None, grad_c, *grads)


class LocalDecoder(nn.Module):
    """Decoder conditioned on a local 3-D feature grid and / or the canonical feature planes ('xz', 'xy', 'yz').

    Args mirror the reference (decoder.py:23-24): dim, c_dim, hidden_size,
    n_blocks, leaky, sample_mode, padding, with_contact.
    """

    def __init__(self, dim=3, c_dim=128, hidden_size=256, n_blocks=5, leaky=False,
                 sample_mode='bilinear', padding=0.1, with_contact=False, **kwargs):
        super().__init__()
        if dim != 3:
            raise VtError("LocalDecoder: only dim=3 is built")
        if sample_mode not in ('bilinear', 'nearest'):
            raise VtError(f"LocalDecoder: sample_mode must be 'bilinear' or 'nearest' (F.grid_sample's modes for 5-D input), got {sample_mode!r}")
        self.c_dim, self.n_blocks, self.hidden_size = c_dim, n_blocks, hidden_size
        # `leaky`: leaky_relu(0.2) in front of the output heads (reference decoder.py:46-49, 157; the blocks stay ReLU).  The shipped
        # shape (32 / 32, relu) runs on the LDS-resident kernels of decode.hip, training included; every other shape -- hidden_size
        # and c_dim multiples of 32 up to 256, e.g. the class defaults 256 / 128 -- on the weight-streaming kernels of
        # decode_wide.hip: vt_decode_fwd_wide (exact f32) or vt_decode_fwd_wide_f16x3 (split-f16 operands, for the half-precision
        # settings of ``precision``), and under autograd vt_decode_fwd_wide_train / vt_decode_bwd_wide / vt_rows_wgrad (_DecodeWideFn)
        self.leaky = bool(leaky)
        self._wide = self.leaky or hidden_size != 32 or c_dim != 32 or sample_mode == 'nearest'
        self.sample_mode, self.padding = sample_mode, padding
        self.fc_c = nn.ModuleList(nn.Linear(c_dim, hidden_size) for _ in range(n_blocks))
        self.fc_p = nn.Linear(dim, hidden_size)
        self.fc_p_img = nn.Linear(dim + c_dim, hidden_size)
        self.blocks = nn.ModuleList(ResnetBlockFC(hidden_size) for _ in range(n_blocks))
        self.fc_out = nn.Linear(hidden_size, 1)
        if with_contact:
            self.fc_out_contact = nn.Linear(hidden_size, 1)
        self._blobs = {}
        # arithmetic of the 16 dense layers on the no-grad paths: "f32" (exact-f32 MFMA), "bf16x3" / "f16x3" (split 16-bit MFMA
        # operands: ~2e-5 / ~1e-6 abs on O(1) logits) or "f16f8" (f16 products + fp8 corrections, lattice slabs only: ~4e-5, the
        # fastest; point queries then run as "f16x3"); training is always "f32"
        self.precision = os.environ.get("VTACO_DECODE_PRECISION", "f32")

    def _point_precision(self):
        return "f16x3" if self.precision == "f16f8" else self.precision

    # -- weights -> MFMA-fragment blob, cached until a parameter changes ---------
    def _blob(self, img=False, contact=False, precision="f32"):
        head2 = (self.fc_out_contact.weight, self.fc_out_contact.bias) if contact else None
        first = self.fc_p_img if img else self.fc_p
        params = [first.weight, first.bias, self.fc_out.weight, self.fc_out.bias]
        for lin, blk in zip(self.fc_c, self.blocks):
            params += [lin.weight, lin.bias, *blk.packed()]
        if head2:
            params += list(head2)
        stamp = tuple((p.data_ptr(), p._version) for p in params)
        if self._wide:
            precision = self._wide_precision(precision)
        hit = self._blobs.get((img, contact, precision))
        if hit is not None and hit[0] == stamp:
            return hit[1]
        blob = ops.pack_decoder(first.weight, first.bias,
                                [(l.weight, l.bias) for l in self.fc_c],
                                [b.packed() for b in self.blocks],
                                (self.fc_out.weight, self.fc_out.bias), head2,
                                out=hit[1] if hit is not None else None, precision=precision)
        self._blobs[(img, contact, precision)] = (stamp, blob)
        return blob

    def _blob_t(self, img=False, contact=False):
        first = self.fc_p_img if img else self.fc_p
        out2 = (self.fc_out_contact.weight, self.fc_out_contact.bias) if contact else None
        return ops.pack_decoder(first.weight, first.bias, [(l.weight, l.bias) for l in self.fc_c],
                                [b.packed() for b in self.blocks], (self.fc_out.weight, self.fc_out.bias), out2,
                                transposed=True)

    def _param_order(self, img):
        """(gradient key, index) for every tensor passed to _DecodeFn, in order."""
        order = [("fc_p.weight", None), ("fc_p.bias", None)]
        for i in range(self.n_blocks):
            order += [("fc_c.weight", i), ("fc_c.bias", i), ("fc_0.weight", i), ("fc_0.bias", i),
                      ("fc_1.weight", i), ("fc_1.bias", i)]
        return order + [("fc_out.weight", None), ("fc_out.bias", None)]

    def _params(self, img):
        first = self.fc_p_img if img else self.fc_p
        ps = [first.weight, first.bias]
        for lin, blk in zip(self.fc_c, self.blocks):
            ps += [lin.weight, lin.bias, *blk.packed()]
        return ps + [self.fc_out.weight, self.fc_out.bias]

    def _wants_grad(self, grid, c_img=None):
        if not torch.is_grad_enabled():
            return False
        return grid.requires_grad or (c_img is not None and c_img.requires_grad) or any(
            p.requires_grad for p in self.parameters())

    def _wide_train(self, p, grid, c_img=None, contact=False):
        """The wide shapes under autograd: _DecodeWideFn (HIP forward and backward)."""
        if not grid.is_cuda:
            raise VtError(f"LocalDecoder: inputs must live on a HIP device (got {grid.device})")
        params = self._params(c_img is not None)
        if contact:
            params = params + [self.fc_out_contact.weight, self.fc_out_contact.bias]
        return _DecodeWideFn.apply(self, p.float(), grid, None if c_img is None else c_img.float(), contact, *params)

    @staticmethod
    def _wide_precision(precision):
        """The kernel of the shapes beyond 32 / 32 for a requested arithmetic: the split-f16 forward (vt_decode_fwd_wide_f16x3) for the
        half-precision forms, the exact-f32 one (vt_decode_fwd_wide) for "f32" and for "bf16x3" (the range guard's way out)."""
        return "wide_f16x3" if precision in ("f16x3", "f16f8", "wide_f16x3") else "wide"

    def _wide_fwd(self, grid, precision=None, **kw):
        wp = self._wide_precision(precision or self._point_precision())
        img = kw.get("c_img") is not None or kw.get("finger_ids") is not None
        return ops.decode_fwd(grid, self._blob(img=img, contact=kw.get("want_contact", False), precision=wp),
                              padding=self.padding, precision=wp,
                              wide=(self.hidden_size, self.n_blocks, self.leaky, self.sample_mode == 'nearest'), **kw)

    @staticmethod
    def _grid_of(c_plane, what="this route"):
        """The feature volume of a grid-only ``c_plane``: the resolver of the routes whose kernels take nothing else."""
        if set(c_plane.keys()) != {'grid'}:
            raise VtError(f"LocalDecoder: {what} takes the 'grid' feature volume alone (got {sorted(c_plane.keys())}): the fused "
                          "decode kernels (vt_decode_fwd*) sample a volume; plane features ('xz','xy','yz') are decoded by "
                          "forward, AttentionDecoder.forward_img and decode_lattice through vt_sample_planes")
        return c_plane['grid']

    @staticmethod
    def _features_of(c_plane):
        """(grid or None, {plane: tensor}) of any non-empty subset of 'grid','xz','xy','yz' (decoder.py:137-146)."""
        keys = set(c_plane.keys())
        if not keys or not keys <= {'grid', 'xz', 'xy', 'yz'}:
            raise VtError(f"LocalDecoder: c_plane must hold a non-empty subset of 'grid','xz','xy','yz' (got {sorted(keys)})")
        return c_plane.get('grid'), {k: c_plane[k] for k in ('xz', 'xy', 'yz') if k in c_plane}

    def _refuse_planes(self, c_plane, what, kernel):
        if set(c_plane.keys()) != {'grid'}:
            raise VtError(f"LocalDecoder.{what} with plane features {sorted(c_plane.keys())} is not built: {kernel}")

    # -- the route through sampled features: grid and / or planes -> c [B,N,C] -> the conditioned MLP on given features -------------
    def _check_nearest_grid(self, grid):
        if grid is not None and self.sample_mode == 'nearest':
            raise VtError("LocalDecoder: 'grid' mixed with planes under sample_mode='nearest' is not built (vt_sample_grid has no "
                          "'nearest' form)")

    def _sample(self, p, grid, planes, lattice=None, prepared=None):
        """c = grid? + xz? + xy? + yz? at the points (or the lattice slab), no autograd: ops.sample_grid, then ops.planes.sample_planes.
        ``prepared``: an ops.planes.Prepared the caller keeps over the calls of one scene (the planes are laid out once)."""
        if not planes:
            return ops.sample_grid(grid, p, self.padding, lattice=lattice)
        self._check_nearest_grid(grid)
        base = ops.sample_grid(grid, p, self.padding, lattice=lattice) if grid is not None else None
        return ops.planes.sample_planes(planes, p, self.padding, base=base, lattice=lattice, nearest=self.sample_mode == 'nearest',
                                        prepared=prepared)

    def _sample_train(self, p, grid, planes):
        """The same under autograd: _SampleGridFn, then _SamplePlanesFn (HIP forward and backward, differentiable in every source)."""
        base = _SampleGridFn.apply(grid, p, self.padding) if grid is not None else None
        if not planes:
            return base
        self._check_nearest_grid(grid)
        keys = tuple(planes)
        return _SamplePlanesFn.apply(p, self.padding, self.sample_mode == 'nearest', base, keys, *[planes[k].float() for k in keys])

    def _mlp_given(self, c, p, precision=None, lattice=None, out=None):
        """The conditioned MLP on given features, no autograd, in the arithmetic the grid path takes for ``precision`` (default: the
        decoder's point precision): the split-f16 kernels for the half-precision settings, the exact-f32 ones otherwise (those
        kernels have no split-bf16 form); the wide kernels at widths beyond 32 / 32 and with `leaky`.  ``lattice``: a slab
        (nx, box, first, count) instead of points."""
        prec = precision or self._point_precision()
        if self._wide:
            mp, wide = self._wide_precision(prec), (self.hidden_size, self.n_blocks, self.leaky)
        else:
            mp, wide = ("f16x3" if prec in ("f16x3", "f16f8") else "f32"), None
        blob = self._blob(precision=mp)
        if lattice is not None:
            return ops.planes.decode_mlp_lattice(c, blob, lattice, precision=mp, wide=wide, out=out)
        return ops.decode_mlp_fwd(c, blob, p, precision=mp, wide=wide)

    def _forward_planes(self, p, grid, planes):
        if not next(iter(planes.values())).is_cuda:
            raise VtError(f"LocalDecoder: inputs must live on a HIP device (got {next(iter(planes.values())).device})")
        feats = ([grid] if grid is not None else []) + list(planes.values())
        if torch.is_grad_enabled() and (any(t.requires_grad for t in feats) or any(q.requires_grad for q in self.parameters())):
            p = p.float()
            c = self._sample_train(p, grid, planes)
            return (_DecodeMlpWideFn if self._wide else _DecodeMlpFn).apply(self, p, c, *self._params(False))
        return self._mlp_given(self._sample(p, grid, planes), p)

    # -- reference call signatures ---------------------------------------------
    def forward(self, p, c_plane, **kwargs):
        """logits [B,N] for points p [B,N,3] (decoder.py:135-161)."""
        grid, planes = self._features_of(c_plane)
        if planes:
            return self._forward_planes(p, grid, planes)
        if self._wants_grad(grid):
            return self._wide_train(p, grid) if self._wide else _DecodeFn.apply(self, p, grid, None, *self._params(False))
        if self._wide:
            return self._wide_fwd(grid, pts=p)
        prec = self._point_precision()
        return ops.decode_fwd(grid, self._blob(precision=prec), pts=p, padding=self.padding, precision=prec)

    def forward_img(self, p, c_plane, c_img, **kwargs):
        """Tactile concat variant (decoder.py:71-103): fc_p_img([p; c_img])."""
        self._refuse_planes(c_plane, "forward_img", "the MLP-on-given-features kernels (vt_decode_mlp_fwd*) take no c_img column "
                            "block (fc_p_img), and the fused vt_decode_fwd* sample a volume only")
        grid = self._grid_of(c_plane)
        if self._wants_grad(grid, c_img):
            return self._wide_train(p, grid, c_img) if self._wide else _DecodeFn.apply(self, p, grid, c_img, *self._params(True))
        if self._wide:
            return self._wide_fwd(grid, pts=p, c_img=c_img.float())
        prec = self._point_precision()
        return ops.decode_fwd(grid, self._blob(img=True, precision=prec), pts=p, c_img=c_img, padding=self.padding, precision=prec)

    def forward_contact(self, p, c_plane, **kwargs):
        """(occupancy logits, contact logits) (decoder.py:105-133)."""
        self._refuse_planes(c_plane, "forward_contact", "the MLP-on-given-features kernels (vt_decode_mlp_fwd*) have no second head "
                            "(fc_out_contact), and the fused vt_decode_fwd* sample a volume only")
        grid = self._grid_of(c_plane)
        if self._wants_grad(grid) and self._wide:
            return self._wide_train(p, grid, contact=True)
        if self._wants_grad(grid):
            # training with the contact head: the fused decode kernel with both heads and its HIP backward
            return _DecodeContactFn.apply(self, p.float(), grid, *self._params(False),
                                          self.fc_out_contact.weight, self.fc_out_contact.bias)
        if self._wide:
            return self._wide_fwd(grid, pts=p, want_contact=True)
        prec = self._point_precision()
        return ops.decode_fwd(grid, self._blob(contact=True, precision=prec), pts=p, padding=self.padding, want_contact=True,
                              precision=prec)

    # -- dense fast path: the lattice is generated in-kernel ---------------------
    def decode_lattice(self, grid, nx, box=1.1, first=0, count=None, c_img=None, out=None, precision=None):
        """Logits of ``box * make_3d_grid((-.5,)*3,(.5,)*3,(nx,)*3)[first:first+count]``
        (generation.py:155-157 + eval_points) without materialising the points.  ``grid``: the feature volume, or a ``c_plane`` dict
        (any non-empty subset of 'grid','xz','xy','yz').  Returns [B,count]; ``out``: a contiguous tensor of B * count floats to write
        into ([B,count], or [count] for one scene)."""
        count = nx ** 3 - first if count is None else count
        if isinstance(grid, dict):                 # a c_plane dict: the volume alone takes the path below, planes the sampled route
            grid, planes = self._features_of(grid)
            if planes:
                return self._decode_lattice_planes(grid, planes, nx, box, first, count, c_img, out, precision)
        if self._wide:
            return self._wide_fwd(grid, precision=precision or self.precision, lattice=(nx, box, first, count), out=out,
                                  **({} if c_img is None else {"c_img": c_img.float()}))
        precision = precision or self.precision
        if precision == "f16f8" and not ops.f16f8_covers(grid, (nx, box, first, count), self.padding):
            precision = "f16x3"                   # slabs the fp8-corrected kernel does not cover
        return ops.decode_fwd(grid, self._blob(img=c_img is not None, precision=precision), c_img=c_img,
                              padding=self.padding, lattice=(nx, box, first, count), out=out, precision=precision)


LATTICE_SLAB_POINTS = 1 << 20       # lattice points per slab of the plane route: the feature tensor stays at 2^20 x C floats (134 MB at C = 32)


def _decode_lattice_planes(self, grid, planes, nx, box, first, count, c_img=None, out=None, precision=None):
    """decode_lattice with plane features: per slab of LATTICE_SLAB_POINTS points the lattice sampler (vt_sample_grid for the volume,
    then vt_sample_planes) and the conditioned MLP on the slab's features (ops.planes.decode_mlp_lattice) -- no point tensor.
    "f16f8" runs as "f16x3" here, as on the point path."""
    if c_img is not None:
        raise VtError("LocalDecoder.decode_lattice with plane features and c_img is not built: the MLP-on-given-features kernels "
                      "(vt_decode_mlp_fwd*) take no c_img column block (fc_p_img)")
    precision = precision or self.precision
    if precision == "f16f8":
        precision = "f16x3"
    B = next(iter(planes.values())).shape[0]
    if out is None:
        out = torch.empty((B, count), dtype=torch.float32, device=next(iter(planes.values())).device)
    elif out.numel() != B * count or not out.is_contiguous():
        raise VtError(f"LocalDecoder.decode_lattice: out must be a contiguous [B,count]=({B},{count}) tensor ([count] for one scene), "
                      f"got {tuple(out.shape)}")
    out = out.view(B, count)
    step = max(1, LATTICE_SLAB_POINTS // B)
    prepared = ops.planes.Prepared()             # the planes' layout and tables are made by the first slab and kept for the others
    for lo in range(0, count, step):
        n = min(step, count - lo)
        lat = (nx, box, first + lo, n)
        c = self._sample(None, grid, planes, lattice=lat, prepared=prepared)
        if B == 1 or n == count:
            self._mlp_given(c, None, precision, lattice=lat, out=out[:, lo:lo + n])
        else:
            out[:, lo:lo + n] = self._mlp_given(c, None, precision, lattice=lat)
    return out


LocalDecoder._decode_lattice_planes = _decode_lattice_planes


def _decode_lattice_ids(self, grid, nx, finger_ids, finger_feats, box=1.1, first=0, count=None, out=None, precision=None):
    """``decode_lattice`` with the tactile feature given as (finger id per point, [F,c_dim] table)
    instead of a dense c_img tensor (what the 256^3 configuration needs: 16.7 MB of ids instead of
    2.1 GB of c_img_all)."""
    if isinstance(grid, dict):
        self._refuse_planes(grid, "decode_lattice_ids", "the finger-id kernels (vt_decode_fwd_ids, vt_decode_fwd_wide*_ids) sample a "
                            "volume only, and the MLP-on-given-features kernels take no tactile feature")
        grid = grid['grid']
    count = nx ** 3 - first if count is None else count
    if self._wide:
        # the wide kernels read the ids themselves (vt_decode_fwd_wide[_f16x3]_ids): no dense [B, count, c_dim] tensor
        return self._wide_fwd(grid, precision=precision or self.precision, lattice=(nx, box, first, count), out=out,
                              finger_ids=finger_ids.reshape(grid.shape[0], count), finger_feats=finger_feats)
    precision = precision or self.precision
    if precision == "f16f8" and not ops.f16f8_covers(grid, (nx, box, first, count), self.padding):
        precision = "f16x3"
    return ops.decode_fwd_ids(grid, self._blob(img=True, precision=precision), finger_ids, finger_feats,
                              padding=self.padding, lattice=(nx, box, first, count), out=out, precision=precision)


LocalDecoder.decode_lattice_ids = _decode_lattice_ids


class AttentionDecoder(LocalDecoder):
    """``attention_local`` (reference decoder.py:163-329): ``forward_img`` replaces the sampled
    grid features by TransformerFusion(c_img, c) -- attention + InstanceNorm across the N query
    points of the call -- before the same conditioned MLP (with fc_p, not fc_p_img).
    ``forward`` / ``forward_contact`` are LocalDecoder's."""

    def __init__(self, dim=3, c_dim=128, input_size=2048, hidden_size=256, n_blocks=5, leaky=False,
                 sample_mode='bilinear', padding=0.1, with_contact=False, **kwargs):
        super().__init__(dim=dim, c_dim=c_dim, hidden_size=hidden_size, n_blocks=n_blocks, leaky=leaky,
                         sample_mode=sample_mode, padding=padding, with_contact=with_contact)
        if self._wide and (c_dim not in (32, 64, 96, 128) or sample_mode != 'bilinear'):
            raise VtError("AttentionDecoder: the TransformerFusion kernels take c_dim (= d_model) 32, 64, 96 or 128 (the reference's "
                          "default) and the trilinear sample")
        self.mlp_precision = os.environ.get("VTACO_ATTENTION_MLP_PRECISION", "f16x3")
        self.fuser = TransformerFusion(use_xyz=True, input_size=input_size, d_model=c_dim, num_layers=1,
                                       key_feature_dim=64, with_pos_embed=False,
                                       encoder_pos_embed_input_dim=3, decoder_pos_embed_input_dim=3)
        # the reference registers fuser before fc_out_contact; order is irrelevant for load_state_dict

    def forward_img(self, p, c_plane, c_img, **kwargs):
        grid, planes = self._features_of(c_plane)
        feats = ([grid] if grid is not None else []) + list(planes.values())
        if self._wants_grad(feats[0], c_img) or (torch.is_grad_enabled() and any(t.requires_grad for t in feats)):
            # under autograd every stage is HIP, forward and backward: vt_sample_grid[_bwd] and vt_sample_planes[_bwd], vt_fusion_fwd_train /
            # vt_fusion_bwd (train-mode dropout replayed from a seed), vt_decode_mlp_fwd_train / vt_decode_mlp_bwd / vt_decode_wgrad -- at the
            # widths beyond 32 / 32 vt_decode_mlp_fwd_wide_train / vt_decode_mlp_bwd_wide / vt_rows_wgrad
            c = self._sample_train(p, grid, planes)
            c = self.fuser.forward_train(c_img, c)
            return (_DecodeMlpWideFn if self._wide else _DecodeMlpFn).apply(self, p, c, *self._params(False))
        c = self._sample(p, grid, planes)
        c = self.fuser(c_img, 1, c, 1)
        return self._mlp_fwd(c, p)

    def _mlp_fwd(self, c, p):
        """The conditioned MLP behind the fusion (inference): split-f16 layers by default (vt_decode_mlp_fwd_f16x3: f32-level logits at
        2.6x the exact-f32 kernel's rate; `mlp_precision = "f32"` / VTACO_ATTENTION_MLP_PRECISION for the exact form, which the
        generator's range guard also falls back to)."""
        prec = self.mlp_precision
        if self._wide:                                  # widths beyond 32 / 32 (the reference's defaults are 128 / 256): decode_wide.hip
            wp = self._wide_precision(prec)
            return ops.decode_mlp_fwd(c, self._blob(precision=wp), p, precision=wp, wide=(self.hidden_size, self.n_blocks, self.leaky))
        return ops.decode_mlp_fwd(c, self._blob(precision=prec), p, precision=prec)


class _PointSampleFn(torch.autograd.Function):
    """The point-feature sampler (vt_point_sample_fwd / vt_point_sample_bwd), differentiable in the features alone: neither the
    queries nor the cloud -- the network's input -- gets a gradient."""

    @staticmethod
    def forward(ctx, cloud, fea, p, sample_mode, gaussian_val):
        c, shift, total = ops.points.point_sample(cloud, fea, pts=p, sample_mode=sample_mode, gaussian_val=gaussian_val, want_saved=True)
        ctx.saved = (cloud.detach(), p.detach(), shift, total)
        ctx.mode = (sample_mode, gaussian_val)
        return c

    @staticmethod
    def backward(ctx, grad_c):
        cloud, p, shift, total = ctx.saved
        return None, ops.points.point_sample_bwd(cloud, p, shift, total, grad_c, *ctx.mode), None, None, None


class LocalPointDecoder(LocalDecoder):
    """``simple_local_point``, the decoder of the PointConv baseline (reference decoder.py:427-515): the conditioning feature of a
    query is the normalised kernel-weighted sum of per-point features over the whole input cloud -- ``c = (cloud [B,N,3], features
    [B,N,c_dim])``, what ``PointNetPlusPlus`` returns -- followed by LocalDecoder's conditioned MLP on given features.

    ``sample_mode='gaussian'`` (needs ``gaussian_val``): w = exp(-(|p_n - q| + 10e-6)^2 / gaussian_val^2); any other mode:
    w = 1 / (|p_n - q| + 10e-6).  The Gaussian quotient is evaluated with the query's largest exponent subtracted: where the
    reference's sum underflows and it returns NaN (nearest cloud point beyond ~10 gaussian_val) this returns the finite limit.
    The sampler is vt_point_sample_fwd / _bwd (``VTACO_POINTCONV=host``: its torch restatement); the reference's split into 10 000
    queries changes no value and is not mirrored.  ``padding`` and ``with_contact`` (what get_model passes) are swallowed."""

    def __init__(self, dim=3, c_dim=128, hidden_size=256, leaky=False, n_blocks=5, sample_mode='gaussian', **kwargs):
        if dim != 3:
            raise VtError("LocalPointDecoder: only dim=3 is built")
        if c_dim == 0:
            raise VtError("LocalPointDecoder: c_dim = 0 (an unconditioned MLP) is not built")
        if hidden_size % 32 or c_dim % 32 or not 32 <= hidden_size <= 256 or not 32 <= c_dim <= 256:
            raise VtError(f"LocalPointDecoder: the MLP-on-features kernels take hidden_size and c_dim multiples of 32 up to 256 "
                          f"(got {hidden_size} / {c_dim})")
        if sample_mode == 'gaussian' and kwargs.get('gaussian_val') is None:
            raise VtError("LocalPointDecoder: sample_mode 'gaussian' needs gaussian_val")
        super().__init__(dim=dim, c_dim=c_dim, hidden_size=hidden_size, n_blocks=n_blocks, leaky=leaky, sample_mode='bilinear')
        del self.fc_p_img                                   # the reference class has fc_p, fc_c, blocks and fc_out alone
        self.sample_mode = sample_mode
        self.gaussian_val = float(kwargs['gaussian_val']) if sample_mode == 'gaussian' else None

    @staticmethod
    def _pair(c):
        if not isinstance(c, (tuple, list)) or len(c) != 2:
            raise VtError("LocalPointDecoder: c must be the pair (cloud [B,N,3], features [B,N,c_dim]) the pointnet_plus_plus encoder returns")
        cloud, fea = c
        if not fea.is_cuda:
            raise VtError(f"LocalPointDecoder: inputs must live on a HIP device (got {fea.device})")
        return cloud, fea

    def _sample_points(self, cloud, fea, p=None, lattice=None):
        from ... import pointconv_host as host
        fn = ops.points.point_sample if host.form("sample" if lattice is None else "sample_lattice") == "hip" else host.point_sample
        return fn(cloud, fea, pts=p, lattice=lattice, sample_mode=self.sample_mode, gaussian_val=self.gaussian_val)

    def forward(self, p, c, **kwargs):
        """logits [B,M] for the queries p [B,M,3] (decoder.py:487-515)."""
        from ... import pointconv_host as host
        cloud, fea = self._pair(c)
        p = p.float()
        if torch.is_grad_enabled() and (fea.requires_grad or any(q.requires_grad for q in self.parameters())):
            if host.form("sample") == "hip":
                feat = _PointSampleFn.apply(cloud, fea.float(), p, self.sample_mode, self.gaussian_val)
            else:
                feat = self._sample_points(cloud.detach(), fea.float(), p)
            return (_DecodeMlpWideFn if self._wide else _DecodeMlpFn).apply(self, p, feat.contiguous(), *self._params(False))
        with torch.no_grad():
            return self._mlp_given(self._sample_points(cloud, fea, p), p)

    def forward_img(self, p, c, c_img, **kwargs):
        raise VtError("LocalPointDecoder.forward_img: the reference's PointConv decoder has no tactile variant (decoder.py:427-515)")

    def forward_contact(self, p, c, **kwargs):
        raise VtError("LocalPointDecoder.forward_contact: the reference's PointConv decoder has no contact head (decoder.py:427-515)")

    def decode_lattice(self, c, nx, box=1.1, first=0, count=None, c_img=None, out=None, precision=None):
        """Logits of ``box * make_3d_grid(...)[first:first+count]`` without materialising the points: the lattice form of the sampler,
        then ops.planes.decode_mlp_lattice, slab by slab so the feature buffer stays at LATTICE_SLAB_POINTS rows."""
        if c_img is not None:
            raise VtError("LocalPointDecoder.decode_lattice: the PointConv decoder takes no tactile feature")
        cloud, fea = self._pair(c)
        count = nx ** 3 - first if count is None else count
        precision = precision or self.precision
        if precision == "f16f8":
            precision = "f16x3"
        B = fea.shape[0]
        if out is None:
            out = torch.empty((B, count), dtype=torch.float32, device=fea.device)
        elif out.numel() != B * count or not out.is_contiguous():
            raise VtError(f"LocalPointDecoder.decode_lattice: out must be a contiguous [B,count]=({B},{count}) tensor ([count] for one "
                          f"scene), got {tuple(out.shape)}")
        out = out.view(B, count)
        step = max(1, LATTICE_SLAB_POINTS // B)
        with torch.no_grad():
            for lo in range(0, count, step):
                n = min(step, count - lo)
                lat = (nx, box, first + lo, n)
                feat = self._sample_points(cloud, fea, lattice=lat)
                if B == 1 or n == count:
                    self._mlp_given(feat, None, precision, lattice=lat, out=out[:, lo:lo + n])
                else:
                    out[:, lo:lo + n] = self._mlp_given(feat, None, precision, lattice=lat)
        return out

    def decode_lattice_ids(self, *args, **kwargs):
        raise VtError("LocalPointDecoder.decode_lattice_ids: the PointConv decoder takes no tactile feature")
