"""A plain reference of TransformerFusion (CPU, torch only) for the float64 gates of tests/test_fusion_f64_gpu.py: one attention unit
and the whole fuser restated in float64, float64 MODELS of the operand roundings the kernels make on purpose, the case tables, the
launch plan restated from the kernels' comments, and the error measures.

One attention unit, X_q (queries) against X_k (keys / values), all [B,N,C] (oracle/vtaco_oracle.py: _relation_unit, _trans_nonlinear):

    Q = l2norm(X_q WQ^T), K = l2norm(X_k WK^T) (64-d), V = X_k WV^T
    E = exp(Q K^T);  l_q = sum_k E_qk;  s_k = sum_q E_qk / l_q;  O_q = (1 / l_q) sum_k E_qk V'_k,  V' = V / (1e-9 + s)
    r = relu((X_q - O) Wt^T);  y = LayerNorm(r + m1 (W2 (m0 relu(W1 r + b1)) + b2));  z = X_q + y        (m0, m1: dropout factors)
    out = relu(InstanceNorm_N(z))

The fuser: mem = unit_self(c, c), tgt = unit_self(c_img, c_img) (the SAME weights), out = unit_cross(tgt, mem).

``form`` (the comments at the top of vtaco_amd/csrc/fusion.hip):
    "exact"      no rounding
    "full"       Q log2(e) and K as half pairs -- hi = half(v), lo = half(v - hi) -- with the score hi.hi + hi.lo + lo.hi (no lo.lo), E = 2^score;
                 E and V' as bf16 pairs with the same three products; l and s from the unsplit E.  The training forward, every d_model > 32
    "half_pair"  as "full" with K replaced by half(K): inference, N < 512
(inference at N >= 512 adds fp8 correction products, which are not modelled: that form keeps the contract of tests/test_fusion_gpu.py)
Every rounding is written straight-through, v + (round(v) - v).detach(), so autograd through a model gives the gradients of the
rounded-operand computation (a pair's hi carries the gradient of v, its lo none).

Parameters travel as ``units = {"self": {...}, "cross": {...}}`` with the ten names of ops.FUSION_TENSORS; gradients as a flat dict
"c_img", "c", "self.WK", ..., "cross.norm2_b" (the shared self-attention's: the sum of both uses).
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GATE = 8.0
F8_CONTRACT = 5e-5                    # tests/test_fusion_gpu.py: the fused features to 5e-5 absolute
LOG2E = 1.4426950408889634
NAMES = ("WK", "WQ", "WV", "trans_conv", "linear1_w", "linear1_b", "linear2_w", "linear2_b", "norm2_w", "norm2_b")
_SD = {"WK": "head.0.WK.weight", "WQ": "head.0.WQ.weight", "WV": "head.0.WV.weight", "trans_conv": "head.0.trans_conv.weight",
       "linear1_w": "extra_nonlinear.0.linear1.weight", "linear1_b": "extra_nonlinear.0.linear1.bias",
       "linear2_w": "extra_nonlinear.0.linear2.weight", "linear2_b": "extra_nonlinear.0.linear2.bias",
       "norm2_w": "extra_nonlinear.0.norm2.weight", "norm2_b": "extra_nonlinear.0.norm2.bias"}
_PRE = {"self": "decoder.layers.0.self_attn.", "cross": "decoder.layers.0.cross_attn."}


def units_of(sd, dtype=torch.float64):
    """The two units out of a fuser's state_dict (keys relative to the fuser), as fresh tensors of ``dtype``."""
    return {u: {n: sd[_PRE[u] + _SD[n]].detach().to(dtype).clone() for n in NAMES} for u in ("self", "cross")}


def oracle_sd(units):
    """The state_dict oracle.vtaco_oracle.transformer_fusion reads; the encoder's and the decoder's self-attention are the SAME tensors,
    so autograd sums both uses."""
    sd = {}
    for pre, u in (("encoder.layers.0.self_attn.", "self"), (_PRE["self"], "self"), (_PRE["cross"], "cross")):
        for n in NAMES:
            sd[pre + _SD[n]] = units[u][n]
    return sd


# ---- the operand roundings -----------------------------------------------------------------------------------------------------
def _st(v, dt):
    return v + (v.to(dt).to(v.dtype) - v).detach()


def _pair(v, dt):
    hi = _st(v, dt)
    return hi, _st(v - hi, dt)


def _t(x):
    return x.transpose(1, 2)


def attention_unit(u, xq, xk, form="exact", masks=None, taps=None):
    """One unit in the dtype of its arguments.  ``masks`` = (m0 [B,N,64], m1 [B,N,C]) or None; ``taps``: a list that receives the
    pre-InstanceNorm tensor z."""
    q = F.normalize(xq @ u["WQ"].t(), p=2, dim=-1)
    k = F.normalize(xk @ u["WK"].t(), p=2, dim=-1)
    v = xk @ u["WV"].t()
    if form == "exact":
        e = torch.exp(q @ _t(k))
        l = e.sum(dim=-1, keepdim=True)
        s = (e / l).sum(dim=1)                                   # [B,Nk]: the column sums of the softmax
        o = (e @ (v / (1e-9 + s).unsqueeze(-1))) / l
    elif form in ("full", "half_pair"):
        qh, ql = _pair(q * LOG2E, torch.float16)
        kh, kl = _pair(k, torch.float16)
        sc = qh @ _t(kh) + ql @ _t(kh)
        if form == "full":
            sc = sc + qh @ _t(kl)
        e = torch.exp2(sc)
        l = e.sum(dim=-1, keepdim=True)
        s = (e / l).sum(dim=1)
        eh, el = _pair(e, torch.bfloat16)
        vh, vl = _pair(v / (1e-9 + s).unsqueeze(-1), torch.bfloat16)
        o = (eh @ vh + eh @ vl + el @ vh) / l
    else:
        raise ValueError(f"form {form!r}")
    r = torch.relu((xq - o) @ u["trans_conv"].t())
    h = torch.relu(r @ u["linear1_w"].t() + u["linear1_b"])
    if masks is not None:
        h = h * masks[0]
    y = h @ u["linear2_w"].t() + u["linear2_b"]
    if masks is not None:
        y = y * masks[1]
    z = xq + F.layer_norm(r + y, (r.shape[-1],), u["norm2_w"], u["norm2_b"], 1e-5)
    if taps is not None:
        taps.append(z)
    m = z.mean(dim=1, keepdim=True)
    var = ((z - m) ** 2).mean(dim=1, keepdim=True)
    return torch.relu((z - m) / torch.sqrt(var + 1e-5))


def fuser(units, c_img, c, form="exact", masks=None, taps=None):
    """TransformerFusion.forward(search=c_img, template=c); ``masks``: three pairs (encoder self-attention on c, decoder
    self-attention on c_img, cross-attention) or None."""
    masks = masks or (None, None, None)
    mem = attention_unit(units["self"], c, c, form, masks[0], taps)
    tgt = attention_unit(units["self"], c_img, c_img, form, masks[1], taps)
    return attention_unit(units["cross"], tgt, mem, form, masks[2], taps)


# ---- the launch plan, restated from the comments of fusion.hip / fusion_bwd.hip / include/vtaco_hip.h ---------------------------
def expected_plan(B, N, d_model=32, train=False, cus=256):
    """What ops.fusion_plan must answer (VTACO_FUSION_SCORE_TERMS unset); ``cus``: the device's compute units (MI355X: 256)."""
    up = lambda a, b: -(-a // b)
    P, wide = B * N, d_model > 32
    form = "full" if (wide or train) else ("f8" if N >= 512 else "half_pair")
    strided = []
    if up(B * up(N, 32) * (64 if form == "f8" else 128), 256) > 8192:
        strided.append("scalev")
    if wide and up(P, 32) > 4 * cus:
        strided.append("epilogue")
    if train and up(P * d_model, 256) > 4096:               # (the backward's two grids: of a call that keeps the state for one)
        strided.append("add")
    if train and wide and up(P, 4) > cus:
        strided.append("bwd_point")
    return {"form": form, "proj_tiles": 8 if wide else min(8, max(1, P // (128 * 1536))),
            "inorm": "streamed" if (wide or N > 2048) else "cached", "fwd_row_blocks": up(N, 256), "bwd_row_blocks": up(N, 128),
            "strided": tuple(strided)}


# ---- cases ---------------------------------------------------------------------------------------------------------------------
# (name, d_model, B, N, mode, distinct, weights, want): mode "infer" (fusion_fwd at d_model 32), "fwd" (fusion_fwd at d_model > 32: all
# three score products), "bwd" (fusion_fwd_train + fusion_bwd without dropout), "drop" (the same in train mode, p = 0.1);  distinct: the
# batch is that many distinct chunks repeated (chunk b = distinct chunk PATTERN[b % len]);  want: the part of the plan the case is
# listed for.  Seeds: 1000 + the case's index; a seed that fails one of test_fusion_ref_cpu.py's checks of the cases -- all judged by
# the reference alone -- moves on by 500 (RESEEDED).
# min std: the smallest per-channel standard deviation over a chunk of the three pre-InstanceNorm tensors (float64, the reference
# alone: test_fusion_ref_cpu.py prints it); a channel that is nearly constant has its rounding noise multiplied by up to 316.
CASES = [
    # inference, d_model 32                                                             (the trailing comment of each case: its min std)
    ("i-1x2", 32, 1, 2, "infer", 0, "seed", {"form": "half_pair", "fwd_row_blocks": 1}),  # 0.00231
    ("i-2x31", 32, 2, 31, "infer", 0, "seed", {"form": "half_pair"}),  # 0.108
    ("i-2x32", 32, 2, 32, "infer", 0, "seed", {"form": "half_pair"}),  # 0.236
    ("i-2x33", 32, 2, 33, "infer", 0, "seed", {"form": "half_pair"}),  # 0.32
    ("i-3x255", 32, 3, 255, "infer", 0, "seed", {"form": "half_pair", "fwd_row_blocks": 1}),  # 0.45
    ("i-1x256-g5", 32, 1, 256, "infer", 0, "g5", {"form": "half_pair", "fwd_row_blocks": 1}),  # 0.474
    ("i-2x257", 32, 2, 257, "infer", 0, "seed", {"form": "half_pair", "fwd_row_blocks": 2}),  # 0.385
    ("i-1x511", 32, 1, 511, "infer", 0, "seed", {"form": "half_pair"}),  # 0.552
    ("i-1x512", 32, 1, 512, "infer", 0, "seed", {"form": "f8"}),  # 0.491
    ("i-2x513", 32, 2, 513, "infer", 0, "seed", {"form": "f8", "fwd_row_blocks": 3}),  # 0.37
    ("i-1x2048", 32, 1, 2048, "infer", 0, "seed", {"form": "f8", "inorm": "cached"}),  # 0.421
    ("i-2x2049", 32, 2, 2049, "infer", 0, "seed", {"form": "f8", "inorm": "streamed", "fwd_row_blocks": 9}),  # 0.488
    ("i-193x2048", 32, 193, 2048, "infer", 2, "seed", {"form": "f8", "proj_tiles": 2}),  # 0.545
    ("i-8200x33", 32, 8200, 33, "infer", 2, "seed", {"form": "half_pair", "strided": ("scalev",)}),  # 0.257
    ("i-2050x512", 32, 2050, 512, "infer", 2, "seed", {"form": "f8", "strided": ("scalev",)}),  # 0.318
    # training forward and backward, d_model 32
    ("t-1x127", 32, 1, 127, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 1}),  # 0.426
    ("t-2x128", 32, 2, 128, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 1}),  # 0.388
    ("t-1x129", 32, 1, 129, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 2}),  # 0.445
    ("t-3x171", 32, 3, 171, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 2}),  # 0.446
    ("t-1x2049", 32, 1, 2049, "bwd", 0, "seed", {"form": "full", "inorm": "streamed", "bwd_row_blocks": 17}),  # 0.547
    ("t-17x2048", 32, 17, 2048, "bwd", 2, "seed", {"form": "full", "strided": ("add",)}),  # 0.37
    ("t-2x257-drop", 32, 2, 257, "drop", 0, "seed", {"form": "full", "fwd_row_blocks": 2, "bwd_row_blocks": 3}),  # 0.584
    # wide forward
    ("w64-2x33", 64, 2, 33, "fwd", 0, "seed", {"form": "full", "inorm": "streamed"}),  # 0.254
    ("w64-1x257", 64, 1, 257, "fwd", 0, "seed", {"form": "full", "fwd_row_blocks": 2}),  # 0.49
    ("w64-1x2049", 64, 1, 2049, "fwd", 0, "seed", {"form": "full", "fwd_row_blocks": 9}),  # 0.484
    ("w64-17x2048", 64, 17, 2048, "fwd", 2, "seed", {"form": "full", "strided": ("epilogue",)}),  # 0.354
    ("w128-2x33", 128, 2, 33, "fwd", 0, "seed", {"form": "full", "inorm": "streamed"}),  # 0.24
    ("w128-1x257", 128, 1, 257, "fwd", 0, "seed", {"form": "full", "fwd_row_blocks": 2}),  # 0.391
    ("w128-1x2049", 128, 1, 2049, "fwd", 0, "seed", {"form": "full", "fwd_row_blocks": 9}),  # 0.475
    ("w128-17x2048", 128, 17, 2048, "fwd", 2, "seed", {"form": "full", "strided": ("epilogue",)}),  # 0.361
    # wide backward (eval mode: the fuser's differentiable path without dropout)
    ("w64-b2x129", 64, 2, 129, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 2, "strided": ()}),  # 0.364
    ("w64-b3x171", 64, 3, 171, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 2, "strided": ()}),  # 0.404
    ("w128-b2x129", 128, 2, 129, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 2, "strided": ()}),  # 0.272
    ("w128-b3x171", 128, 3, 171, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 2, "strided": ()}),  # 0.315
    ("w96-b2x65", 96, 2, 65, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 1, "strided": ()}),  # 0.403
    # (beyond the list the suite was asked for: the wide backward's per-point kernels past one workgroup per compute unit)
    ("w64-b1x1100", 64, 1, 1100, "bwd", 0, "seed", {"form": "full", "bwd_row_blocks": 9, "strided": ("bwd_point",)}),  # 0.437
]
NAMES_OF_CASES = [c[0] for c in CASES]
# the cases whose seed failed a reference-only check of test_fusion_ref_cpu.py, and how many steps of 500 their seed moved on.
# i-2x33: the half-pair MODEL's own error e_form is 8.0e-5, 5.6e-5, 5.4e-5, 5.7e-5 at steps 0..3 -- above the 5e-5 every forward floor must
# keep -- and 3.5e-5 at step 4 (33 keys average the keys' half rounding least of all the cases; 4.1e-5..4.6e-5 at the other chunks of
# 31..33 points).  No kernel output was looked at.
RESEEDED = {"i-2x33": 4}
PATTERN = (0, 1, 1, 0, 1)               # which distinct chunk sits where in a repeated batch (both at odd and even places)
DROP_SEED, P_DROP = 24680, 0.1


def chunk_index(B, distinct):
    """[B] long: the distinct chunk of batch element b; the identity where the case repeats nothing."""
    if not distinct:
        return torch.arange(B)
    return torch.tensor([PATTERN[b % len(PATTERN)] for b in range(B)])


def form_of(case):
    """The model that is the floor of the case's forward gate, or None for the f8 form (not modelled: fixed contract)."""
    f = expected_plan(case[2], case[3], case[1], case[4] != "infer")["form"]
    return None if f == "f8" else f


@functools.lru_cache(maxsize=None)
def case_inputs(i):
    """(units float32, c_img, c, wgt) of CASES[i] -- the DISTINCT chunks only: _fusion_case of tests/test_fusion_gpu.py (a seeded
    TransformerFusion with perturbed biases and norm2, ~30 % of the c_img rows non-zero), or the golden g5's weights and inputs."""
    name, C, B, N, mode, distinct, weights, _want = CASES[i]
    nb = distinct or B
    if weights == "g5":
        from conftest import load_golden, sub_sd
        a, sd = load_golden("g5_fusion.npz")
        units = units_of(sub_sd(sd, "fuser."), torch.float32)
        c_img, c = torch.from_numpy(a[f"c_img{N}"][:nb]).clone(), torch.from_numpy(a[f"c{N}"][:nb]).clone()
        wgt = torch.randn(nb, N, C, generator=torch.Generator().manual_seed(1000 + i))
        return units, c_img, c, wgt
    from vtaco_amd.transformer_fusion import TransformerFusion
    seed = 1000 + i + 500 * RESEEDED.get(name, 0)
    rng = torch.random.get_rng_state()
    torch.manual_seed(seed)
    net = TransformerFusion(d_model=C, key_feature_dim=64, with_pos_embed=False)
    torch.random.set_rng_state(rng)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for pname, prm in net.named_parameters():
            if "norm2" in pname or pname.endswith(".bias"):
                prm.add_(torch.randn(prm.shape, generator=g) * 0.2)
    c_img = torch.randn(nb, N, C, generator=g) * (torch.rand(nb, N, 1, generator=g) < 0.3)
    c = torch.randn(nb, N, C, generator=g)
    wgt = torch.randn(nb, N, C, generator=g)
    return units_of(net.state_dict(), torch.float32), c_img, c, wgt


def module_of(units, C):
    """A TransformerFusion carrying ``units`` (the library's module, for the GPU tests)."""
    from vtaco_amd.transformer_fusion import TransformerFusion
    net = TransformerFusion(d_model=C, key_feature_dim=64, with_pos_embed=False)
    sd = net.state_dict()
    for k, v in oracle_sd(units).items():
        sd[k] = v.clone()
    net.load_state_dict(sd)
    return net


def grad_names():
    return ["c_img", "c"] + [f"{u}.{n}" for u in ("self", "cross") for n in NAMES]


def _run(units32, c_img, c, wgt, mult, dtype, form, masks, want_grads, oracle=False):
    """out (detached) and, with ``want_grads``, the flat gradient dict of L = sum_b mult_b sum(out_b wgt_b): the parameter gradients
    are then the multiplicity-weighted sums of the repeated batch and the input gradients (divided by mult) those of one copy."""
    units = {u: {n: t.to(dtype).clone().requires_grad_(want_grads) for n, t in d.items()} for u, d in units32.items()}
    ci, cc = c_img.to(dtype).clone().requires_grad_(want_grads), c.to(dtype).clone().requires_grad_(want_grads)
    mk = None if masks is None else [tuple(m.to(dtype) for m in pair) for pair in masks]
    with torch.set_grad_enabled(want_grads):
        if oracle:
            from oracle import vtaco_oracle as orc
            out = orc.transformer_fusion(oracle_sd(units), ci, cc, masks=mk)
        else:
            out = fuser(units, ci, cc, form, mk)
    if not want_grads:
        return out.detach().double(), None
    mw = mult.to(dtype).reshape(-1, 1, 1)
    (out * wgt.to(dtype) * mw).sum().backward()
    grads = {"c_img": (ci.grad / mw).double(), "c": (cc.grad / mw).double()}
    for u in ("self", "cross"):
        for n in NAMES:
            grads[f"{u}.{n}"] = units[u][n].grad.double()
    return out.detach().double(), grads


def dropout_mask(p_drop, seed, call, which, points, d_model=32):
    """The dropout factors (0 or 1 / (1 - p)) of attention call ``call`` (0 encoder, 1 decoder self-attention, 2 cross-attention),
    ``which`` 0 ([points, 64], after linear1) or 1 ([points, d_model], after linear2): the keep rule of fusion_common.h restated -- a
    64-bit mix of (seed, call, which, point, channel), keep iff its high word >= p 2^32 -- which ops.fusion_dropout_mask must equal."""
    width, shift = (64 if which == 0 else d_model), (6 if d_model == 32 else 8)
    p32 = np.float32(p_drop)
    thresh = np.uint64(min(int(float(p32) * 4294967296.0), 0xffffffff))
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    pt, ch = np.meshgrid(np.arange(points, dtype=np.uint64), np.arange(width, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * ((np.uint64(call * 2 + which) << np.uint64(40)) + (pt << np.uint64(shift)) + ch + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return torch.from_numpy(np.where((z >> np.uint64(32)) >= thresh, scale, np.float32(0.0)).astype(np.float32))


def case_masks(i):
    """The three pairs of dropout factors [B,N,.] of a "drop" case, None otherwise."""
    name, C, B, N, mode = CASES[i][:5]
    if mode != "drop":
        return None
    return [tuple(dropout_mask(P_DROP, DROP_SEED, call, which, B * N, C).reshape(B, N, -1) for which in (0, 1)) for call in range(3)]


@functools.lru_cache(maxsize=None)
def references(i):
    """Of CASES[i], on its distinct chunks: {"out64", "out32", "out_full", "out_half_pair" (inference cases), "e32", "e_full",
    "e_half_pair", and for the backward cases "g64", "ge32", "ge_full": per-tensor rel_err of the float32 oracle's and of the "full"
    model's autograd against float64 autograd of the exact reference}."""
    name, C, B, N, mode, distinct, weights, _want = CASES[i]
    units, c_img, c, wgt = case_inputs(i)
    nb = c.shape[0]
    mult = torch.bincount(chunk_index(B, distinct), minlength=nb).double() if distinct else torch.ones(nb, dtype=torch.float64)
    masks = case_masks(i)
    bwd = mode in ("bwd", "drop")
    r = {"mult": mult}
    r["out64"], g64 = _run(units, c_img, c, wgt, mult, torch.float64, "exact", masks, bwd)
    r["out32"], g32 = _run(units, c_img, c, wgt, mult, torch.float32, None, masks, bwd, oracle=True)
    r["out_full"], gfull = _run(units, c_img, c, wgt, mult, torch.float64, "full", masks, bwd)
    r["e32"] = float((r["out32"] - r["out64"]).abs().max())
    r["e_full"] = float((r["out_full"] - r["out64"]).abs().max())
    if mode == "infer":
        r["out_half_pair"], _ = _run(units, c_img, c, wgt, mult, torch.float64, "half_pair", None, False)
        r["e_half_pair"] = float((r["out_half_pair"] - r["out64"]).abs().max())
    if bwd:
        r["g64"] = g64
        r["ge32"] = rel_errs(g32, g64, mult)
        r["ge_full"] = rel_errs(gfull, g64, mult)
    return r


# ---- error measures ------------------------------------------------------------------------------------------------------------
def rel_errs(g, g64, mult=None):
    """Per tensor ||t - t64||_2 / ||t64||_2 (L2: a single ReLU flip moves single entries); a PARAMETER whose float64 gradient norm is
    below 1e-2 of the largest parameter gradient norm is measured against 1e-2 of that largest norm (_check_fusion_grads' floor).
    ``mult`` [chunks]: the input gradients' chunks count that many times, as in the repeated batch they stand for."""
    top = max(float(v.norm()) for k, v in g64.items() if "." in k)
    out = {}
    for k, v in g64.items():
        d = g[k].double() - v
        if "." in k:
            den = max(float(v.norm()), 1e-2 * top)
        else:
            w = torch.ones(v.shape[0], dtype=torch.float64) if mult is None else mult.sqrt()
            d, v = d * w.reshape(-1, 1, 1), v * w.reshape(-1, 1, 1)
            den = float(v.norm())
        out[k] = float(d.norm()) / max(den, 1e-300)
    return out


def forward_floor(r, form):
    """max(e32, e_form): the floor of a forward gate."""
    return max(r["e32"], r["e_" + form])


def min_channel_std(i):
    """The smallest per-channel standard deviation over a chunk of the three pre-InstanceNorm tensors of CASES[i] (float64, exact)."""
    units, c_img, c, _ = case_inputs(i)
    taps = []
    u64 = {u: {n: t.double() for n, t in d.items()} for u, d in units.items()}
    mk = case_masks(i)
    with torch.no_grad():
        fuser(u64, c_img.double(), c.double(), "exact", mk and [tuple(m.double() for m in pair) for pair in mk], taps)
    return [float(z.std(dim=1, unbiased=False).min()) for z in taps]
