"""The lattice decode's references and cases (CPU, torch and numpy only), for tests/test_decode_lattice_f64_gpu.py:

* the float64 / float32 / magnitude-sum forwards of tests/decode_train_ref.py on the query lattice of tests/decode_train_cases.py;
* ``forward_split64``: a plain float64 model of the split arithmetic of the "bf16x3" and "f16x3" kernels as decode_common.h states it.
  In each of the 15 dense 32x32 layers (fc_c_i on c, fc_0_i on relu(x_i), fc_1_i on relu(h_i)) the product is
  W_hi x_hi + W_hi x_lo + W_lo x_hi with hi + lo the two 16-bit parts of an operand -- "f16x3": hi the IEEE half rounded toward zero,
  lo = half(v - hi); "bf16x3": hi = bf16(v), lo = bf16(v - hi) -- the parts held exactly and summed in float64; fc_p, the biases, the
  residual stream and the output heads are float64.  Its distance from forward64, e_split = max |split64 - ref64|, is what the operand
  rounding of a split kernel costs: the yardstick of those kernels.  A yardstick of magnitude, not a bit model of the kernels;
* ``expected_form``: the dispatch rule of the lattice launchers, restated from the comments of vtaco_amd/csrc/decode.hip;
* ``CASES``: the lattices at the bounds of every kernel form, each with the form it has to run.
"""
import functools
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_train_cases as cases
import decode_train_ref as ref

NB = ref.NB
FORMS = ("linear", "brick", "staged", "staged2", "staged3")
PRECISIONS = ("f32", "bf16x3", "f16x3")


# ---- 16-bit roundings of float64 values, written out ----------------------------------------------------------------------------
def _round(v, bits, emin, toward_zero=False):
    """float64 tensor -> the binary format with ``bits`` significand bits and smallest normal 2^emin, to nearest (ties to even) or
    toward zero, as float64.  Normal range: on the bit pattern, where the dropped 53 - bits significand bits are the low bits of a
    sign-magnitude integer (a carry out of the significand moves the exponent, as it should); below 2^emin the spacing is the
    constant 2^(emin - bits + 1) of the subnormals."""
    v = torch.as_tensor(v, dtype=torch.float64).contiguous()
    drop = 53 - bits
    u = v.view(torch.int64)
    if not toward_zero:
        u = u + ((u >> drop) & 1) + ((1 << (drop - 1)) - 1)
    r = (u & ~((1 << drop) - 1)).view(torch.float64)
    q = 2.0 ** (emin - bits + 1)
    small = (torch.trunc(v / q) if toward_zero else torch.round(v / q)) * q          # torch.round: halves to even
    return torch.where(v.abs() < 2.0 ** emin, small, r)


def round_half(v, toward_zero=False):
    """float64 -> the nearest IEEE half (ties to even), or the next half toward zero; the result as float64.  Saturates at 65504, as
    the kernels' round-toward-zero conversion does."""
    return _round(v, 11, -14, toward_zero).clamp(-65504.0, 65504.0)


def round_bf16(v):
    """float64 -> the nearest bfloat16 (8 significand bits, float32's exponent range; ties to even) as float64."""
    return _round(v, 8, -126)


def split(v, kind):
    """(hi, lo) of ``v`` (a float64 tensor) as float64 tensors: "f16x3" hi = half toward zero, lo = half(v - hi); "bf16x3" hi = bf16(v),
    lo = bf16(v - hi).  v - hi is exact in float64."""
    v = v.detach().double()
    if kind == "f16x3":
        hi = round_half(v, toward_zero=True)
        return hi, round_half(v - hi)
    if kind == "bf16x3":
        hi = round_bf16(v)
        return hi, round_bf16(v - hi)
    raise ValueError(kind)


def split_linear(x, W, kind):
    """x @ W^T of one dense layer in split arithmetic: W_hi x_hi + W_hi x_lo + W_lo x_hi, summed in float64.  ``x``: the operand or
    its (hi, lo) pair.  x_hi + x_lo is exact in float64 (at most 24 significand bits), so the two W_hi products are one matmul."""
    xh, xl = x if isinstance(x, tuple) else split(x, kind)
    wh, wl = split(W, kind)
    return (xh + xl) @ wh.t() + xh @ wl.t()


def forward_split64(sd, pts, grid, kind, c_img=None, contact=False, padding=0.1, c=None):
    """decode_train_ref.forward64 with the 15 dense layers in split arithmetic.  Logits [B,N], or the pair with ``contact``.
    ``c``: forward64's float64 features (its first saved tensor), if they are at hand."""
    dt = torch.float64
    P = ref._params(sd, c_img is not None, dt)
    pf = pts.detach().float().to(dt)
    if c is None:
        idx, w = ref.trilinear(pts, grid.shape[2], padding, dt)
        c = ref.sample(grid.detach().to(dt), idx, w)
    cs = split(c, kind)
    x = pf @ P["Wp"][:, :3].t() + P["bp"]
    if c_img is not None:
        x = x + c_img.detach().to(dt) @ P["Wp"][:, 3:].t()
    x = x + split_linear(cs, P["Wc"][0], kind) + P["bc"][0]
    for i in range(NB):
        h = split_linear(torch.relu(x), P["W0"][i], kind) + P["b0"][i]
        x = x + split_linear(torch.relu(h), P["W1"][i], kind) + P["b1"][i]
        if i + 1 < NB:
            x = x + split_linear(cs, P["Wc"][i + 1], kind) + P["bc"][i + 1]
    a = torch.relu(x)
    out = (a @ P["Wo"].t() + P["bo"]).squeeze(-1)
    if contact:
        return out, (a @ P["Wo2"].t() + P["bo2"]).squeeze(-1)
    return out


def e_split(split64, ref64):
    """max |split64 - ref64| over the scenes ``split64`` has (the leading ones of ``ref64``)."""
    assert split64.shape[1:] == ref64.shape[1:] and split64.shape[0] <= ref64.shape[0]
    return float((split64.double() - ref64[:split64.shape[0]].double()).abs().max())


def gate_ratio_floor(got, ref64, floor, bound):
    """max over the elements of |got - ref64| / max(floor, 2^-24 bound): decode_train_ref.gate_ratio with the scalar floor given."""
    ref64 = ref64.double()
    err = (got.detach().double().cpu().reshape(ref64.shape) - ref64).abs()
    base = torch.clamp(bound.double().reshape(ref64.shape) * 2.0 ** -24, min=float(floor))
    assert float(base.min()) > 0.0
    return float((err / base).max())


# ---- the dispatch rule, restated ----------------------------------------------------------------------------------------------------
LDS_BYTES = 160 * 1024
BLOB_FLOATS = 11 * 32 + 96 + 128 + 15 * 1024 + 1024 + 5 * 256 + 256          # the packed decoder (vt_common.h), staged whole in LDS
ROW_BYTES = 144                                                              # one voxel's 32 channels + 16 B pad
ST_IMAGE = 48 * ROW_BYTES                                                    # 3 x 4 x 4 voxels, twelve waves
ST2_IMAGE = 72 * ROW_BYTES                                                   # 3 x 4 x 6 voxels, eight waves
TAIL_BYTES = 256


def step_voxels(nx, R, box=1.1, padding=0.1):
    """s = (R - 1) box / ((nx - 1) divisor): voxels per lattice step."""
    return (R - 1) * float(np.float32(box)) / ((nx - 1) * ref.divisor(padding))


def _atoi(text):
    m = re.match(r"\s*[+-]?\d+", text)
    return int(m.group()) if m else 0


def expected_form(nx, R, box=1.1, first=0, count=None, padding=0.1, precision="f32", want_contact=False, c_direct=False, env=None):
    """The form decode.hip's comments promise: linear tiles unless the slab is whole x-plane pairs of an nx % 4 == 0 lattice; bricks
    staged in LDS for a sampled grid of R >= 4, nx <= 512 with s < 0.66 (3 x 4 x 4 footprint); double bricks for nx % 8 == 0, R >= 6,
    s < 0.55 without a contact head (3 x 4 x 6 footprint) -- staged3 for the half-precision forms, staged2 for the others; each only
    if blob + tables + images fit the CU's 160 KiB.  "f16f8" exists as staged3 only (None otherwise).  ``env``: the A/B knobs."""
    env = os.environ if env is None else env
    count = nx ** 3 - first if count is None else count
    pair = 2 * nx * nx
    s = step_voxels(nx, R, box, padding)
    aligned = first % pair == 0 and count % pair == 0
    st3 = nx % 8 == 0 and R >= 6 and 0 < s < 0.55 and BLOB_FLOATS * 4 + 20 * nx + 8 * ST2_IMAGE + TAIL_BYTES <= LDS_BYTES
    if precision == "f16f8":
        return "staged3" if nx >= 8 and count > 0 and aligned and st3 and not want_contact and not c_direct else None
    if nx % 4 != 0 or not aligned:
        return "linear"
    if "VTACO_DECODE_DIRECT" in env or R < 4 or nx > 512 or c_direct:
        return "brick"
    pairs = "VTACO_DECODE_NO_PAIR" not in env and not want_contact
    no_st3 = "VTACO_DECODE_ST3" in env and _atoi(env["VTACO_DECODE_ST3"]) == 0
    if precision == "f16x3" and pairs and not no_st3 and st3:
        return "staged3"
    if pairs and nx % 8 == 0 and R >= 6 and 0 < s < 0.55 and BLOB_FLOATS * 4 + 16 * nx + 8 * ST2_IMAGE + TAIL_BYTES <= LDS_BYTES:
        return "staged2"
    if 0 < s < 0.66 and BLOB_FLOATS * 4 + 16 * nx + 12 * ST_IMAGE <= LDS_BYTES:
        return "staged"
    return "brick"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
class Case:
    """A lattice (nx, box) over a grid of side R with the module's ``padding``, the step it was listed with, the form the f32 / bf16x3
    kernels and the f16x3 kernel have to run (``form``, ``form16``), and whether the tactile and contact forms are run on it too."""

    def __init__(self, nx, R, s, form, form16=None, box=1.1, padding=0.1, extras=False):
        self.nx, self.R, self.s, self.form, self.form16 = nx, R, s, form, form16 or form
        self.box, self.padding, self.extras = box, padding, extras
        self.id = f"nx{nx}-R{R}" + (f"-box{box}" if box != 1.1 else "") + (f"-pad{padding}" if padding != 0.1 else "")

    def listed(self, precision):
        return self.form16 if precision in ("f16x3", "f16f8") else self.form

    def lattice(self, first=0, count=None):
        return (self.nx, self.box, first, self.nx ** 3 - first if count is None else count)

    def slab(self):
        """Two x-plane pairs starting at plane pair 1."""
        return self.lattice(2 * self.nx ** 2, 4 * self.nx ** 2)

    def ragged(self):
        """A range that starts inside a row: linear tiles."""
        return self.lattice(7, min(1000, self.nx ** 3 - 7))


CASES = [
    Case(10, 8, 0.777, "linear"),                                  # nx % 4 != 0
    Case(16, 3, 0.133, "brick"),                                   # R < 4
    Case(8, 4, 0.428, "staged"),                                   # the smallest grid: the footprint is the whole grid
    Case(8, 5, 0.571, "staged"),                                   # nx % 8 == 0 but R < 6
    Case(12, 8, 0.636, "staged"),                                  # nx % 8 != 0
    Case(16, 6, 0.333, "staged2", "staged3"),                      # the smallest double-brick grid
    Case(16, 9, 0.533, "staged2", "staged3", extras=True),
    Case(32, 18, 0.548, "staged2", "staged3"),                     # just under 0.55
    Case(16, 10, 0.600, "staged", extras=True),                    # just over 0.55
    Case(24, 16, 0.652, "staged"),
    Case(48, 32, 0.659, "staged"),                                 # just under 0.66
    Case(16, 11, 0.666, "brick", extras=True),                     # just over 0.66
    Case(16, 9, 0.533, "staged2", "staged3", box=1.0, padding=0.0),   # another divisor
    Case(16, 8, 0.509, "staged2", "staged3", box=1.2),             # points clamped on both sides
    Case(16, 9, 0.630, "staged", box=1.3),                         # clamped, single bricks
]
BATCH = 2
N_FINGERS = 5


def weight_sets():
    return cases.weight_sets()


@functools.lru_cache(maxsize=None)
def inputs(case_index):
    """(pts [B,nx^3,3] -- the lattice, the same in both scenes --, grid [B,32,R,R,R] -- two different grids --) and, for the cases with
    extras, (finger ids [B,nx^3] uint8 with about 30 % of the rows set, the feature table [F,32], the dense c_img they stand for)."""
    cs = CASES[case_index]
    g = torch.Generator().manual_seed(7919 * cs.nx + 31 * cs.R + case_index)
    grid = torch.randn(BATCH, 32, cs.R, cs.R, cs.R, generator=g)
    pts = torch.from_numpy(cases.lattice_points(cs.nx, cs.box)).unsqueeze(0).expand(BATCH, -1, -1).contiguous()
    out = {"pts": pts, "grid": grid}
    if cs.extras:
        n = cs.nx ** 3
        feats = torch.randn(N_FINGERS, 32, generator=g)
        ids = torch.full((BATCH, n), 255, dtype=torch.uint8)
        hit = torch.rand(BATCH, n, generator=g) < 0.3
        ids[hit] = torch.randint(0, N_FINGERS, (int(hit.sum()),), generator=g).to(torch.uint8)
        dense = torch.zeros(BATCH, n, 32)
        dense[hit] = feats[ids[hit].long()]
        out.update(ids=ids, feats=feats, c_img=dense)
    return out


_WEIGHTS = {}


def _sample_lattice(grid, idx, w):
    """decode_train_ref.sample where every scene has the same points: idx, w [N,8] of one scene, grid [B,C,R,R,R] -> [B,N,C] in the dtype
    of ``w``.  The same products summed in the same order, so the same bits; whole rows are picked instead of gathered by element."""
    B, C = grid.shape[:2]
    gcl = grid.permute(0, 2, 3, 4, 1).reshape(B, -1, C).to(w.dtype)
    out = torch.zeros(B, idx.shape[0], C, dtype=w.dtype)
    for k in range(8):
        out = out + w[:, k:k + 1] * gcl.index_select(1, idx[:, k])
    return out


@functools.lru_cache(maxsize=1)
def _features(case_index):
    """What the weight sets share: the sampled features c in float64 and float32 and c's magnitude sums (sum_k |w_k grid_k|).  The
    lattice is the same in every scene, so the corner indices and weights are made for one."""
    cs, inp = CASES[case_index], inputs(case_index)
    out = []
    for dt in (torch.float64, torch.float32):
        idx, w = (t[0] for t in ref.trilinear(inp["pts"][:1], cs.R, cs.padding, dt))
        out.append(_sample_lattice(inp["grid"], idx, w))
        if dt == torch.float64:
            out.append(_sample_lattice(inp["grid"].abs(), idx, w))
    return out[0], out[2], out[1]


@functools.lru_cache(maxsize=None)
def references(case_index, wname, form="plain"):
    """Computed once per (case, weight set, form in "plain" / "img" / "contact") and shared: {"ref64", "ref32", "bound", "bf16x3", "f16x3"}
    -- logits [B,nx^3] of forward64, forward32 and forward_bound, and [1,nx^3] of the two split models on scene 0 (e_split, a maximum,
    is taken there: over fewer points it is never the larger one); with "contact" each is the pair (occupancy, contact).  Nothing that
    receives them changes them."""
    if not _WEIGHTS:
        _WEIGHTS.update(weight_sets())
    sd, cs, inp = _WEIGHTS[wname], CASES[case_index], inputs(case_index)
    ci = inp["c_img"] if form == "img" else None
    c64, c32, cb = _features(case_index)
    args = (sd, inp["pts"], None, ci, form == "contact")
    out = {"ref64": ref.forward64(*args, c64)[0], "ref32": ref.forward32(*args, c32)[0], "bound": ref.forward_bound(*args, c64, cb=cb)[0]}
    for kind in ("bf16x3", "f16x3"):
        out[kind] = forward_split64(sd, inp["pts"][:1], None, kind, None if ci is None else ci[:1], form == "contact", cs.padding, c=c64[:1])
    return out
