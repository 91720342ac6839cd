"""Seeded inputs and the case tables of the wide decoder's float64 suite (CPU only; tests/test_decode_wide_f64_gpu.py runs them,
tests/test_decode_wide_ref_cpu.py asserts what they claim):

* ``weights(H, C, nb)``: a seeded state dict in the style of decode_train_cases.weight_sets()["half"] at any width -- pre-activations
  negative about half of the time, fc_1 / fc_c gains that keep the residual stream from growing over eight blocks, a clear share of
  negative net_final entries for ``leaky``, both input layers (fc_p, fc_p_img) and both heads;
* ``make_points``: decode_train_cases.make_points' families plus a TIE family for sample_mode 'nearest' -- float32 coordinates whose
  float32 grid coordinate is exactly k + 0.5 -- and no other coordinate within 2^-16 of a half-integer grid coordinate: every point
  has one voxel whatever the last bit of the kernel's coordinate, so no point is excluded from any gate;
* ``expected_form``: the launchers' rule (decode_wide.hip wide_form), restated;
* the case tables, each entry with the regime it is meant for.
"""
import functools
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_train_cases as cases
from decode_train_ref import divisor

F32 = np.float32
TIE_CLEAR = 2.0 ** -16
KNOBS = ("VTACO_WIDE_PIPE", "VTACO_WIDE_NG3")


# ---- weights -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(H, C, nb, seed=0):
    gen = torch.Generator().manual_seed(4321 + 1000003 * seed + 7919 * H + 31 * C + nb)
    shapes = [("fc_p", H, 3), ("fc_p_img", H, 3 + C)]
    shapes += [(f"fc_c.{i}", H, C) for i in range(nb)]
    for i in range(nb):
        shapes += [(f"blocks.{i}.fc_0", H, H), (f"blocks.{i}.fc_1", H, H)]
    shapes += [("fc_out", 1, H), ("fc_out_contact", 1, H)]
    sd = {}
    for name, o, k in shapes:
        gain = 0.45 if (".fc_1" in name or name.startswith("fc_c.")) else 1.0          # keeps the residual stream from growing block by block
        sd[name + ".weight"] = torch.randn(o, k, generator=gen) * (gain / float(k) ** 0.5)
        sd[name + ".bias"] = 0.05 * torch.randn(o, generator=gen)
    return sd


# ---- points ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_values(R, padding=0.1):
    """Per k = 0 .. R - 2, a float32 coordinate whose float32 grid coordinate is exactly k + 0.5 (searched among the neighbours of the
    real-valued preimage, as decode_train_cases.node_values searches the nodes); half-integers without one are left out."""
    out = []
    d = divisor(padding)
    for k in range(R - 1):
        v0 = F32(((k + 0.5) / (R - 1) - 0.5) * d)
        cand = [v0]
        lo = hi = v0
        for _ in range(64):
            lo, hi = np.nextafter(lo, F32(-1)), np.nextafter(hi, F32(1))
            cand += [lo, hi]
        hit = [v for v in cand if float(cases.grid_coord32(v, R, padding)) == k + 0.5]
        if hit:
            out.append(hit[0])
    return np.array(out, F32)


def half_distance(p, R, padding=0.1):
    """|frac(f) - 0.5| of the float32 grid coordinate f of every coordinate (float64 array): 0 at an exact tie."""
    f = cases.grid_coord32(p, R, padding).astype(np.float64)
    return np.abs(f - np.floor(f) - 0.5)


def is_tie(p, R, padding=0.1):
    return half_distance(p, R, padding) == 0.0


def make_points(B, N, R, seed=0, padding=0.1):
    """float32 [B,N,3]: decode_train_cases.make_points, then every coordinate closer than 2^-16 to a half-integer grid coordinate is
    moved by 2^-9 (the same value to the same place: duplicates stay duplicates), then every sixth point (the uniform family's slots
    of the small totals) gets one to three of its coordinates from the tie family."""
    pts = cases.make_points(B, N, R, seed, padding).numpy().reshape(-1, 3).copy()
    for _ in range(4):
        near = half_distance(pts, R, padding) < TIE_CLEAR
        if not near.any():
            break
        pts[near] = (pts[near] + F32(2.0 ** -9)).astype(F32)
    ties = tie_values(R, padding)
    rng = np.random.RandomState(77 + 13 * R + B * N + seed)
    if len(ties):
        for i in range(5, B * N, 6):
            axes = rng.permutation(3)[:rng.randint(1, 4)]
            pts[i, axes] = ties[rng.randint(0, len(ties), size=len(axes))]
    d = half_distance(pts, R, padding)
    assert bool(np.all((d == 0.0) | (d >= TIE_CLEAR)))
    return torch.from_numpy(pts.reshape(B, N, 3))


@functools.lru_cache(maxsize=8)
def make_inputs(B, N, R, C, seed=0):
    """{"pts", "grid" [B,C,R,R,R], "c_img" [B,N,C] (about 40 % of the rows set), "c" [B,N,C] (features given directly), "grad_out"
    (every 7th row 0), "grad_out2"}.  Shared: nothing that receives them changes them."""
    g = torch.Generator().manual_seed(100003 * R + 101 * B + N + 17 * C + seed)
    out = {"pts": make_points(B, N, R, seed), "grid": torch.randn(B, C, R, R, R, generator=g)}
    out["c_img"] = torch.randn(B, N, C, generator=g) * (torch.rand(B, N, 1, generator=g) < 0.4)
    out["c"] = torch.randn(B, N, C, generator=g)
    go = torch.randn(B, N, generator=g)
    go.view(-1)[::7] = 0.0
    go2 = torch.randn(B, N, generator=g)
    go2.view(-1)[3::11] = 0.0
    out.update(grad_out=go, grad_out2=go2)
    return out


# ---- the launchers' rule, restated (decode_wide.hip wide_form) --------------------------------------------------------------------------
LDS_BYTES = 160 * 1024
FORM_KEYS = ("waves", "groups", "pairs", "heads_on_c", "tile_points", "grid_cap", "pipeline")


def _atoi(text):
    m = re.match(r"\s*[+-]?\d+", text)
    return int(m.group()) if m else 0


def expected_form(H, C, nb, kind="f32", tactile=False, workspace=False, cus=256, env=None):
    """The launch shape of a wide decode as a dict of FORM_KEYS plus "pairs_asked" (None: the launcher refuses).  Exact f32: one 32-row
    block per wave, four waves up to 128 wide and eight above -- the forward by hidden, the backward by max(hidden, c_dim) --, tiles of 32
    points, at most 8 workgroups per CU.  Split f16: 64 / 32 / <= 5 without tactile columns on given features is the pipeline (2 nb + 2
    waves, one workgroup per CU); otherwise two 32-point groups per wave and as many sets of them as the waves a narrow layer leaves over
    can take (waves / (H / 32), at most 4) while planes + heads stay within 150 KiB; three groups per wave where an eight-wave workgroup
    with one set fits its planes in 160 KiB and its heads in the c planes -- there the heads lie over the c planes (heads_on_c) when
    planes + heads exceed 160 KiB; at most 4 workgroups per CU."""
    env = os.environ if env is None else env
    p_in = 3 + C if tactile else 3
    f = dict(waves=4, groups=1, pairs=1, pairs_asked=1, heads_on_c=0, tile_points=32, grid_cap=8 * cus, pipeline=0)
    if kind == "f32":
        f["waves"] = 4 if H <= 128 else 8
        return f
    if kind == "bwd":
        f["waves"] = 4 if max(H, C) <= 128 else 8
        return f
    assert kind == "f16x3"
    pipe_off = env.get("VTACO_WIDE_PIPE", "1")[:1] == "0"
    if workspace and not pipe_off and H == 64 and C == 32 and 1 <= nb <= 5 and p_in == 3:
        f.update(waves=2 * nb + 2, grid_cap=cus, pipeline=1)
        return f
    Kp = (p_in + 15) // 16 * 16
    waves = 4 if H <= 128 else 8
    wid = max(H, Kp)
    pitch = lambda ch: 2 * ch + 16
    planes = lambda gp, n: 2 * gp * n * pitch(C) + 2 * gp * n * pitch(wid)
    heads = lambda gp: waves * 2 * 2 * gp * 4
    asked = npair = min(4, max(1, waves // (H // 32)))
    ng3_off = "VTACO_WIDE_NG3" in env and _atoi(env["VTACO_WIDE_NG3"]) == 0
    ng3 = waves == 8 and npair == 1 and not ng3_off and planes(96, 1) <= LDS_BYTES and heads(96) <= 2 * 96 * pitch(C)
    gp = 96 if ng3 else 64
    while npair > 1 and planes(gp, npair) + heads(gp) > 150 * 1024:
        npair -= 1
    on_c = int(ng3 and planes(gp, npair) + heads(gp) > LDS_BYTES)
    if planes(gp, npair) + (0 if on_c else heads(gp)) > LDS_BYTES:
        return None
    f.update(waves=waves, groups=3 if ng3 else 2, pairs=npair, pairs_asked=asked, heads_on_c=on_c, tile_points=gp * npair, grid_cap=4 * cus)
    return f


def form_tuple(f):
    """(waves, NG, pairs asked, pairs kept, heads_on_c, points per tile)."""
    return (f["waves"], f["groups"], f["pairs_asked"], f["pairs"], f["heads_on_c"], f["tile_points"])


# ---- the case tables -----------------------------------------------------------------------------------------------------------------
# exact-f32 forward / training forward / backward: (hidden, c_dim, blocks, forward waves, backward waves, what it reaches)
F32_SHAPES = [
    (32, 32, 1, 4, 4, "4 waves, three idle"),
    (128, 128, 2, 4, 4, "4 waves, full"),
    (160, 32, 1, 8, 8, "8 waves, three idle"),
    (256, 128, 5, 8, 8, "the reference default"),
    (32, 160, 2, 4, 8, "backward at 8 waves because of c_dim, nc > nh"),
    (32, 64, 1, 4, 4, "with tactile concat Kp = 72 > hidden: buffer A sized by Kp"),
    (64, 96, 8, 4, 4, "the block limit"),
]
# (B, N, R): B N from {1, 31, 33, 3 x 11, 2 x 333, 1 023}, R from {2, 5, 8}; 3 x 11 and 2 x 333 have tiles that straddle scenes
F32_TOTALS = [(1, 1, 2), (1, 31, 2), (1, 33, 5), (3, 11, 8), (2, 333, 5), (1, 1023, 8)]
F32_FORMS = ("plain", "img", "contact", "mlp")       # mlp: the features given directly (decode_mlp_*), bilinear tests only

# split-f16 streaming forward: one shape per launch form -- (waves, NG, pairs asked, pairs kept, heads_on_c, points per tile) and the
# (hidden, c_dim, tactile, blocks) that takes it; the last: the tactile concat moves 160 / 224 from NG = 3 to NG = 2
F16_SHAPES = [
    ((4, 2, 1, 1, 0, 64), (96, 32, False, 2)),
    ((4, 2, 2, 1, 0, 64), (64, 224, False, 1)),
    ((4, 2, 2, 2, 0, 128), (64, 64, False, 2)),
    ((4, 2, 4, 1, 0, 64), (32, 256, False, 1)),
    ((4, 2, 4, 2, 0, 128), (32, 160, False, 1)),
    ((4, 2, 4, 3, 0, 192), (32, 128, False, 2)),
    ((4, 2, 4, 4, 0, 256), (32, 32, False, 5)),
    ((8, 2, 1, 1, 0, 64), (160, 256, False, 1)),
    ((8, 3, 1, 1, 0, 96), (160, 32, False, 2)),
    ((8, 3, 1, 1, 1, 96), (256, 128, False, 5)),
    ((8, 2, 1, 1, 0, 64), (160, 224, True, 1)),
]
TEN_FORMS = sorted({t for t, _ in F16_SHAPES})


def f16_totals(tile):
    """Point totals relative to the tile: one point; one 32-point group minus 1; tile + 1; 3 tiles - 1."""
    return [1, 31, tile + 1, 3 * tile - 1]


PIPE_BLOCKS = (1, 5)                                  # 64 / 32: the register-resident pipeline

# more tiles than workgroups: (kernel, hidden, c_dim, blocks); totals of loop_total(form)
LOOP_SHAPES = [("f32", 32, 32, 1), ("f32", 160, 32, 1), ("bwd", 32, 32, 1), ("bwd", 32, 160, 1), ("f16x3", 128, 32, 1), ("f16x3", 160, 32, 1)]


def loop_total(form):
    return form["tile_points"] * form["grid_cap"] + form["tile_points"] + 17


def loop_tiles(total, form):
    """The tiles whose points the loop cases gate: the first, cap - 1, cap, cap + 1 (the end of the first trip and the start of the
    second), and the last two (the last one ragged)."""
    tile, cap = form["tile_points"], form["grid_cap"]
    ntiles = (total + tile - 1) // tile
    assert ntiles == cap + 2
    return sorted({0, cap - 1, cap, cap + 1, ntiles - 2, ntiles - 1})


def tile_points(total, form, tiles):
    tile = form["tile_points"]
    return torch.cat([torch.arange(t * tile, min((t + 1) * tile, total)) for t in tiles])
