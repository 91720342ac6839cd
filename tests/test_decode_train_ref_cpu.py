"""CPU: the float64 reference of the decoder's training path (tests/decode_train_ref.py) is pinned against torch.autograd and the
reference-made golden g8, and the seeded inputs prepared for the GPU tests of the kernels (tests/decode_train_cases.py) are shown to
hold the edges they claim, so a test built on them cannot pass vacuously."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden, sub_sd
import decode_train_cases as cases
import decode_train_ref as ref

T = torch.from_numpy
PARAM_KEYS = ("fc_p.weight", "fc_p.bias", "fc_c.weight", "fc_c.bias", "fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias",
              "fc_out.weight", "fc_out.bias")


def _module_name(key, i, img):
    if key.startswith("fc_p."):
        return ("fc_p_img." if img else "fc_p.") + key[5:]
    if key.startswith("fc_c."):
        return f"fc_c.{i}." + key[5:]
    if key.startswith(("fc_0.", "fc_1.")):
        return f"blocks.{i}." + key
    return key


def _by_module(grads, img):
    """The reference's stacked gradients under the module's parameter names."""
    out = {}
    for k, v in grads.items():
        if k.startswith("grad_") or v is None:
            continue
        if v.dim() >= 2 and v.shape[0] == ref.NB and k.split(".")[0] in ("fc_c", "fc_0", "fc_1"):
            for i in range(ref.NB):
                out[_module_name(k, i, img)] = v[i]
        else:
            out[_module_name(k, None, img)] = v
    return out


def _plain_forward64(sd, pts, grid, c_img, contact, padding=0.1):
    """The module in float64 from torch's own operators (F.grid_sample, F.linear): what autograd differentiates."""
    q = pts.double() / ref.divisor(padding) + 0.5
    q = torch.where(q >= 1, torch.full_like(q, ref.Q_HI), q)
    q = torch.where(q < 0, torch.zeros_like(q), q)
    vg = (2 * q - 1)[:, :, None, None, :]
    c = F.grid_sample(grid, vg, padding_mode="border", align_corners=True, mode="bilinear").squeeze(-1).squeeze(-1).transpose(1, 2)
    c.retain_grad()
    lin = lambda n, x: F.linear(x, sd[n + ".weight"], sd[n + ".bias"])
    net = lin("fc_p_img", torch.cat((pts.double(), c_img), 2)) if c_img is not None else lin("fc_p", pts.double())
    for i in range(ref.NB):
        net = net + lin(f"fc_c.{i}", c)
        net = net + lin(f"blocks.{i}.fc_1", F.relu(lin(f"blocks.{i}.fc_0", F.relu(net))))
    a = F.relu(net)
    out = lin("fc_out", a).squeeze(-1)
    return (out, lin("fc_out_contact", a).squeeze(-1) if contact else None), c


@pytest.mark.parametrize("B,N,R", [(2, 37, 5), (1, 64, 3)])
@pytest.mark.parametrize("form", ["plain", "c_img", "contact"])
@pytest.mark.parametrize("wset", ["g1", "half"])
def test_backward64_equals_autograd_of_a_plain_float64_forward(B, N, R, form, wset):
    sd = cases.weight_sets()[wset]
    x = cases.make_inputs(B, N, R)
    img, contact = form == "c_img", form == "contact"
    c_img = x["c_img"] if img else None
    logits, saves = ref.forward64(sd, x["pts"], x["grid"], c_img, contact)
    assert len(saves) == 12 and all(s.shape == (B, N, 32) and s.dtype == torch.float64 for s in saves)
    go2 = x["grad_out2"] if contact else None
    g, bound = ref.backward64(sd, x["pts"], x["grid"].shape, saves, x["grad_out"], go2, c_img)
    # autograd
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    grid = x["grid"].double().requires_grad_(True)
    ci = c_img.double().requires_grad_(True) if img else None
    (o, o2), c = _plain_forward64(leaves, x["pts"], grid, ci, contact)
    lo = (logits[0] if contact else logits)
    assert float((o.detach() - lo).abs().max()) <= 1e-12 * float(ref.forward_bound(sd, x["pts"], x["grid"], c_img)[0].max())
    loss = (o * x["grad_out"].double()).sum()
    if contact:
        assert float((o2.detach() - logits[1]).abs().max()) <= 1e-12 * float(ref.forward_bound(sd, x["pts"], x["grid"], None, True)[0][1].max())
        loss = loss + (o2 * go2.double()).sum()
    loss.backward()
    assert float((saves[0] - c.detach()).abs().max()) <= 1e-13 * float(x["grid"].abs().max())

    def close(name, got, want, bnd):
        err = (got - want).abs()
        assert bool((err <= 1e-10 * bnd + 1e-300).all()), (name, float(err.max()), float(bnd.max()))
    close("grad_grid", g["grad_grid"], grid.grad.permute(0, 2, 3, 4, 1), bound["grad_grid"])
    close("grad_c", g["grad_c"], c.grad, bound["grad_c"])
    if img:
        close("grad_c_img", g["grad_c_img"], ci.grad, bound["grad_c_img"])
    mine, mb = _by_module(g, img), _by_module(bound, img)
    assert ("fc_out_contact.weight" in mine) == contact
    for name, leaf in leaves.items():
        if leaf.grad is None:
            assert name not in mine, name
            continue
        close(name, mine[name], leaf.grad, mb[name])
    assert len(mine) == (36 if contact else 34)
    # float32 and the magnitude sums are the same function: e32 is small against the bound, the bound dominates the value
    g32 = ref.backward32(sd, x["pts"], x["grid"].shape, saves, x["grad_out"], go2, c_img)
    for k in g:
        if g[k] is None:
            continue
        assert bool((g[k].abs() <= bound[k] * (1 + 1e-12) + 1e-300).all()), k
        assert float((g32[k].double() - g[k]).abs().max()) <= 64 * 2.0 ** -24 * float(bound[k].max()), k


def test_reference_reproduces_the_reference_made_golden_g8():
    """The tolerances of tests/test_train_gpu.py, applied to forward64 / backward64 on the golden's own inputs."""
    from oracle import vtaco_oracle as orc
    a, sd = load_golden("g8_trainstep.npz")
    dsd = sub_sd(sd, "dec.")
    with torch.no_grad():
        grid = orc.pointnet_encoder_forward(sub_sd(sd, "enc."), T(a["p_in"]), 16, unet3d=False)
    if isinstance(grid, dict):
        grid = grid["grid"]
    pq, occ, c_img = T(a["pq"]), T(a["occ"]), T(a["c_img"])

    def close(got, want, name, rel=2e-4, floor=2e-6):
        err = float((got.double() - torch.as_tensor(want).double()).abs().max())
        tol = floor + rel * float(np.abs(want).max())
        assert err <= tol, f"{name}: {err} > {tol}"
    for img in (True, False):
        ci = c_img if img else None
        logits, saves = ref.forward64(dsd, pq, grid, ci)
        loss = float((logits - occ.double()).abs().mean())
        assert abs(loss - float(a["loss"] if img else a["loss_v"])) <= 1e-6
        go = torch.sign(logits - occ.double()) / occ.numel()
        g, _ = ref.backward64(dsd, pq, grid.shape, saves, go, None, ci)
        by = _by_module(g, img)
        pre = "g.dec." if img else "gv."
        for name, v in by.items():
            close(v, a[pre + name], pre + name)
        unused = "fc_p." if img else "fc_p_img."
        assert all(not a[pre + unused + s].any() for s in ("weight", "bias"))
        if img:
            close(logits, a["logits"], "logits", rel=0, floor=1e-4)
            close(g["grad_c_img"], a["c_img_grad"], "c_img_grad", rel=1e-4, floor=1e-8)
            gi = a["grid_grad_idx"].astype(np.int64)
            gg = g["grad_grid"].reshape(2, -1, 32)
            # the golden holds the gradient that reached the grid through the decoder alone (the grid is a retained non-leaf)
            close(gg[gi[:, 0], gi[:, 1]], a["grid_grad_val"], "grid.grad", rel=1e-4, floor=1e-8)
            mask = torch.ones(2, 16 ** 3, dtype=torch.bool)
            mask[gi[:, 0], gi[:, 1]] = False
            assert float(gg[mask].abs().max()) == 0.0


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------
BIG = [(B, N) for B, N in cases.TOTALS if B * N >= 600]


@pytest.mark.parametrize("R", cases.RS)
def test_point_sets_hold_the_edges_they_claim(R):
    """Totals of 600 points and more carry every family whole (>= 32 on nodes, >= 32 beyond the box on both sides of each axis,
    +-divisor/2, 8 x 8 duplicates, 200 points in one cell).  The small totals take the families in turn, so (1, 31) and (3, 11) hold
    at least five points of each and (1, 1) one cluster point: they are there for the tile and scene-boundary edges."""
    d = ref.divisor()
    nodes = cases.node_values(R)
    assert len(nodes) >= min(R - 1, 4) and all(float(cases.grid_coord32(v, R)) == round(float(cases.grid_coord32(v, R))) for v in nodes)
    for B, N in BIG:
        p = cases.make_points(B, N, R).numpy()
        assert p.shape == (B, N, 3) and p.dtype == np.float32
        f = cases.grid_coord32(p, R)
        raw = cases.raw_norm32(p)
        on_node = (f == np.floor(f)).all(-1) & (raw < 1).all(-1) & (raw >= 0).all(-1)
        assert int(on_node.sum()) >= 32, (B, N, int(on_node.sum()))
        assert int(((raw >= 1) | (raw < 0)).any(-1).sum()) >= 32
        for ax in range(3):
            assert int((raw[..., ax] > 1).sum()) >= 4 and int((raw[..., ax] < 0).sum()) >= 4, ax
            assert (p[..., ax] == np.float32(0.5) * np.float32(d)).any() and (p[..., ax] == -np.float32(0.5) * np.float32(d)).any()
        assert (raw[p == np.float32(0.5) * np.float32(d)] == 1).all() and (raw[p == -np.float32(0.5) * np.float32(d)] == 0).all()
        assert float(np.abs(p).max()) <= 0.5 * d + 0.21 and float(np.abs(p[..., 0]).min()) < 0.62
        cell = np.floor(f).astype(np.int64)
        lin = (cell[..., 2] * R + cell[..., 1]) * R + cell[..., 0]
        most, dups = 0, 0
        for b in range(B):
            most = max(most, int(np.bincount(lin[b]).max()))
            _, cnt = np.unique(p[b], axis=0, return_counts=True)
            dups += int((cnt >= 8).sum())
        assert most >= 200 and dups >= 8, (B, N, most, dups)
        # the float64 reference and the float32 kernels take the same side of both clamps on every coordinate
        q64 = p.astype(np.float64) / d + 0.5
        assert ((q64 >= 1) == (raw >= 1)).all() and ((q64 < 0) == (raw < 0)).all()
    for B, N in cases.TOTALS:
        p = cases.make_points(B, N, R)
        assert p.shape == (B, N, 3) and torch.equal(p, cases.make_points(B, N, R))
        go = cases.make_inputs(B, N, R)["grad_out"]
        assert int((go == 0).sum()) >= 1
        if 6 <= B * N < 600:
            pn = p.numpy().reshape(-1, 3)
            f, raw = cases.grid_coord32(pn, R), cases.raw_norm32(pn)
            inside = ((raw < 1) & (raw >= 0)).all(-1)
            assert int(((f == np.floor(f)).all(-1) & inside).sum()) >= 5 and int((~inside).sum()) >= 5
            assert (np.abs(pn) == np.float32(0.5) * np.float32(d)).any()
            assert int((np.floor(f) == np.array(cases.cluster_cell(R))).all(-1).sum()) >= 5


def test_half_weight_set_has_both_relu_sides_in_every_layer():
    sets = cases.weight_sets()
    x = cases.make_inputs(3, 427, 5)
    for form in ("plain", "c_img"):
        _, saves = ref.forward64(sets["half"], x["pts"], x["grid"], x["c_img"] if form == "c_img" else None)
        for slot in range(1, 12):
            neg = float((saves[slot] == 0).double().mean())
            assert 0.3 <= neg <= 0.7, (form, slot, neg)
    _, saves = ref.forward64(sets["g1"], x["pts"], x["grid"])
    assert all(0.0 < float((saves[s] == 0).double().mean()) < 1.0 for s in range(1, 12))


def _boundary_values(R, ulps):
    """float32 coordinates within ``ulps`` of the preimage of every cell boundary of a grid of resolution R, and a coarse sweep."""
    d = ref.divisor()
    vals = [np.linspace(-0.7, 0.7, 200001).astype(np.float32)]
    for k in range(R):
        v = np.float32((k / (R - 1) - 0.5) * d)
        run = [v]
        lo = hi = v
        for _ in range(ulps):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(1))
            run += [lo, hi]
        vals.append(np.array(run, np.float32))
    return np.concatenate(vals)


@pytest.mark.parametrize("R", [3, 5, 9, 17, 33])
def test_a_voxel_bin_at_R_minus_1_is_the_trilinear_cell(R):
    """Why sample_grid_bwd_sorted_kernel's fallback never runs under ops.decode_bwd: vt_voxel_build at R - 1 bins a coordinate by
    int(q (R - 1)), the scatter takes floor(((2q - 1) + 1) / 2 (R - 1)) with the same float32 q -- the round trip through 2q - 1
    gives q back on every value probed: 200 001 coordinates across the box and beyond it, and +-200 ulps around the preimage of every
    cell boundary."""
    v = _boundary_values(R, 200)
    q = cases.norm32(v)
    g = np.float32(2) * q - np.float32(1)
    assert (((g + np.float32(1)) / np.float32(2)).astype(np.float32) == q).all()
    assert (cases.voxel_bin32(v, R - 1) == np.floor(cases.grid_coord32(v, R)).astype(np.int64)).all()


@pytest.mark.parametrize("R", [2, 3, 5, 8, 9, 16, 17, 32, 33, 64, 128])
def test_the_top_border_corner_is_never_the_base_cell(R):
    """x0 = R - 1 (the corner whose +1 neighbour tri_setup clamps, with weight 0) needs f = R - 1, i.e. q = 1 after the clamps; the
    largest q is 1 - 2^-24 (or 0.999 beyond the box) and float32((1 - 2^-24)(R - 1)) < R - 1 for every R.  The clamp is a guard,
    not a path: no input reaches it, in float32 or float64."""
    qmax = np.nextafter(np.float32(1), np.float32(0))
    g = np.float32(2) * qmax - np.float32(1)
    f = ((g + np.float32(1)) / np.float32(2)) * np.float32(R - 1)
    assert float(f) < R - 1
    v = _boundary_values(R, 200)
    assert int(np.floor(cases.grid_coord32(v, R)).max()) == R - 2
    idx, w = ref.trilinear(T(v).view(1, -1, 1).expand(1, -1, 3), R)
    assert int(idx.max()) <= R ** 3 - 1 and float(w.min()) >= 0.0 and float((w.sum(-1) - 1).abs().max()) <= 1e-12


@pytest.mark.parametrize("nx", [6, 12])
def test_lattice_points_restate_the_query_lattice_bit_for_bit(nx):
    from vtaco_amd.common import make_3d_grid
    want = 1.1 * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (nx,) * 3)
    assert torch.equal(T(cases.lattice_points(nx)), want)
