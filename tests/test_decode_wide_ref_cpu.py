"""CPU: what tests/test_decode_wide_f64_gpu.py stands on -- tests/decode_wide_ref.py is the 32/32 training reference at its shape, its
backward is autograd's through its own forward in every form, its float32 forward is the oracle's decoder, the reference project's own
outputs (g16_decode_wide.npz) lie within the gate of its float64 forward; tests/decode_wide_cases.py's tie family holds exact ties and
the nearest rule is F.grid_sample's, the restated launch rule yields the ten split-f16 forms of the case table, and the weight sets
have the sign balance they claim."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_train_cases as tcases
import decode_train_ref as tref
import decode_wide_cases as wc
import decode_wide_ref as wref
from conftest import load_golden

NO_KNOBS = {}
GATE = 8.0


def test_at_32_32_5_it_is_the_training_reference_exactly():
    sd = wc.weights(32, 32, 5)
    inp = wc.make_inputs(2, 333, 5, 32)
    for c_img, contact in ((None, False), (inp["c_img"], False), (None, True)):
        go2 = inp["grad_out2"] if contact else None
        out_w, sv_w = wref.forward64(sd, inp["pts"], inp["grid"], c_img, contact)
        out_t, sv_t = tref.forward64(sd, inp["pts"], inp["grid"], c_img, contact)
        for a, b in zip(out_w if contact else (out_w,), out_t if contact else (out_t,)):
            assert torch.equal(a, b)
        # slot orders: wide c | a0_0 a1_0 a0_1 a1_1 ... | af; training c | relu(x_0..4) | relu(h_0..4) | relu(net_5)
        assert torch.equal(sv_w[0], sv_t[0]) and torch.equal(sv_w[-1], sv_t[11])
        for i in range(5):
            assert torch.equal(sv_w[1 + 2 * i], sv_t[1 + i]) and torch.equal(sv_w[2 + 2 * i], sv_t[6 + i])
        bo_w, bd_w = wref.forward_bound(sd, inp["pts"], inp["grid"], c_img, contact)
        bo_t, bd_t = tref.forward_bound(sd, inp["pts"], inp["grid"], c_img, contact)
        for a, b in zip(bo_w if contact else (bo_w,), bo_t if contact else (bo_t,)):
            assert torch.equal(a, b)
        assert torch.equal(bd_w[1], bd_t[1]) and torch.equal(bd_w[2], bd_t[6]) and torch.equal(bd_w[-1], bd_t[11])
        (g_w, b_w), (g_t, b_t) = (m.backward64(sd, inp["pts"], inp["grid"].shape, s, inp["grad_out"], go2, c_img) for m, s in ((wref, sv_w), (tref, sv_t)))
        for got, want in ((g_w, g_t), (b_w, b_t)):
            for k, v in want.items():
                assert torch.equal(got[k], v), k
        assert set(g_w) - set(g_t) == {"rows.dN", "rows.dH"}


FORMS = [(H, C, nb, leaky, nearest, form) for H, C, nb in ((32, 32, 1), (64, 96, 3), (160, 32, 2))
         for leaky in (False, True) for nearest in (False, True) for form in ("plain", "img", "contact", "mlp") if not (form == "mlp" and nearest)]


@pytest.mark.parametrize("H,C,nb,leaky,nearest,form", FORMS)
def test_backward64_is_autograd_through_forward64(H, C, nb, leaky, nearest, form):
    sd0 = wc.weights(H, C, nb)
    inp = wc.make_inputs(3, 11, 5, C)
    B, N, R = 3, 11, 5
    img, contact, mlp = form == "img", form == "contact", form == "mlp"
    sd = {k: v.double().requires_grad_(True) for k, v in sd0.items()}
    grid = inp["grid"].double().requires_grad_(True)
    c_img = inp["c_img"].double().requires_grad_(True) if img else None
    c = inp["c"].double().requires_grad_(True) if mlp else None
    out, saves = wref.forward(sd, inp["pts"], None if mlp else grid, c_img, contact, c, leaky=leaky, nearest=nearest)
    go, go2 = inp["grad_out"].double(), inp["grad_out2"].double()
    ((out[0] * go).sum() + (out[1] * go2).sum() if contact else (out * go).sum()).backward()
    if leaky:
        assert float((saves[-1] < 0).double().mean()) > 0.2
    g = wref.backward(sd0, inp["pts"], None if mlp else grid.shape, [s.detach() for s in saves], go, go2 if contact else None,
                      inp["c_img"] if img else None, leaky=leaky, nearest=nearest)

    def close(got, want, tag):
        err, top = float((got - want).abs().max()), float(want.abs().max())
        assert err <= 1e-12 * max(top, 1e-300), (tag, err, top)
    first = "fc_p_img" if img else "fc_p"
    close(g["fc_p.weight"], sd[first + ".weight"].grad, "fc_p.weight")
    close(g["fc_p.bias"], sd[first + ".bias"].grad, "fc_p.bias")
    for i in range(nb):
        close(g["fc_c.weight"][i], sd[f"fc_c.{i}.weight"].grad, f"fc_c.{i}.weight")
        close(g["fc_c.bias"][i], sd[f"fc_c.{i}.bias"].grad, f"fc_c.{i}.bias")
        for l in ("fc_0", "fc_1"):
            close(g[l + ".weight"][i], sd[f"blocks.{i}.{l}.weight"].grad, f"{l}.{i}.weight")
            close(g[l + ".bias"][i], sd[f"blocks.{i}.{l}.bias"].grad, f"{l}.{i}.bias")
    close(g["fc_out.weight"], sd["fc_out.weight"].grad, "fc_out.weight")
    close(g["fc_out.bias"], sd["fc_out.bias"].grad, "fc_out.bias")
    if contact:
        close(g["fc_out_contact.weight"], sd["fc_out_contact.weight"].grad, "fc_out_contact.weight")
        close(g["fc_out_contact.bias"], sd["fc_out_contact.bias"].grad, "fc_out_contact.bias")
    if mlp:
        close(g["grad_c"], c.grad, "grad_c")
        assert g["grad_grid"] is None
    else:
        close(g["grad_grid"], grid.grad.permute(0, 2, 3, 4, 1), "grad_grid")
    if img:
        close(g["grad_c_img"], c_img.grad, "grad_c_img")
    assert g["rows.dN"].shape == (nb + 1, B, N, H) and g["rows.dH"].shape == (nb, B, N, H)


@pytest.mark.parametrize("H,C,nb,leaky,nearest", [(32, 32, 1, True, False), (256, 128, 5, False, False), (32, 160, 2, True, True), (64, 96, 8, False, True)])
def test_forward32_is_the_oracles_decoder(H, C, nb, leaky, nearest):
    from oracle import vtaco_oracle as orc
    sd = wc.weights(H, C, nb)
    inp = wc.make_inputs(2, 333, 8, C)
    kw = dict(leaky=leaky, sample_mode="nearest" if nearest else "bilinear")
    rk = dict(leaky=leaky, nearest=nearest)
    pairs = [(wref.forward32(sd, inp["pts"], inp["grid"], **rk)[0], orc.local_decoder_forward(sd, inp["pts"], inp["grid"], **kw)),
             (wref.forward32(sd, inp["pts"], inp["grid"], inp["c_img"], **rk)[0], orc.local_decoder_forward_img(sd, inp["pts"], inp["grid"], inp["c_img"], **kw))]
    ours, theirs = wref.forward32(sd, inp["pts"], inp["grid"], None, True, **rk)[0], orc.local_decoder_forward_contact(sd, inp["pts"], inp["grid"], **kw)
    pairs += list(zip(ours, theirs))
    for got, want in pairs:
        err, top = float((got - want).abs().max()), float(want.abs().max())
        print(f"{H}/{C}/{nb}: max |forward32 - oracle| = {err:.3e} (logits up to {top:.2f})")
        assert err <= 1e-5 * max(1.0, top)                          # float32 rounding over the layer widths, summation order only


@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_the_reference_projects_logits_lie_within_the_gate_of_forward64(tag):
    a, sd = load_golden("g16_decode_wide.npz")
    arrs = {k[2:]: v for k, v in a.items() if k.startswith(tag + ".")}
    sd = {k[2:]: v.float() for k, v in sd.items() if k.startswith(tag + ".")}
    H, C, nb, leaky, nx, nearest = (int(x) for x in arrs["shape"])
    assert wref.n_blocks(sd) == nb and sd["fc_p.weight"].shape[0] == H
    T = lambda k: torch.from_numpy(arrs[k].astype(np.float32))
    grid, pts, c_img = T("grid"), T("prand"), T("c_img")
    rk = dict(leaky=bool(leaky), nearest=bool(nearest))
    if nearest:                                                     # the fixture's points were not made for the tie rule: none may be near one
        assert float(wc.half_distance(pts.numpy(), grid.shape[2]).min()) >= wc.TIE_CLEAR
    runs = [("logits", (None, False), None), ("logits_img", (c_img, False), None), ("logits_contact", (None, True), 0), ("logits_contact2", (None, True), 1)]
    for key, (ci, contact), part in runs:
        pick = lambda v: v if part is None else v[part]
        r64 = pick(wref.forward64(sd, pts, grid, ci, contact, **rk)[0])
        r32 = pick(wref.forward32(sd, pts, grid, ci, contact, **rk)[0])
        bound = pick(wref.forward_bound(sd, pts, grid, ci, contact, **rk)[0])
        ratio, e32 = wref.gate_ratio(T(key), r64, r32, bound)
        print(f"RATIO g16 {tag} {key}: {ratio:.3f} (e32 {e32:.3e})")
        assert ratio <= GATE


@pytest.mark.parametrize("R", [2, 5, 8])
def test_the_tie_family_holds_exact_ties_and_nearest_is_grid_samples(R):
    ties = wc.tie_values(R)
    assert len(ties) >= 1 and np.all(wc.is_tie(ties, R))
    if R == 8:
        f = tcases.grid_coord32(ties, R)
        assert set(f.tolist()) >= {2.5, 3.5, 4.5, 5.5}              # both parities of k: half-to-even and half-away differ on every other one
    pts = wc.make_points(2, 4000, R, seed=3)
    tie = wc.is_tie(pts.numpy(), R)
    n_tie = int(tie.any(-1).sum())
    print(f"R = {R}: {n_tie} of {pts.shape[0] * pts.shape[1]} points have an exactly tied coordinate")
    assert n_tie >= 1000
    d = wc.half_distance(pts.numpy(), R)
    assert np.all((d == 0.0) | (d >= wc.TIE_CLEAR))
    # the rule against torch's own nearest sampling of a grid that holds its voxel index
    grid = torch.arange(R ** 3, dtype=torch.float32).view(1, 1, R, R, R).expand(2, 1, R, R, R)
    q = torch.from_numpy(tcases.norm32(pts.numpy()))
    vgrid = (2.0 * q - 1.0)[:, :, None, None]
    want = F.grid_sample(grid, vgrid, mode="nearest", padding_mode="border", align_corners=True).view(2, -1).long()
    assert torch.equal(wref.nearest_voxel(pts, R), want)
    away = np.floor(tcases.grid_coord32(pts.numpy(), R).astype(np.float64) + 0.5).astype(np.int64)          # round half away: another voxel
    away = torch.from_numpy((away[..., 2] * R + away[..., 1]) * R + away[..., 0])
    assert int((away != want).sum()) >= (100 if R > 2 else 0) or R == 2


def test_the_restated_rule_yields_the_ten_split_f16_forms():
    seen = {}
    for tactile in (False, True):
        for H in range(32, 257, 32):
            for C in range(32, 257, 32):
                f = wc.expected_form(H, C, 1, "f16x3", tactile, env=NO_KNOBS)
                assert f is not None, (H, C, tactile)
                seen.setdefault(wc.form_tuple(f), (H, C, tactile))
    assert sorted(seen) == wc.TEN_FORMS and len(wc.TEN_FORMS) == 10
    for want, (H, C, tactile, nb) in wc.F16_SHAPES:
        assert wc.form_tuple(wc.expected_form(H, C, nb, "f16x3", tactile, env=NO_KNOBS)) == want, (H, C, tactile)
    # the tactile concat moves 160 / 224 from three groups per wave to two
    assert wc.form_tuple(wc.expected_form(160, 224, 1, "f16x3", False, env=NO_KNOBS))[:2] == (8, 3)
    # the knobs, the pipeline and the exact-f32 kernels
    assert wc.expected_form(256, 128, 5, "f16x3", env={"VTACO_WIDE_NG3": "0"})["groups"] == 2
    pipe = wc.expected_form(64, 32, 5, "f16x3", workspace=True, env=NO_KNOBS)
    assert pipe["pipeline"] == 1 and pipe["waves"] == 12 and pipe["grid_cap"] == 256 and pipe["tile_points"] == 32
    for kw in (dict(workspace=False), dict(workspace=True, tactile=True), dict(workspace=True, env={"VTACO_WIDE_PIPE": "0"})):
        assert wc.expected_form(64, 32, 5, "f16x3", **{"env": NO_KNOBS, **kw})["pipeline"] == 0
    assert wc.expected_form(64, 32, 6, "f16x3", workspace=True, env=NO_KNOBS)["pipeline"] == 0
    for H, C, nb, fw, bw, _ in wc.F32_SHAPES:
        assert wc.expected_form(H, C, nb, "f32")["waves"] == fw and wc.expected_form(H, C, nb, "bwd")["waves"] == bw
    assert {(k, H, C) for k, H, C, _ in wc.LOOP_SHAPES} == {("f32", 32, 32), ("f32", 160, 32), ("bwd", 32, 32), ("bwd", 32, 160), ("f16x3", 128, 32), ("f16x3", 160, 32)}
    for kind, H, C, nb in wc.LOOP_SHAPES:
        f = wc.expected_form(H, C, nb, kind, env=NO_KNOBS)
        total = wc.loop_total(f)
        assert 65000 < total < 99000 and wc.loop_tiles(total, f)[-1] == f["grid_cap"] + 1


def test_the_library_answers_the_form_query_as_the_rule_does():
    """vt_decode_wide_form is host code: every width, with and without the tactile concat and the pipeline's inputs, without a GPU."""
    if any(k in os.environ for k in wc.KNOBS):
        pytest.skip("the wide decode's form is forced by an A/B knob of the environment")
    from vtaco_amd import ops
    cus = ops.decode_wide_form(32, 32, 1, "f16x3")["grid_cap"] // 4
    for kind in ops.WIDE_KINDS:
        for tactile in (False, True):
            for workspace in (False, True):
                for H in range(32, 257, 32):
                    for C in range(32, 257, 32):
                        for nb in (1, 5, 6):
                            want = wc.expected_form(H, C, nb, kind, tactile, workspace, cus, env=NO_KNOBS)
                            got = ops.decode_wide_form(H, C, nb, kind, tactile, workspace=workspace)
                            assert got == {k: want[k] for k in wc.FORM_KEYS}, (kind, H, C, nb, tactile, workspace, got, want)
    for bad in ((48, 32, 1), (32, 288, 1), (32, 32, 9)):
        with pytest.raises(ops.VtError):
            ops.decode_wide_form(*bad)


@pytest.mark.parametrize("H,C,nb", sorted({(H, C, nb) for H, C, nb, *_ in wc.F32_SHAPES} | {(H, C, nb) for _, (H, C, _, nb) in wc.F16_SHAPES}
                                         | {(64, 32, nb) for nb in wc.PIPE_BLOCKS} | {(H, C, nb) for _, H, C, nb in wc.LOOP_SHAPES}))
def test_every_weight_set_has_the_sign_balance_it_claims(H, C, nb):
    sd = wc.weights(H, C, nb)
    assert wref.n_blocks(sd) == nb and sd["fc_p_img.weight"].shape == (H, 3 + C) and sd["fc_out_contact.weight"].shape == (1, H)
    inp = wc.make_inputs(2, 333, 8, C)
    for c_img in (None, inp["c_img"]):
        _, saves = wref.forward64(sd, inp["pts"], inp["grid"], c_img, leaky=True)
        for k, s in enumerate(saves[1:-1]):
            share = float((s > 0).double().mean())
            assert 0.3 < share < 0.7, (k, share)                    # pre-activations negative about half of the time
        neg = float((saves[-1] < 0).double().mean())
        assert 0.3 < neg < 0.7, neg                                  # a clear share of negative net_final entries for leaky
        stream = float(saves[-1].abs().max())
        assert stream < 20.0, stream                                 # the residual stream does not grow over the blocks
