"""TransformerFusion on the MI355X against the float64 reference of tests/fusion_ref.py, one case per boundary of the kernels
(vtaco_amd/csrc/fusion.hip, fusion_bwd.hip): the 32-point tiles, the 256-row blocks of the forward and the 128-row blocks of the
backward, the half-pair -> f8 switch at 512 points, the cached -> streamed InstanceNorm past 2048, two projection tiles per wave,
the grid-stride regimes of the capped grids (scale-V, the wide epilogue, fb_add, the wide backward's per-point kernels) and the
512-point weight-gradient chunks running over a scene boundary.

Every case first asks ops.fusion_plan (vt_fusion_plan: the launchers' own rule) and asserts that it equals the rule restated in
fusion_ref.expected_plan and that it is the regime the case is listed for; then

    training forward, every d_model > 32 (full form)   |got - ref64| <= 8 max(e32, e_form("full"))        elementwise
    inference, N < 512 (half-pair form)                  the same with e_form("half_pair")
    inference, N >= 512 (f8 form)                        max |got - ref64| <= 5e-5, the contract of tests/test_fusion_gpu.py; the ratio
                                                         to the half-pair floor is printed, not asserted (fp8 corrections: not modelled)
    backward: d c_img, d c, twenty parameter gradients   per tensor rel_err <= 8 max(e32_t, e_full_t), L2-relative, both floors taken
                                                         against float64 autograd of the exact reference

e32: the float32 oracle on the CPU; e_form: the float64 model of the form's operand roundings (straight-through, so e_full_t is its
autograd).  Every floor comes from fusion_ref.py alone; no figure of a kernel entered a case, a seed or a bound.  Every comparison
prints `RATIO <tag>: ...`; the largest of a run on the MI355X are kept in profiles/fusion_f64_ratios.txt.

Repeated cases (two distinct chunks expanded on the device): equal chunks must give equal bits wherever they sit in the batch, the
reference is computed for the distinct chunks, and the parameter gradients are its multiplicity-weighted sums.

What the suite found on the MI355X (40 tests, largest ratios in profiles/fusion_f64_ratios.txt): no kernel defect.  Forward <= 1.9 of
the floor (gate 8), the f8 form <= 0.41 of its 5e-5 (1.1 to 1.6 x the half-pair floor), gradients <= 6.4 (cross.WQ of t-17x2048, its sum
over 17 chunks; <= 4.3 elsewhere).  One thing about the cases rather than the kernels: on 31 to 33 keys the half-pair MODEL's own error
is 3.5e-5 to 8.0e-5 (fusion_ref.RESEEDED), at the edge of the 5e-5 tests/test_fusion_gpu.py states -- the kernel sits at 0.97 to 1.05 of
that model there.  N = 1 gives zeros, as the reference restated here does (documented in ops/fusion.py; last test).

Evidence that the gates bite -- two changes of arithmetic alone, each tried on a scratch copy of the library:
  * the full form without its q_lo . k_hi score product (score_tile): 17 of the 40 tests fail -- every training forward / backward
    case (forward 8.1 to 18.3 x the floor; t-2x128 passes its forward at 7.8 and fails on cross.WK at 14.1) and the four d_model 64
    forwards (8.2 to 11.3); the d_model 128 forwards stay at 5.7 or below and pass.  tests/test_fusion_gpu.py notices in 5 of its 28
    tests, all of them backward comparisons (its forward checks at 5e-5 pass).
  * fusion_inorm_relu_kernel dividing by the padded length instead of N: 14 fail -- i-2x2049 (4.0e3 x its contract) and t-1x2049
    (4.1e4 x the floor), the only d_model 32 cases that run the streamed kernel, and every d_model > 32 case whose N is no multiple
    of 32 (3.2e4 to 6.6e5 x).  tests/test_fusion_gpu.py notices in 6 tests, all at d_model > 32: none of its cases passes N > 2048.
"""
import os

import pytest
import torch

import fusion_ref as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOBS = ("VTACO_FUSION_SCORE_TERMS",)

FWD_CASES = [i for i, c in enumerate(fr.CASES) if c[4] in ("infer", "fwd")]
BWD_CASES = [i for i, c in enumerate(fr.CASES) if c[4] in ("bwd", "drop")]
IDS = lambda idx: [fr.CASES[i][0] for i in idx]


@pytest.fixture(autouse=True)
def _default_dispatch():
    if any(k in os.environ for k in KNOBS):
        pytest.skip("the fuser's score form is forced by an A/B knob of the environment")


def _plan(case, train):
    """The launchers' plan of the case: equal to the restated rule, and the regime the case is listed for."""
    from vtaco_amd import ops
    name, C, B, N, mode, distinct, _w, want = case
    plan = ops.fusion_plan(B, N, C, train)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert plan == fr.expected_plan(B, N, C, train, cus=cus), (name, plan)
    assert {k: plan[k] for k in want} == want, (name, plan, want)
    return plan


def _device_case(i):
    """The module on the device and the case's batch, the distinct chunks expanded there."""
    name, C, B, N, mode, distinct, _w, _want = fr.CASES[i]
    units, c_img, c, wgt = fr.case_inputs(i)
    idx = fr.chunk_index(B, distinct)
    net = fr.module_of(units, C).to(DEV)
    di = idx.to(DEV)
    expand = (lambda t: t.to(DEV)[di].contiguous()) if distinct else (lambda t: t.to(DEV))
    return net, expand(c_img), expand(c), expand(wgt), idx


def _gate_forward(tag, got, r, idx, form):
    """got [B,N,C] on the device against out64 of the distinct chunks."""
    ref = r["out64"].to(DEV)[idx.to(DEV)]
    err = float((got.double() - ref).abs().max())
    assert bool(torch.isfinite(got).all()), tag
    if form == "f8":
        floor = fr.forward_floor(r, "half_pair")
        print(f"RATIO {tag} fwd f8: {err / fr.F8_CONTRACT:.3f} of {fr.F8_CONTRACT} (err {err:.3e}; {err / floor:.2f} x the half-pair floor {floor:.3e}, e32 {r['e32']:.3e})")
        assert err <= fr.F8_CONTRACT, (tag, err)
        return
    floor = fr.forward_floor(r, form)
    print(f"RATIO {tag} fwd {form}: {err / floor:.3f} (floor {floor:.3e}, e32 {r['e32']:.3e})")
    assert err <= fr.GATE * floor, (tag, form, err, floor)


def _equal_chunks_equal_bits(tag, t, idx):
    for d in sorted(set(idx.tolist())):
        rows = t[(idx == d).to(t.device)]
        assert bool((rows == rows[:1]).all()), (tag, d)


@pytest.mark.parametrize("i", FWD_CASES, ids=IDS(FWD_CASES))
def test_inference_forward_vs_float64(i):
    case = fr.CASES[i]
    plan = _plan(case, False)
    net, c_img, c, _wgt, idx = _device_case(i)
    net.eval()
    with torch.no_grad():
        got = net(c_img, 1, c, 1)
    if case[5]:
        _equal_chunks_equal_bits(case[0], got, idx)
    _gate_forward(case[0], got, fr.references(i), idx, plan["form"])


def _grads_of(net, ch, gh):
    layer = net.decoder.layers[0]
    g = {"c_img": ch.grad, "c": gh.grad}
    for u, mod in (("self", layer.self_attn), ("cross", layer.cross_attn)):
        for n, t in mod.unit_tensors().items():
            g[f"{u}.{n}"] = t.grad
    assert len(g) == 22 and all(v is not None for v in g.values())
    return g


def _step(net, case, c_img, c, wgt):
    for prm in net.parameters():
        prm.grad = None
    ch, gh = c_img.clone().requires_grad_(), c.clone().requires_grad_()
    out = net.forward_train(ch, gh, seed=fr.DROP_SEED) if case[4] == "drop" else net(ch, 1, gh, 1)
    assert out.requires_grad
    (out * wgt).sum().backward()
    return out.detach(), {k: v.detach().clone() for k, v in _grads_of(net, ch, gh).items()}


@pytest.mark.parametrize("i", BWD_CASES, ids=IDS(BWD_CASES))
def test_training_forward_and_backward_vs_float64(i):
    from vtaco_amd import ops
    case = fr.CASES[i]
    name, C, B, N, mode = case[:5]
    plan = _plan(case, True)
    assert plan["form"] == "full"
    net, c_img, c, wgt, idx = _device_case(i)
    net.train(mode == "drop")
    if mode == "drop":                                   # the masks the kernels draw are the restated rule's, which the reference got
        assert net.p_drop == fr.P_DROP
        for call in range(3):
            for which in (0, 1):
                m = ops.fusion_dropout_mask(net.p_drop, fr.DROP_SEED, call, which, B * N, DEV, d_model=C)
                assert torch.equal(m.cpu(), fr.dropout_mask(fr.P_DROP, fr.DROP_SEED, call, which, B * N, C)), (call, which)
    r = fr.references(i)
    out, g = _step(net, case, c_img, c, wgt)
    _gate_forward(name, out, r, idx, "full")
    g64 = {k: (v[idx] if "." not in k else v) for k, v in r["g64"].items()}
    rel = fr.rel_errs({k: v.cpu() for k, v in g.items()}, g64)
    worst = []
    for k in fr.grad_names():
        floor = max(r["ge32"][k], r["ge_full"][k])
        print(f"RATIO {name} bwd {k}: {rel[k] / floor:.3f} (floor {floor:.3e}, e32 {r['ge32'][k]:.3e}, e_full {r['ge_full'][k]:.3e})")
        if not rel[k] <= fr.GATE * floor:
            worst.append((k, rel[k], floor))
    assert not worst, (name, worst)
    # bit-reproducible: a second run gives the same numbers
    out2, g2 = _step(net, case, c_img, c, wgt)
    assert torch.equal(out2, out) and all(torch.equal(g2[k], g[k]) for k in g), name


@pytest.mark.parametrize("name", ["i-2x257", "i-1x512", "i-2x2049"])
def test_finger_id_path_is_bit_equal_to_the_gathered_tensor(name):
    """ops.fusion_fwd_ids, with and without chunk_index, against ops.fusion_fwd on the gathered rows: both row-block counts of the
    half-pair form, the f8 form, and the streamed InstanceNorm."""
    from vtaco_amd import ops
    i = fr.NAMES_OF_CASES.index(name)
    case = fr.CASES[i]
    _, C, B, N = case[:4]
    _plan(case, False)
    net, _c_img, c, _wgt, _idx = _device_case(i)
    layer = net.eval().decoder.layers[0]
    sa, ca = layer.self_attn.unit_tensors(), layer.cross_attn.unit_tensors()
    g = torch.Generator().manual_seed(2000 + i)
    feats = torch.randn(5, C, generator=g).to(DEV)
    ids = torch.randint(0, 16, (B + 3, N), generator=g).to(torch.uint8)
    ids[ids >= 5] = 255                                                  # ~30 % of the rows carry a feature
    ids = ids.to(DEV)
    table = torch.cat([feats, torch.zeros(1, C, device=DEV)])
    gather = lambda rows: table[torch.where(rows == 255, torch.full_like(rows, 5), rows).long()]
    with torch.no_grad():
        assert torch.equal(ops.fusion_fwd_ids(ids[:B], feats, c, sa, ca), ops.fusion_fwd(gather(ids[:B]), c, sa, ca))
        pick = torch.tensor([(B + 2 - 2 * b) % (B + 3) for b in range(B)], dtype=torch.int32, device=DEV)
        assert torch.equal(ops.fusion_fwd_ids(ids, feats, c, sa, ca, chunk_index=pick), ops.fusion_fwd(gather(ids[pick.long()]), c, sa, ca))


def test_a_chunk_of_one_point_gives_zeros():
    """N = 1 (documented in ops/fusion.py): z - mean = 0 in the InstanceNorm, so the fused feature is 0 -- as the reference restated
    here gives; torch's InstanceNorm1d refuses one element."""
    i = fr.NAMES_OF_CASES.index("i-1x2")
    net, c_img, c, _wgt, _idx = _device_case(i)
    with torch.no_grad():
        got = net.eval()(c_img[:, :1].contiguous().expand(3, 1, 32).contiguous(), 1, c[:, :1].contiguous().expand(3, 1, 32).contiguous(), 1)
        want = fr.fuser(fr.units_of(net.cpu().state_dict()), c_img[:1, :1].cpu().double(), c[:1, :1].cpu().double())
    assert tuple(got.shape) == (3, 1, 32) and float(got.abs().max()) == 0.0 and float(want.abs().max()) == 0.0
