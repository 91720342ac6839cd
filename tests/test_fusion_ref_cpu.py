"""The float64 reference of TransformerFusion (tests/fusion_ref.py) pinned before any kernel runs: against the oracle and the golden g5,
its rounding models ordered as the roundings are, the cases' conditioning judged by the reference alone, the launch plan at the
boundary sizes, the repeated-chunk shortcut of the large-launch cases, and the dropout rule restated."""
import os
import statistics

import pytest
import torch

import fusion_ref as fr
from conftest import load_golden, sub_sd

CASE_IDS = list(range(len(fr.CASES)))


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("masked", [False, True])
def test_exact_form_is_the_oracle_in_float64(C, masked):
    from oracle import vtaco_oracle as orc
    i = fr.NAMES_OF_CASES.index("t-2x128" if C == 32 else "w128-b2x129")
    units, c_img, c, wgt = fr.case_inputs(i)
    B, N = c.shape[:2]
    masks = None
    if masked:
        masks = [tuple(fr.dropout_mask(0.1, 77, call, which, B * N, C).reshape(B, N, -1).double() for which in (0, 1)) for call in range(3)]
    u64 = {u: {n: t.double().requires_grad_() for n, t in d.items()} for u, d in units.items()}
    a, b = c_img.double().requires_grad_(), c.double().requires_grad_()
    mine = fr.fuser(u64, a, b, "exact", masks)
    (mine * wgt.double()).sum().backward()
    o64 = {u: {n: t.double().requires_grad_() for n, t in d.items()} for u, d in units.items()}
    a2, b2 = c_img.double().requires_grad_(), c.double().requires_grad_()
    ref = orc.transformer_fusion(fr.oracle_sd(o64), a2, b2, masks=masks)
    (ref * wgt.double()).sum().backward()
    assert _rel(mine.detach(), ref.detach()) <= 1e-12
    assert _rel(a.grad, a2.grad) <= 1e-10 and _rel(b.grad, b2.grad) <= 1e-10      # (autograd of two orders of the same sums)
    for u in ("self", "cross"):
        for n in fr.NAMES:
            assert float((u64[u][n].grad - o64[u][n].grad).abs().max()) <= 1e-10 * max(float(o64[u][n].grad.abs().max()), 1.0), (u, n)


def test_exact_form_reproduces_the_golden_fuser_output():
    a, sd = load_golden("g5_fusion.npz")
    units = fr.units_of(sub_sd(sd, "fuser."), torch.float64)
    with torch.no_grad():
        out = fr.fuser(units, torch.from_numpy(a["c_img256"]).double(), torch.from_numpy(a["c256"]).double())
    assert float((out - torch.from_numpy(a["fused256"]).double()).abs().max()) <= 5e-5      # tests/test_fusion_gpu.py's tolerance for it


@pytest.mark.parametrize("i", CASE_IDS, ids=fr.NAMES_OF_CASES)
def test_models_are_ordered_and_every_forward_floor_is_within_the_old_tolerance(i):
    """0 < e_form("full") <= e_form("half_pair") (rounding the keys as well can only add error), and the floor of the case's forward
    gate is at most the 5e-5 of tests/test_fusion_gpu.py: the new gate is never looser than eight times the old one."""
    case, r = fr.CASES[i], fr.references(i)
    assert 0.0 < r["e_full"] and 0.0 < r["e32"]
    form = fr.form_of(case)
    if case[4] == "infer":
        assert r["e_full"] <= r["e_half_pair"], (r["e_full"], r["e_half_pair"])
        form = form or "half_pair"                               # f8: the half-pair floor is what its recorded ratio refers to
    print(f"FLOOR {case[0]}: e32 {r['e32']:.3g} e_full {r['e_full']:.3g} e_half_pair {r.get('e_half_pair', float('nan')):.3g}")
    assert fr.forward_floor(r, form) <= fr.F8_CONTRACT, (form, r["e32"], r["e_" + form])
    if "ge32" in r:
        assert len(r["g64"]) == 22 and all(torch.isfinite(v).all() for v in r["g64"].values())
        assert all(0.0 < max(r["ge32"][k], r["ge_full"][k]) < 1e-3 for k in r["g64"]), (r["ge32"], r["ge_full"])


def test_cases_are_well_conditioned_by_the_reference_alone():
    """Per case the smallest per-channel standard deviation over a chunk of the three pre-InstanceNorm tensors (printed; the table in
    fusion_ref.py records it), and e32 within a factor of 10 of the median e32 of the cases of the same d_model: a case where the
    InstanceNorm multiplies rounding noise would swamp its gate.  A seed that fails moves on by 500 (fusion_ref.RESEEDED)."""
    by_width = {}
    for i, case in enumerate(fr.CASES):
        by_width.setdefault(case[1], []).append(fr.references(i)["e32"])
    for i, case in enumerate(fr.CASES):
        stds = fr.min_channel_std(i)
        med = statistics.median(by_width[case[1]])
        e32 = fr.references(i)["e32"]
        print(f"MINSTD {case[0]}: {min(stds):.3g} ({', '.join(f'{s:.3g}' for s in stds)}) e32 {e32:.3g} median {med:.3g}")
        assert len(stds) == 3 and min(stds) >= 0.0
        assert med / 10 <= e32 <= med * 10, (case[0], e32, med)


PLAN = lambda form, tiles, inorm, f, b, strided=(): {"form": form, "proj_tiles": tiles, "inorm": inorm, "fwd_row_blocks": f,
                                                     "bwd_row_blocks": b, "strided": tuple(strided)}
BOUNDARIES = [
    ((1, 2, 32, False), PLAN("half_pair", 1, "cached", 1, 1)),
    ((3, 255, 32, False), PLAN("half_pair", 1, "cached", 1, 2)),
    ((1, 256, 32, False), PLAN("half_pair", 1, "cached", 1, 2)),
    ((2, 257, 32, False), PLAN("half_pair", 1, "cached", 2, 3)),
    ((1, 511, 32, False), PLAN("half_pair", 1, "cached", 2, 4)),
    ((1, 512, 32, False), PLAN("f8", 1, "cached", 2, 4)),
    ((1, 512, 32, True), PLAN("full", 1, "cached", 2, 4)),
    ((1, 2048, 32, False), PLAN("f8", 1, "cached", 8, 16)),
    ((2, 2049, 32, False), PLAN("f8", 1, "streamed", 9, 17)),
    ((1, 2049, 32, True), PLAN("full", 1, "streamed", 9, 17)),
    ((192, 2048, 32, False), PLAN("f8", 2, "cached", 8, 16)),            # 393 216 points exactly
    ((191, 2048, 32, False), PLAN("f8", 1, "cached", 8, 16)),
    ((193, 2048, 32, False), PLAN("f8", 2, "cached", 8, 16)),
    ((8192, 33, 32, False), PLAN("half_pair", 1, "cached", 1, 1)),       # 2 tiles x 128 items x 8192 chunks = 8192 blocks of 256: the cap itself
    ((8193, 33, 32, False), PLAN("half_pair", 1, "cached", 1, 1, ["scalev"])),
    ((8200, 33, 32, False), PLAN("half_pair", 1, "cached", 1, 1, ["scalev"])),
    ((2048, 512, 32, False), PLAN("f8", 5, "cached", 2, 4)),
    ((2050, 512, 32, False), PLAN("f8", 5, "cached", 2, 4, ["scalev"])),
    ((1, 127, 32, True), PLAN("full", 1, "cached", 1, 1)),
    ((2, 128, 32, True), PLAN("full", 1, "cached", 1, 1)),
    ((1, 129, 32, True), PLAN("full", 1, "cached", 1, 2)),
    ((16, 2048, 32, True), PLAN("full", 1, "cached", 8, 16)),            # 32 768 points x 32 / 256 = 4096 blocks: the cap itself
    ((17, 2048, 32, True), PLAN("full", 1, "cached", 8, 16, ["add"])),
    ((2, 33, 64, False), PLAN("full", 8, "streamed", 1, 1)),
    ((16, 2048, 64, False), PLAN("full", 8, "streamed", 8, 16)),         # 1024 groups of 32 points = 4 x 256 compute units: the cap itself
    ((17, 2048, 128, False), PLAN("full", 8, "streamed", 8, 16, ["epilogue"])),
    ((2, 129, 64, True), PLAN("full", 8, "streamed", 1, 2)),
    ((1, 1024, 128, True), PLAN("full", 8, "streamed", 4, 8)),           # 256 groups of 4 points: one per compute unit
    ((1, 1025, 128, True), PLAN("full", 8, "streamed", 5, 9, ["bwd_point"])),
    ((3, 171, 96, True), PLAN("full", 8, "streamed", 1, 2)),
]


@pytest.mark.parametrize("args,want", BOUNDARIES, ids=[f"{a[0]}x{a[1]}-{a[2]}{'-train' if a[3] else ''}" for a, _ in BOUNDARIES])
def test_expected_plan_at_the_boundary_sizes(args, want):
    """The restated rule on both sides of every threshold, written out; and, at d_model 32 (where the query reads no device property),
    the library's own answer where it is built."""
    assert fr.expected_plan(*args) == want
    if args[2] == 32 and not os.environ.get("VTACO_FUSION_SCORE_TERMS"):
        from vtaco_amd import _lib, ops
        if os.path.exists(_lib.LIB_PATH):
            assert ops.fusion_plan(*args) == want


@pytest.mark.parametrize("terms,forms", [("3", ("full", "full", "full")), ("2", ("half_pair", "half_pair", "full"))])
def test_plan_honours_the_score_terms_knob_as_the_launchers_do(terms, forms):
    """VTACO_FUSION_SCORE_TERMS is read once per process by the one rule the launchers and the query share: 3 forces all three
    products, 2 the half-pair form at every N; the training forward keeps the full form either way.  (A fresh process: the knob is
    latched at the first call.)"""
    import subprocess
    import sys
    code = ("from vtaco_amd import ops; "
            "print(ops.fusion_plan(1, 511)['form'], ops.fusion_plan(1, 512)['form'], ops.fusion_plan(1, 512, train=True)['form'])")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "VTACO_FUSION_SCORE_TERMS": terms}, cwd=root,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert tuple(out.stdout.split()) == forms


def test_every_case_is_listed_for_the_plan_the_rule_gives():
    for name, C, B, N, mode, distinct, _w, want in fr.CASES:
        plan = fr.expected_plan(B, N, C, mode in ("bwd", "drop"))
        assert {k: plan[k] for k in want} == want, (name, plan)


def test_a_repeated_chunk_gives_copies_and_weighted_parameter_gradients():
    """What the large-launch cases rely on: on a batch of two distinct chunks repeated, the reference is the copies of the distinct
    chunks' outputs, the input gradients are those of one copy and the parameter gradients the multiplicity-weighted sums."""
    i = fr.NAMES_OF_CASES.index("t-1x127")
    units, c_img, c, wgt = fr.case_inputs(i)
    g = torch.Generator().manual_seed(5)
    c_img = torch.cat([c_img, torch.randn(1, 127, 32, generator=g) * (torch.rand(1, 127, 1, generator=g) < 0.3)])
    c, wgt = torch.cat([c, torch.randn(1, 127, 32, generator=g)]), torch.cat([wgt, torch.randn(1, 127, 32, generator=g)])
    idx = fr.chunk_index(7, 2)
    assert sorted(set(idx.tolist())) == [0, 1]
    mult = torch.bincount(idx, minlength=2).double()
    out_d, g_d = fr._run(units, c_img, c, wgt, mult, torch.float64, "exact", None, True)
    out_e, g_e = fr._run(units, c_img[idx], c[idx], wgt[idx], torch.ones(7, dtype=torch.float64), torch.float64, "exact", None, True)
    assert _rel(out_e, out_d[idx]) <= 1e-13
    for k in fr.grad_names():
        want = g_d[k][idx] if "." not in k else g_d[k]
        assert float((g_e[k] - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max())), k


def test_restated_dropout_rule():
    m0, m1 = fr.dropout_mask(0.1, fr.DROP_SEED, 1, 0, 500), fr.dropout_mask(0.1, fr.DROP_SEED, 1, 1, 500, 96)
    assert tuple(m0.shape) == (500, 64) and tuple(m1.shape) == (500, 96)
    for m in (m0, m1):
        assert 0.08 <= float((m == 0).float().mean()) <= 0.12 and bool(((m == 0) | (m == float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.1))))).all())
    assert not torch.equal(m0, fr.dropout_mask(0.1, fr.DROP_SEED + 1, 1, 0, 500))
    assert float(fr.dropout_mask(0.0, 3, 0, 0, 10).min()) == 1.0
