"""GPU: every kernel of decode_wide.hip in every launch regime, against the float64 reference of tests/decode_wide_ref.py on the inputs of
tests/decode_wide_cases.py (tests/test_decode_wide_ref_cpu.py asserts what those two hold).

The kernels are called through ops -- decode_fwd(precision="wide" | "wide_f16x3"), decode_fwd_wide_train, decode_bwd_wide, decode_mlp_fwd,
decode_mlp_fwd_wide_train, decode_mlp_bwd_wide -- so a failure names a kernel.  Every case first asks ops.decode_wide_form which kernel
runs and with what launch shape, and requires both the shape it is listed with and the rule restated in decode_wide_cases.expected_form:
a case cannot pass by quietly taking another kernel.

The gates, at ALL points, elementwise, with GATE = 8 as in the other float64 suites:
    exact f32   |got - ref64| <= 8 max(e32, 2^-24 bound)           logits, every save slot, grad_c, grad_c_img, dN / dH, every parameter
                gradient and the grid gradient; e32 = max |ref32 - ref64| over the tensor, bound the magnitude sums.  The backward
                reference takes masks and layer inputs from the kernel's own save buffer, which the forward gates by itself.
    split f16   |got - ref64| <= 8 max(e32, e_split, 2^-24 bound)  e_split = max |forward_split64 - forward64|; the pipeline, whose heads
                are summed in another order, has the same floor; ops.decode_range_status() stays 0.
    equalities  bit for bit: training-forward logits == inference logits; a lattice range == the same points given explicitly; finger
                ids == the dense tensor.
Every comparison prints `RATIO <tag>: ...`; the largest per family of a run on the MI355X are kept in profiles/decode_wide_f64_ratios.txt.

That the gates bite was tried on the kernels, one change of decode_wide.hip at a time, each built as its own library and run against
this file (48 tests) and tests/test_decode_wide_gpu.py (43 tests):
  * the W_lo x_hi product of fc_0 of block 0 dropped in wideh_gemm: the 11 streaming split-f16 tests and the two split-f16 loop tests
    fail at their first comparison (11 to 261 times the floor); the pipeline tests pass -- decode_wide_p_kernel has its own products --
    as does every exact-f32 test.  test_decode_wide_gpu.py notices this one too: 18 of its tests fail (the split-f16 oracle comparisons
    at 2e-5, the pipeline-against-streaming comparisons at 2e-6).
  * roundf (halves away from zero) instead of rintf in the nearest voxel, forward, backward and the pipeline's sampling pre-pass: the 14
    `nearest` exact-f32 tests, the four split-f16 shapes run with `nearest` and both pipeline tests fail (4e5 to 7e6 times the floor:
    another voxel's features); all 43 tests of test_decode_wide_gpu.py pass -- none of them has a point on a tie.
  * the leaky slope taken as 0 at af < 0 in the backward's head: the 14 `leaky` exact-f32 tests and the two backward loop tests fail
    (3e4 to 7e6 times the floor, at the first parameter gradient); test_decode_wide_gpu.py: 2 of 43 fail, 96/64/2 and 32/160/2 leaky.
  * the last tile of every later trip skipped (tile < ntiles - 1 once tile >= gridDim.x) in the forward, the backward and the streaming
    split-f16 kernel: the six loop tests fail, the other 42 pass; test_decode_wide_gpu.py: 1 of 43 fails (the 70 001-point case, where
    the 4-wave exact-f32 forward loops) -- the backward, the 8-wave forward and the split-f16 kernel go unnoticed there.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_train_cases as tcases
import decode_wide_cases as wc
import decode_wide_ref as wref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0


@pytest.fixture(autouse=True)
def _default_dispatch():
    if any(k in os.environ for k in wc.KNOBS):
        pytest.skip("the wide decode's form is forced by an A/B knob of the environment")


class _Net:
    """One weight set and its blobs on the device, packed once per (precision, form)."""

    def __init__(self, H, C, nb):
        self.H, self.C, self.nb = H, C, nb
        self.sd = wc.weights(H, C, nb)
        self._blobs = {}

    def _g(self, k):
        return self.sd[k].to(DEV)

    def blob(self, precision, form="plain"):
        from vtaco_amd import ops
        key = (precision, form)
        if key not in self._blobs:
            g, nb = self._g, self.nb
            first = "fc_p_img" if form == "img" else "fc_p"
            if precision == "t":
                self._blobs[key] = ops.pack_decoder_wide_t(g(first + ".weight"), [g(f"fc_c.{i}.weight") for i in range(nb)],
                                                           [(g(f"blocks.{i}.fc_0.weight"), g(f"blocks.{i}.fc_1.weight")) for i in range(nb)],
                                                           g("fc_out.weight"), g("fc_out_contact.weight") if form == "contact" else None)
            else:
                fc_c = [(g(f"fc_c.{i}.weight"), g(f"fc_c.{i}.bias")) for i in range(nb)]
                blocks = [(g(f"blocks.{i}.fc_0.weight"), g(f"blocks.{i}.fc_0.bias"), g(f"blocks.{i}.fc_1.weight"), g(f"blocks.{i}.fc_1.bias"))
                          for i in range(nb)]
                out2 = (g("fc_out_contact.weight"), g("fc_out_contact.bias")) if form == "contact" else None
                self._blobs[key] = ops.pack_decoder(g(first + ".weight"), g(first + ".bias"), fc_c, blocks, (g("fc_out.weight"), g("fc_out.bias")),
                                                    out2, precision=precision)
        return self._blobs[key]


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(H, C, nb):
        if (H, C, nb) not in cache:
            cache[(H, C, nb)] = _Net(H, C, nb)
        return cache[(H, C, nb)]
    return get


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _form(H, C, nb, kind, tactile=False, workspace=False, total=0):
    """The launch shape the library says it takes == the one the restated rule gives."""
    from vtaco_amd import ops
    got = ops.decode_wide_form(H, C, nb, kind, tactile=tactile, total=total, workspace=workspace)
    want = wc.expected_form(H, C, nb, kind, tactile, workspace, _cus())
    assert want is not None and got == {k: want[k] for k in wc.FORM_KEYS}, (H, C, nb, kind, tactile, workspace, got, want)
    return got


def _gate(tag, got, r64, r32, bound, floor=None):
    if floor is None:
        ratio, e32 = wref.gate_ratio(got, r64, r32, bound)
        floor = e32
    else:
        e32 = float((r32.double() - r64.double()).abs().max())
        floor = max(e32, floor)
        ratio = wref.gate_ratio_floor(got, r64, floor, bound)
    print(f"RATIO {tag}: {ratio:.3f} (floor {floor:.3e}, e32 {e32:.3e})")
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(floor {floor:.3e}, 2^-24 bound), above {GATE}"
    return ratio


def _pair(v, contact):
    return v if contact else (v,)


def _forward_f32(tag, net, inp, form, leaky, nearest):
    """Training forward (== inference forward, bit for bit), logits and every save slot gated.  Returns the kernel's save buffer."""
    from vtaco_amd import ops
    H, C, nb = net.H, net.C, net.nb
    B, N = inp["pts"].shape[:2]
    img, contact, mlp = form == "img", form == "contact", form == "mlp"
    pts = inp["pts"].to(DEV)
    ci = inp["c_img"] if img else None
    c = inp["c"] if mlp else None
    bform = "plain" if mlp else form
    if mlp:
        out, save = ops.decode_mlp_fwd_wide_train(c.to(DEV), net.blob("wide", bform), pts, H, nb, leaky)
        fast = ops.decode_mlp_fwd(c.to(DEV), net.blob("wide", bform), pts, precision="wide", wide=(H, nb, leaky))
        got, fast = (out,), (fast,)
        save[:B * N * C] = c.to(DEV).reshape(-1)                     # the c slot is the caller's (left unwritten by the kernel)
    else:
        grid = inp["grid"].to(DEV)
        out, out2, save = ops.decode_fwd_wide_train(grid, net.blob("wide", bform), pts, ci.to(DEV) if img else None, H, nb, leaky, nearest,
                                                    0.1, want_contact=contact)
        fast = ops.decode_fwd(grid, net.blob("wide", bform), pts=pts, c_img=ci.to(DEV) if img else None, padding=0.1, want_contact=contact,
                              precision="wide", wide=(H, nb, leaky, nearest))
        got, fast = ((out, out2) if contact else (out,)), _pair(fast, contact)
    for a, b in zip(got, fast):
        assert torch.equal(a, b), f"{tag}: the training forward's logits are not the inference kernel's"
    args = (net.sd, inp["pts"], None if mlp else inp["grid"], ci, contact, c)
    kw = dict(leaky=leaky, nearest=nearest)
    r64, s64 = wref.forward64(*args, **kw)
    r32, s32 = wref.forward32(*args, **kw)
    rb, sb = wref.forward_bound(*args, **kw)
    for k, (a, x64, x32, xb) in enumerate(zip(got, _pair(r64, contact), _pair(r32, contact), _pair(rb, contact))):
        _gate(f"{tag} fwd logits{k if contact else ''}", a, x64, x32, xb)
    saves = wref.unpack_saves(save, B, N, H, C, nb)
    names = ["c"] + [f"a{k % 2}_{k // 2}" for k in range(2 * nb)] + ["af"]
    for name, a, x64, x32, xb in zip(names, saves, s64, s32, sb):
        if not (mlp and name == "c"):
            _gate(f"{tag} fwd save {name}", a, x64, x32, xb)
    if leaky:
        assert bool((saves[-1] < 0).any()), f"{tag}: af keeps the negative leaky values"
    return save, saves


def _backward_f32(tag, net, inp, form, leaky, nearest, save, saves):
    from vtaco_amd import ops
    H, C, nb = net.H, net.C, net.nb
    img, contact, mlp = form == "img", form == "contact", form == "mlp"
    pts, go = inp["pts"].to(DEV), inp["grad_out"].to(DEV)
    go2 = inp["grad_out2"] if contact else None
    ci = inp["c_img"] if img else None
    blob_t = net.blob("t", "plain" if mlp else form)
    got = {}
    if mlp:
        got["grad_c"], g = ops.decode_mlp_bwd_wide(blob_t, go, save, pts, inp["c"].to(DEV), H, nb, leaky, want_rows=True)
        shape = None
    else:
        shape = tuple(inp["grid"].shape)
        ggrid, gimg, g = ops.decode_bwd_wide(shape, blob_t, go, save, pts, H, nb, leaky, nearest, 0.1, c_img=ci.to(DEV) if img else None,
                                             want_grid_grad=True, grad_out2=go2.to(DEV) if contact else None, want_rows=True)
        got["grad_grid"] = ggrid.permute(0, 2, 3, 4, 1)
        assert (gimg is not None) == img
        if img:
            got["grad_c_img"] = gimg
    got.update({k: (torch.stack(v) if isinstance(v, list) else v) for k, v in g.items()})
    args = (net.sd, inp["pts"], shape, saves, inp["grad_out"], go2, ci)
    kw = dict(leaky=leaky, nearest=nearest)
    r64, rb = wref.backward64(*args, **kw)
    r32 = wref.backward32(*args, **kw)
    keys = [k for k, v in r64.items() if v is not None and not (k == "grad_c" and not mlp)]
    assert set(keys) == set(got), (sorted(keys), sorted(got))
    assert len(keys) == (12 if contact else 10) + 2 + (1 if img else 0) + 1
    for k in keys:
        _gate(f"{tag} bwd {k}", got[k], r64[k], r32[k], rb[k])


F32_IDS = [f"{H}-{C}-{nb}" for H, C, nb, *_ in wc.F32_SHAPES]


@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("leaky", [False, True], ids=["relu", "leaky"])
@pytest.mark.parametrize("index", range(len(wc.F32_SHAPES)), ids=F32_IDS)
def test_exact_f32_forward_saves_and_backward_vs_float64(nets, index, leaky, nearest):
    H, C, nb, fwd_waves, bwd_waves, _ = wc.F32_SHAPES[index]
    net = nets(H, C, nb)
    for B, N, R in wc.F32_TOTALS:
        inp = wc.make_inputs(B, N, R, C)
        for form in wc.F32_FORMS:
            if form == "mlp" and nearest:
                continue
            tactile = form == "img"
            assert _form(H, C, nb, "f32", tactile, total=B * N)["waves"] == fwd_waves
            assert _form(H, C, nb, "bwd", tactile, total=B * N)["waves"] == bwd_waves
            tag = f"f32 {H}/{C}/{nb} {'leaky' if leaky else 'relu'} {'nearest' if nearest else 'bilinear'} {form} {B}x{N} R{R}"
            save, saves = _forward_f32(tag, net, inp, form, leaky, nearest)
            _backward_f32(tag, net, inp, form, leaky, nearest, save, saves)


def _split_refs(net, inp, form, leaky, nearest):
    img, contact, mlp = form == "img", form == "contact", form == "mlp"
    args = (net.sd, inp["pts"], None if mlp else inp["grid"])
    kw = dict(c_img=inp["c_img"] if img else None, contact=contact, c=inp["c"] if mlp else None, leaky=leaky, nearest=nearest)
    r64, saves = wref.forward64(*args, **kw)
    r32 = wref.forward32(*args, **kw)[0]
    rb = wref.forward_bound(*args, **kw)[0]
    kw["c"] = saves[0]
    sp = wref.forward_split64(*args, "f16", **kw)
    return [(x64, x32, xb, wref.e_split(xs, x64)) for x64, x32, xb, xs in zip(_pair(r64, contact), _pair(r32, contact), _pair(rb, contact), _pair(sp, contact))]


def _forward_f16(tag, net, inp, form, leaky, nearest):
    from vtaco_amd import ops
    H, nb = net.H, net.nb
    img, contact, mlp = form == "img", form == "contact", form == "mlp"
    pts = inp["pts"].to(DEV)
    if mlp:
        got = ops.decode_mlp_fwd(inp["c"].to(DEV), net.blob("wide_f16x3", "plain"), pts, precision="wide_f16x3", wide=(H, nb, leaky))
    else:
        got = ops.decode_fwd(inp["grid"].to(DEV), net.blob("wide_f16x3", form), pts=pts, c_img=inp["c_img"].to(DEV) if img else None, padding=0.1,
                             want_contact=contact, precision="wide_f16x3", wide=(H, nb, leaky, nearest))
    for k, (a, (x64, x32, xb, es)) in enumerate(zip(_pair(got, contact), _split_refs(net, inp, form, leaky, nearest))):
        _gate(f"{tag} logits{k if contact else ''}", a, x64, x32, xb, floor=es)
    return got


F16_IDS = [f"{H}-{C}-{nb}{'-img' if t else ''}" for _, (H, C, t, nb) in wc.F16_SHAPES]


@pytest.mark.parametrize("index", range(len(wc.F16_SHAPES)), ids=F16_IDS)
def test_split_f16_streaming_forms_vs_float64(nets, index):
    from vtaco_amd import ops
    listed, (H, C, tactile, nb) = wc.F16_SHAPES[index]
    net = nets(H, C, nb)
    leaky, nearest = index % 2 == 0, index % 3 == 1
    form = _form(H, C, nb, "f16x3", tactile)
    assert (form["waves"], form["groups"], form["pairs"], form["heads_on_c"], form["tile_points"]) == listed[:2] + listed[3:], (form, listed)
    assert wc.form_tuple(wc.expected_form(H, C, nb, "f16x3", tactile, cus=_cus())) == listed and form["pipeline"] == 0
    ops.decode_range_status(reset=True)
    for total in wc.f16_totals(form["tile_points"]):
        B = next((b for b in (3, 2, 5, 7) if total % b == 0 and total > b), 1)      # scenes end inside tiles where the total allows it
        inp = wc.make_inputs(B, total // B, 5 if total < 100 else 8, C)
        for f in (("img", "contact") if tactile else ("plain", "contact", "img")):
            if (f == "img") != tactile:                              # the other input layer: whatever form the rule gives for it
                _form(H, C, nb, "f16x3", f == "img")
            tag = f"f16x3 {H}/{C}/{nb} {'leaky' if leaky else 'relu'} {'nearest' if nearest else 'bilinear'} {f} {B}x{total // B}"
            _forward_f16(tag, net, inp, f, leaky, nearest)
    assert ops.decode_range_status() == 0


@pytest.mark.parametrize("nb", wc.PIPE_BLOCKS)
def test_register_resident_pipeline_vs_float64(nets, nb):
    """64 / 32: fewer tiles than pipeline stages (one point; 33 points = 2 tiles), and more tiles than workgroups (every workgroup walks a
    second tile, one a third); query points through the sampling pre-pass (scene by scene) and features given directly."""
    from vtaco_amd import ops
    net = nets(64, 32, nb)
    form = _form(64, 32, nb, "f16x3", workspace=True)
    assert form["pipeline"] == 1 and form["waves"] == 2 * nb + 2 and form["tile_points"] == 32 and form["grid_cap"] == _cus()
    assert _form(64, 32, nb, "f16x3", workspace=False)["pipeline"] == 0 and _form(64, 32, nb, "f16x3", tactile=True, workspace=True)["pipeline"] == 0
    ops.decode_range_status(reset=True)
    many = wc.loop_total(form)
    for B, N in ((1, 1), (3, 11), (1, many)):
        assert (N + 31) // 32 < 2 * nb + 2 or (N + 31) // 32 == form["grid_cap"] + 2
        inp = wc.make_inputs(B, N, 8, 32)
        leaky = N != 11
        for f, nearest in (("plain", False), ("contact", True), ("mlp", False)):
            tag = f"f16x3 pipeline 64/32/{nb} {'leaky' if leaky else 'relu'} {'nearest' if nearest else 'bilinear'} {f} {B}x{N}"
            _forward_f16(tag, net, inp, f, leaky, nearest)
    assert ops.decode_range_status() == 0


def _loop_inputs(form, C):
    total = wc.loop_total(form)
    B = next((b for b in (5, 3, 7, 11, 13) if total % b == 0), 1)      # tiles straddle scenes where the total allows it
    return total, wc.make_inputs(B, total // B, 8, C)


LOOP_IDS = [f"{k}-{H}-{C}-{nb}" for k, H, C, nb in wc.LOOP_SHAPES]


@pytest.mark.parametrize("index", range(len(wc.LOOP_SHAPES)), ids=LOOP_IDS)
def test_persistent_tile_loop_vs_float64(nets, index):
    """More tiles than workgroups: grid_cap + 2 tiles, the last one ragged -- every workgroup's second trip, the first workgroups' third.
    Gated in full: every point of every tile (the first trip's, cap - 1, cap, cap + 1 and the last two among them), and the sums."""
    from vtaco_amd import ops
    kind, H, C, nb = wc.LOOP_SHAPES[index]
    net = nets(H, C, nb)
    form = _form(H, C, nb, kind, tactile=kind == "bwd")
    total, inp = _loop_inputs(form, C)
    B, N = inp["pts"].shape[:2]
    ntiles = (total + form["tile_points"] - 1) // form["tile_points"]
    assert B * N == total and ntiles == form["grid_cap"] + 2 and total % form["tile_points"] == 17
    assert wc.loop_tiles(total, form) == [0, form["grid_cap"] - 1, form["grid_cap"], form["grid_cap"] + 1]
    leaky = H == 32
    tag = f"loop {kind} {H}/{C}/{nb} {'leaky' if leaky else 'relu'} {B}x{N}"
    if kind == "f16x3":
        ops.decode_range_status(reset=True)
        _forward_f16(tag + " plain", net, inp, "plain", leaky, False)
        assert ops.decode_range_status() == 0
        return
    f = "img" if kind == "bwd" else "contact"
    _form(H, C, nb, "f32", tactile=f == "img")
    save, saves = _forward_f32(f"{tag} {f}", net, inp, f, leaky, False)
    if kind == "bwd":
        _backward_f32(f"{tag} {f}", net, inp, f, leaky, False, save, saves)


def test_lattice_ranges_and_finger_ids_equal_their_explicit_forms(nets):
    """Bit for bit: a lattice range that starts inside a tile == the same points given explicitly (exact f32 and split f16, two scenes);
    the tactile feature by finger id == the dense tensor (both kernels, fc_p_img's K = 72 beyond hidden 32)."""
    from vtaco_amd import ops
    nx, first, count = 12, 7, 1000
    lat = torch.from_numpy(tcases.lattice_points(nx, 1.1))[first:first + count].unsqueeze(0).expand(2, -1, -1).contiguous().to(DEV)
    for H, C, nb, precision in ((128, 128, 2, "wide"), (96, 32, 2, "wide_f16x3")):
        net = nets(H, C, nb)
        grid = wc.make_inputs(2, 333, 8, C)["grid"].to(DEV)
        kw = dict(padding=0.1, precision=precision, wide=(H, nb, True, False))
        by_range = ops.decode_fwd(grid, net.blob(precision), lattice=(nx, 1.1, first, count), **kw)
        by_points = ops.decode_fwd(grid, net.blob(precision), pts=lat, **kw)
        assert torch.equal(by_range, by_points), f"{precision}: the lattice range is not the same points given explicitly, bit for bit"
    net = nets(32, 64, 1)
    inp = wc.make_inputs(2, 333, 5, 64)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(5, 64, generator=g)
    ids = torch.randint(0, 6, (2, 333), generator=g).to(torch.uint8)
    ids[ids == 5] = 255                                              # no finger
    dense = torch.cat([feats, torch.zeros(1, 64)])[torch.where(ids == 255, torch.full_like(ids, 5), ids).long()]
    for precision in ("wide", "wide_f16x3"):
        kw = dict(pts=inp["pts"].to(DEV), padding=0.1, precision=precision, wide=(32, 1, False, False))
        by_id = ops.decode_fwd(inp["grid"].to(DEV), net.blob(precision, "img"), finger_ids=ids.to(DEV), finger_feats=feats.to(DEV), **kw)
        by_dense = ops.decode_fwd(inp["grid"].to(DEV), net.blob(precision, "img"), c_img=dense.to(DEV), **kw)
        assert torch.equal(by_id, by_dense), f"{precision}: finger ids and the dense c_img differ"
