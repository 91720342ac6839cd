"""GPU: every kernel form of the 32/32 lattice decode at the bounds of its footprint, against the float64 reference of
tests/decode_lattice_ref.py (tests/test_decode_lattice_ref_cpu.py asserts what that holds).

decode_launch picks one of five forms -- linear tiles, 2 x 4 x 4 bricks with the direct gather, decode_fwd_staged_kernel (3 x 4 x 4
voxel footprint, s < 0.66 voxels per lattice step), decode_fwd_staged2_kernel and decode_fwd_staged3_kernel (3 x 4 x 6 footprint,
nx % 8 == 0, R >= 6, s < 0.55).  Every case first asks ops.decode_lattice_form which one runs and requires the form it is listed with,
so a boundary case cannot pass by quietly taking another kernel.  Then, for both weight sets and the precisions f32, bf16x3 and f16x3:
the whole lattice of two scenes with different grids, a slab of two x-plane pairs starting at plane pair 1 (bit-equal to that range of
the whole lattice), and a range that starts inside a row (linear tiles); on three cases also the tactile concat (dense and by finger
id, bit-equal) and the contact head, which moves double bricks to single ones.  f16f8 runs on the staged3 cases.

The gates, at ALL points (the logits are continuous: no exclusion), elementwise, with GATE = 8 as in the other float64 suites:
    exact f32   |got - ref64| <= 8 max(e32, 2^-24 bound)           e32 = max |forward32 - forward64|, bound the magnitude sums
    split       |got - ref64| <= 8 max(e32, e_split, 2^-24 bound)  e_split = max |split64 - forward64| of that format's float64 model: the
                kernel adds float32 accumulation to the model's operand rounding, at most two such terms under a factor of 8
    f16f8       max |got - ref64| <= 6e-5 max |logit|              the contract of tests/test_decode_f16f8_gpu.py
Every comparison prints `RATIO <tag>: ...`; the largest of a run on the MI355X are kept in profiles/decode_lattice_f64_ratios.txt.

That the gates bite was tried on the kernels, with two changes of arithmetic alone.  The W_lo x_hi product of one dense layer (fc_0 of
block 1) dropped from the split-f16 forms: all 18 tests here fail at their first f16x3 comparison (9 to 100 times the floor), whatever
the form.  The lower x corner's weight used for both x corners in decode_fwd_staged_kernel's gather: the seven cases listed as staged
fail, as do 16 / 9 and 16 / 10 of the tactile / contact test (the contact head runs staged), the other nine tests pass -- and so does
every test of test_decode_gpu.py, test_decode_bf16x3_gpu.py and test_decode_f16f8_gpu.py, which never run that kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_lattice_ref as lat
import decode_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
F16F8_REL = 6e-5
KNOBS = ("VTACO_DECODE_DIRECT", "VTACO_DECODE_NO_PAIR", "VTACO_DECODE_ST3")


class _Weights:
    """One weight set on the device and its blobs, packed once per (precision, form)."""

    def __init__(self, sd):
        self.sd = sd
        self._blobs = {}

    def blob(self, precision, form="plain"):
        from vtaco_amd import ops
        key = (precision, form)
        if key not in self._blobs:
            g = lambda k: self.sd[k].to(DEV)
            first = "fc_p_img" if form == "img" else "fc_p"
            fc_c = [(g(f"fc_c.{i}.weight"), g(f"fc_c.{i}.bias")) for i in range(5)]
            blocks = [(g(f"blocks.{i}.fc_0.weight"), g(f"blocks.{i}.fc_0.bias"), g(f"blocks.{i}.fc_1.weight"), g(f"blocks.{i}.fc_1.bias"))
                      for i in range(5)]
            out2 = (g("fc_out_contact.weight"), g("fc_out_contact.bias")) if form == "contact" else None
            self._blobs[key] = ops.pack_decoder(g(first + ".weight"), g(first + ".bias"), fc_c, blocks,
                                                (g("fc_out.weight"), g("fc_out.bias")), out2, precision=precision)
        return self._blobs[key]


@pytest.fixture(scope="module")
def weights():
    return {k: _Weights(sd) for k, sd in lat.weight_sets().items()}


def _gate(tag, precision, got, refs, lo=None, hi=None, part=None):
    """Gate ``got`` [B,n] against the reference's range [lo, hi) of every scene (``part``: which of a contact pair)."""
    pick = lambda v: (v if part is None else v[part])[:, lo:hi]
    r64, r32, bound = pick(refs["ref64"]), pick(refs["ref32"]), pick(refs["bound"])
    if precision == "f32":
        ratio, floor = ref.gate_ratio(got, r64, r32, bound)
        e32 = floor
    else:
        e32 = float((r32.double() - r64).abs().max())
        floor = max(e32, lat.e_split(pick(refs[precision]), r64))
        ratio = lat.gate_ratio_floor(got, r64, floor, bound)
    print(f"RATIO {tag}: {ratio:.3f} (floor {floor:.3e}, e32 {e32:.3e})")
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(floor {floor:.3e}, 2^-24 bound), above {GATE}"
    return ratio


def _form(cs, lattice, precision, **kw):
    """The form the library says it runs == the form the restated rule gives."""
    from vtaco_amd import ops
    got = ops.decode_lattice_form(cs.R, lattice, padding=cs.padding, precision=precision, **kw)
    nx, box, first, count = lattice
    assert got == lat.expected_form(nx, cs.R, box, first, count, cs.padding, precision, **kw), (cs.id, lattice, precision, kw, got)
    return got


@pytest.fixture(autouse=True)
def _default_dispatch():
    if any(k in os.environ for k in KNOBS):
        pytest.skip("the lattice decode's form is forced by an A/B knob of the environment")


@pytest.mark.parametrize("index", range(len(lat.CASES)), ids=[cs.id for cs in lat.CASES])
def test_lattice_forms_vs_float64(weights, index):
    from vtaco_amd import ops
    cs, inp = lat.CASES[index], lat.inputs(index)
    grid = inp["grid"].to(DEV)
    n = cs.nx ** 3
    whole, slab, ragged = cs.lattice(), cs.slab(), cs.ragged()
    for wname, W in weights.items():
        refs = lat.references(index, wname)
        for precision in lat.PRECISIONS:
            tag = f"{cs.id}/{wname}/{precision}"
            assert _form(cs, whole, precision) == cs.listed(precision), tag
            assert _form(cs, slab, precision) == cs.listed(precision), tag
            assert _form(cs, ragged, precision) == "linear", tag
            blob = W.blob(precision)
            run = lambda lattice: ops.decode_fwd(grid, blob, lattice=lattice, padding=cs.padding, precision=precision)
            got = run(whole)
            assert got.shape == (lat.BATCH, n)
            _gate(f"{tag} {cs.listed(precision)} whole", precision, got, refs)
            part = run(slab)
            assert torch.equal(part, got[:, slab[2]:slab[2] + slab[3]]), f"{tag}: the slab is not the whole lattice's range, bit for bit"
            odd = run(ragged)
            _gate(f"{tag} linear first 7", precision, odd, refs, ragged[2], ragged[2] + ragged[3])
        if cs.form16 == "staged3":
            assert _form(cs, whole, "f16f8") == "staged3" and ops.f16f8_covers(grid, whole, cs.padding)
            got = ops.decode_fwd(grid, W.blob("f16f8"), lattice=whole, padding=cs.padding, precision="f16f8").cpu().double()
            err, top = float((got - refs["ref64"]).abs().max()), float(refs["ref64"].abs().max())
            print(f"RATIO {cs.id}/{wname}/f16f8 staged3 whole: {err / (F16F8_REL * top):.3f} of {F16F8_REL} max|logit| (err {err:.3e}, max|logit| {top:.2f})")
            assert err <= F16F8_REL * top
            part = ops.decode_fwd(grid, W.blob("f16f8"), lattice=slab, padding=cs.padding, precision="f16f8").cpu().double()
            assert torch.equal(part, got[:, slab[2]:slab[2] + slab[3]])
        else:
            with pytest.raises(ops.VtError):
                ops.decode_lattice_form(cs.R, whole, padding=cs.padding, precision="f16f8")
            assert not ops.f16f8_covers(grid, whole, cs.padding)


EXTRAS = [i for i, cs in enumerate(lat.CASES) if cs.extras]


@pytest.mark.parametrize("index", EXTRAS, ids=[lat.CASES[i].id for i in EXTRAS])
def test_tactile_concat_and_contact_head_vs_float64(weights, index):
    """16 / 9 (double bricks), 16 / 10 (staged single bricks) and 16 / 11 (direct bricks): a dense c_img with about 30 % non-zero rows,
    the same features by finger id (bit-equal), and the contact head -- which the double-brick kernels do not have: those cases run
    the single-brick staged kernel with it, and the form query says so."""
    from vtaco_amd import ops
    cs, inp = lat.CASES[index], lat.inputs(index)
    grid, dense, ids, feats = (inp[k].to(DEV) for k in ("grid", "c_img", "ids", "feats"))
    share = float((inp["c_img"] != 0).any(-1).float().mean())
    assert 0.25 < share < 0.35
    whole = cs.lattice()
    for wname, W in weights.items():
        r_img, r_con = lat.references(index, wname, "img"), lat.references(index, wname, "contact")
        for precision in lat.PRECISIONS:
            tag = f"{cs.id}/{wname}/{precision}"
            form = _form(cs, whole, precision)
            assert form == cs.listed(precision)
            by_dense = ops.decode_fwd(grid, W.blob(precision, "img"), c_img=dense, lattice=whole, padding=cs.padding, precision=precision)
            _gate(f"{tag} {form} c_img", precision, by_dense, r_img)
            by_id = ops.decode_fwd_ids(grid, W.blob(precision, "img"), ids, feats, lattice=whole, padding=cs.padding, precision=precision)
            assert torch.equal(by_id, by_dense), f"{tag}: finger ids and the dense c_img differ"
            form2 = _form(cs, whole, precision, want_contact=True)
            assert form2 == ("staged" if form in ("staged2", "staged3") else form), tag
            occ, con = ops.decode_fwd(grid, W.blob(precision, "contact"), lattice=whole, padding=cs.padding, precision=precision,
                                      want_contact=True)
            _gate(f"{tag} {form2} contact: logits", precision, occ, r_con, part=0)
            _gate(f"{tag} {form2} contact: contact logits", precision, con, r_con, part=1)
        if cs.form16 == "staged3":
            b8 = W.blob("f16f8", "img")
            by_dense = ops.decode_fwd(grid, b8, c_img=dense, lattice=whole, padding=cs.padding, precision="f16f8")
            by_id = ops.decode_fwd_ids(grid, b8, ids, feats, lattice=whole, padding=cs.padding, precision="f16f8")
            assert torch.equal(by_id, by_dense)
            err, top = float((by_dense.cpu().double() - r_img["ref64"]).abs().max()), float(r_img["ref64"].abs().max())
            print(f"RATIO {cs.id}/{wname}/f16f8 staged3 c_img: {err / (F16F8_REL * top):.3f} of {F16F8_REL} max|logit| (err {err:.3e})")
            assert err <= F16F8_REL * top
