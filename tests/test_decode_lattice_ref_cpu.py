"""CPU: what tests/test_decode_lattice_f64_gpu.py stands on (tests/decode_lattice_ref.py) -- the restated dispatch rule gives the form
every case is listed with, the float64 forward is the oracle's decoder on the lattice, the written-out 16-bit roundings are the formats'
own, and the split models order as the formats do."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_lattice_ref as lat
import decode_train_ref as ref

NO_KNOBS = {}


def test_every_case_is_listed_with_the_form_the_rule_gives():
    for cs in lat.CASES:
        s = lat.step_voxels(cs.nx, cs.R, cs.box, cs.padding)
        forms = {p: lat.expected_form(cs.nx, cs.R, cs.box, padding=cs.padding, precision=p, env=NO_KNOBS) for p in lat.PRECISIONS}
        print(f"{cs.id}: s = {s:.4f} (listed {cs.s}), forms {forms}")
        assert abs(s - cs.s) < 1e-3                                # the table's s, to its three digits
        assert forms["f32"] == forms["bf16x3"] == cs.form and forms["f16x3"] == cs.form16
        assert cs.form in lat.FORMS and cs.form16 in lat.FORMS
        # the slab of two plane pairs keeps the form; a range from inside a row is linear tiles; the contact head leaves no double bricks
        for p in lat.PRECISIONS:
            nx, box, first, count = cs.slab()
            assert first == 2 * nx * nx and first + count <= nx ** 3
            assert lat.expected_form(nx, cs.R, box, first, count, cs.padding, p, env=NO_KNOBS) == cs.listed(p)
            nx, box, first, count = cs.ragged()
            assert first + count <= nx ** 3
            assert lat.expected_form(nx, cs.R, box, first, count, cs.padding, p, env=NO_KNOBS) == "linear"
            with_contact = lat.expected_form(cs.nx, cs.R, cs.box, padding=cs.padding, precision=p, want_contact=True, env=NO_KNOBS)
            assert with_contact == ("staged" if cs.listed(p) in ("staged2", "staged3") else cs.listed(p))
        f8 = lat.expected_form(cs.nx, cs.R, cs.box, padding=cs.padding, precision="f16f8", env=NO_KNOBS)
        assert f8 == ("staged3" if cs.form16 == "staged3" else None)
    # every form is run, and both bounds are approached from both sides
    assert {cs.form for cs in lat.CASES} | {cs.form16 for cs in lat.CASES} == set(lat.FORMS)
    steps = sorted(lat.step_voxels(cs.nx, cs.R, cs.box, cs.padding) for cs in lat.CASES)
    for bound in (0.55, 0.66):
        assert max(s for s in steps if s < bound) > bound - 0.003 and min(s for s in steps if s > bound) < bound + 0.06


def test_the_rule_follows_the_knobs_and_the_lds_terms():
    form = lambda nx, R, p="f32", **kw: lat.expected_form(nx, R, precision=p, **kw)
    assert form(16, 9, "f16x3", env={"VTACO_DECODE_ST3": "0"}) == "staged2"
    assert form(16, 9, "f16x3", env={"VTACO_DECODE_ST3": "1"}) == "staged3"
    assert form(16, 9, "f16x3", env={"VTACO_DECODE_NO_PAIR": "1"}) == "staged"
    assert form(16, 9, "f16x3", env={"VTACO_DECODE_DIRECT": "1"}) == "brick"
    assert form(16, 9, "f16f8", env={"VTACO_DECODE_DIRECT": "1"}) == "staged3"        # the f16f8 launcher has no knob
    assert form(16, 9, c_direct=True, env=NO_KNOBS) == "brick"
    # the bench lattices: double bricks at 128^3 and 256^3 over R = 64
    assert form(128, 64, env=NO_KNOBS) == "staged2" and form(256, 64, "f16x3", env=NO_KNOBS) == "staged3"
    # blob + tables + images within 160 KiB: the five-entry table of staged3 ends first, then staged2's, then the single bricks'
    assert lat.BLOB_FLOATS * 4 == 73984
    assert form(328, 150, "f16x3", env=NO_KNOBS) == "staged3" and form(336, 150, "f16x3", env=NO_KNOBS) == "staged2"
    assert form(416, 150, env=NO_KNOBS) == "staged2" and form(424, 150, env=NO_KNOBS) == "staged"
    assert form(432, 150, env=NO_KNOBS) == "staged" and form(436, 150, env=NO_KNOBS) == "brick"


@pytest.mark.parametrize("index", [2, 13], ids=lambda i: lat.CASES[i].id)
def test_forward64_is_the_oracles_decoder_on_the_lattice(index):
    """The smallest grid and the lattice whose outer points are clamped on both sides, golden weights: within 1e-5 of the float32 oracle."""
    from oracle import vtaco_oracle as orc
    cs, inp = lat.CASES[index], lat.inputs(index)
    if cs.box > 1.101:
        q = inp["pts"][0].double() / ref.divisor(cs.padding) + 0.5
        assert bool((q >= 1).any()) and bool((q < 0).any())
    sd = lat.weight_sets()["g1"]
    want = orc.local_decoder_forward(sd, inp["pts"], inp["grid"], padding=cs.padding)
    got = lat.references(index, "g1")["ref64"]
    err = float((got - want.double()).abs().max())
    print(f"{cs.id}: max |forward64 - oracle| = {err:.3e} (logits up to {float(got.abs().max()):.2f})")
    assert err <= 1e-5


def _values():
    rng = np.random.RandomState(5)
    v = np.concatenate([rng.randn(20000) * np.exp(rng.uniform(-12, 8, 20000)), rng.uniform(-2.0 ** -14, 2.0 ** -14, 2000),
                        [0.0, 1.0, -1.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -11, 65504.0, 65519.0, 1e5, -1e5,
                         1.0 + 2.0 ** -10 - 2.0 ** -30, 3 * 2.0 ** -24 + 2.0 ** -40]])
    return v


def test_the_written_out_half_rounding_is_numpys():
    v = _values()
    inside = np.abs(v) < 65520.0
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).astype(np.float64)
    assert np.array_equal(lat.round_half(v).numpy()[inside], want[inside])
    assert np.all(np.abs(lat.round_half(v).numpy()[~inside]) == 65504.0)
    # toward zero: the half at or next below |v|
    rz = lat.round_half(v, toward_zero=True).numpy()
    assert np.array_equal(rz.astype(np.float16).astype(np.float64), rz)                      # a half
    assert np.all(np.abs(rz) <= np.abs(v)) and np.all(rz * v >= 0)
    with np.errstate(over="ignore"):
        up = np.nextafter(rz.astype(np.float16), np.where(v >= 0, np.float16(np.inf), np.float16(-np.inf))).astype(np.float64)
    assert np.all((np.abs(up) > np.abs(v)) | (np.abs(rz) == 65504.0))


def test_f16_toward_zero_split_round_trips():
    v = _values()
    v = v[np.abs(v) < 65504.0]
    hi, lo = (t.numpy() for t in lat.split(torch.from_numpy(v), "f16x3"))
    assert np.all(np.abs(hi) <= np.abs(v))
    normal = np.abs(v) >= 2.0 ** -3                               # lo is a normal half from here on: hi + lo carries 21 bits
    assert np.all(np.abs(hi + lo - v)[normal] <= 2.0 ** -21 * np.abs(v)[normal])
    assert np.all(np.abs(hi + lo - v) <= np.maximum(2.0 ** -21 * np.abs(v), 2.0 ** -25))     # below: half the subnormal spacing 2^-24
    tiny = np.abs(v) < 2.0 ** -14                                 # half subnormals are kept, not flushed
    assert tiny.sum() > 1000 and np.count_nonzero(hi[tiny]) > 0.9 * tiny.sum()
    assert np.array_equal(hi[tiny], np.trunc(v[tiny] * 2.0 ** 24) * 2.0 ** -24)


def test_bf16_split_is_within_two_to_the_minus_16():
    v = _values()
    hi, lo = (t.numpy() for t in lat.split(torch.from_numpy(v), "bf16x3"))
    v32 = v.astype(np.float32)                                    # on float32 values bf16 is the upper half, to nearest even
    bits = v32.view(np.uint32).astype(np.uint64)
    want = (((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32).astype(np.float64)
    assert np.array_equal(lat.round_bf16(v32.astype(np.float64)).numpy(), want)
    assert np.all(np.abs(hi + lo - v) <= 2.0 ** -16 * np.abs(v))
    assert np.all(np.abs(hi - v) <= 2.0 ** -8 * np.abs(v))


def test_the_f16_split_model_is_the_closer_one_on_the_golden_weights():
    for index in (6, 8):                                          # 16 / 9 and 16 / 10
        r = lat.references(index, "g1")
        e16, ebf = lat.e_split(r["f16x3"], r["ref64"]), lat.e_split(r["bf16x3"], r["ref64"])
        e32 = float((r["ref32"].double() - r["ref64"]).abs().max())
        print(f"{lat.CASES[index].id}: e_split f16x3 {e16:.3e}, bf16x3 {ebf:.3e}, e32 {e32:.3e}")
        assert 0.0 < e16 < ebf
        assert ebf < 1e-4                                          # and both are roundings, not another function
