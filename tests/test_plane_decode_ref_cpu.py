"""CPU: tests/plane_decode_ref.py reproduces the real reference's LocalDecoder on plane features (tests/golden/g21_plane_decode.npz:
logits and the gradients of logits.sum()) to 2e-5, the bar of g20's CPU test; and the host-only part of the new C entries: they are in
the signature table, and bad arguments come back as error codes before any GPU call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_decode_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMPLE_SEED = 2000          # tests/golden/make_attn_wide_goldens.py: sample_index


def sample_index(name, numel):
    g = torch.Generator().manual_seed(SAMPLE_SEED + sum(map(ord, name)))
    return torch.randint(0, numel, (64,), generator=g)


def load_case(tag):
    z = np.load(os.path.join(GOLDEN, "g21_plane_decode.npz"))
    keys = str(z[f"{tag}.keys"]).split(",")
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32))
    case = {"keys": keys, "p": t(z[f"{tag}.p"]), "logits": t(z[f"{tag}.logits"]),
            "c_plane": {k: t(z[f"{tag}.c.{k}"]) for k in keys},              # in the fixture's (shuffled) order
            "grad": {k: t(z[f"{tag}.grad.{k}"]) for k in keys},
            "sd": {n[len(tag) + 4:]: t(z[n]) for n in z.files if n.startswith(f"{tag}.sd.")},
            "pgrad": {n[len(tag) + 7:]: z[n] for n in z.files if n.startswith(f"{tag}.pgrad.")},
            "leaky": tag == "B"}
    return case


@pytest.mark.parametrize("tag", ["A", "B"])
def test_ref_reproduces_the_real_decoder(tag):
    c = load_case(tag)
    far = (c["p"].abs() >= 0.56).all(-1).sum(1)
    assert int(far.min()) >= 8 and bool((c["p"] >= 0.56).any()) and bool((c["p"] <= -0.56).any())
    logits, gf, gp = ref.grads(c["sd"], c["p"], c["c_plane"], leaky=c["leaky"])
    assert float((logits - c["logits"]).abs().max()) <= 2e-5
    for k in c["keys"]:
        assert float((gf[k] - c["grad"][k]).abs().max()) <= 2e-5 * max(1.0, float(c["grad"][k].abs().max())), k
    names = sorted({n.rsplit(".", 1)[0] for n in c["pgrad"]})
    assert len(names) == 2 + 6 * 5 + 2
    for name in names:
        g = gp[name].reshape(-1)
        s, sa = c["pgrad"][name + ".sum"]
        assert abs(float(g.sum()) - s) <= 2e-5 * max(1.0, sa), name
        got = g[sample_index(name, g.numel())]
        want = torch.from_numpy(c["pgrad"][name + ".samples"]).double()
        assert float((got - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max())), name


@pytest.mark.parametrize("tag", ["A", "B"])
def test_written_out_backward_is_autograd(tag):
    """mlp_backward + feature_grads from the float64 forward's own saves reproduce plane_decode_ref.grads (autograd) to rounding."""
    c = load_case(tag)
    _, gf, gp = ref.grads(c["sd"], c["p"], c["c_plane"], leaky=c["leaky"])
    feat = ref.features(c["c_plane"], c["p"])
    rx, rh, af = ref.mlp_saves(c["sd"], c["p"], feat, c["leaky"])
    g = ref.mlp_backward(c["sd"], c["p"], feat, rx, rh, af, torch.ones(c["p"].shape[:2]), c["leaky"])
    for name, want in gp.items():
        assert float((g[name] - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max())), name
    for k, got in ref.feature_grads(c["c_plane"], c["p"], g["grad_c"]).items():
        assert float((got - gf[k]).abs().max()) <= 1e-11 * max(1.0, float(gf[k].abs().max())), k
    bound = ref.mlp_backward(c["sd"], c["p"], feat, rx, rh, af, torch.ones(c["p"].shape[:2]), c["leaky"], absolute=True)
    assert all(bool((bound[k] >= g[k].abs() * (1 - 1e-12)).all()) for k in g)


def test_shuffled_dict_order_is_the_reference_order():
    c = load_case("B")
    assert c["keys"] == ["grid", "yz", "xz", "xy"]
    a = ref.features(c["c_plane"], c["p"])
    b = ref.features({k: c["c_plane"][k] for k in ("grid", "xz", "xy", "yz")}, c["p"])
    assert torch.equal(a, b)


NEW = ("vt_sample_planes", "vt_sample_planes_workspace_bytes", "vt_sample_planes_bwd", "vt_sample_planes_bwd_workspace_bytes")


def test_new_entries_are_bound_and_refuse_on_the_host():
    """No device is touched: a null plane set and C = 48 come back as VT_ERR_INVALID / VT_ERR_UNSUPPORTED from the argument checks."""
    from vtaco_amd import _lib
    for n in NEW:
        assert n in _lib.SIGNATURES, n
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()                        # host memory: never dereferenced, the checks come first
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    args = lambda xz, C: (xz, None, None, 1, 4, C, ptr, 4, 0, 0.0, 0, 0.1, 0, None, ptr, ptr, 1 << 30, None)
    assert lib.vt_sample_planes(*args(None, 32)) == -1
    assert b"no plane" in lib.vt_last_error()
    assert lib.vt_sample_planes(*args(ptr, 48)) == -2
    assert lib.vt_sample_planes(*args(ptr, 288)) == -2
    assert lib.vt_sample_planes_bwd(1, 4, 32, ptr, 4, 0.1, 0, ptr, None, None, None, ptr, 1 << 30, None) == -1
    assert lib.vt_sample_planes_bwd(1, 4, 48, ptr, 4, 0.1, 0, ptr, ptr, None, None, ptr, 1 << 30, None) == -2
    # a lattice whose nx^3 does not fit the kernels' 32-bit indices is refused, not wrapped
    lat = lambda nx: (ptr, None, None, 1, 4, 32, None, 4, nx, 1.1, 0, 0.1, 0, None, ptr, ptr, 1 << 40, None)
    assert lib.vt_sample_planes(*lat(1626)) == -2 and lib.vt_sample_planes(*lat(1)) == -1
    assert lib.vt_sample_planes_bwd(1, 4, 32, ptr, 4, 0.1, 4, ptr, ptr, None, None, ptr, 1 << 30, None) == -1      # VT_PLANES_PREPARED
    assert lib.vt_sample_planes_workspace_bytes(2, 9, 32, 3, 0) == 3 * 2 * 81 * 32 * 4
    assert lib.vt_sample_planes_workspace_bytes(2, 9, 32, 0, 0) == 0
