"""CPU: the float64 restatement of the PointConv baseline (tests/pointconv_ref.py) reproduces the golden made from the real
reference (tests/golden/g26_pointconv.npz), the registries hold both names, and the mirror modules carry the reference's
state_dict keys and shapes.

Tolerance: the golden is a float32 evaluation, so it may differ from float64 by what float32 arithmetic costs on these tensors.
That is measured here by the same restatement in float32, e32 = max |ref32 - ref64| per tensor, and the golden has to lie within
MARGIN = 4 of it.  Measured once (torch 2.x CPU): encoder features eval 9.6e-8 (golden 2.1e-7) at scale 0.45, train 7.5e-5
(golden 1.0e-4) at scale 5.3 -- batch statistics over small-variance channels amplify; decoder logits 9.9e-8 / 1.2e-7 (golden
6.7e-8 / 1.0e-7, gaussian / inverse); parameter gradients 1.6e-7 / 2.6e-7 (golden 1.8e-7 / 2.9e-7); feature gradient 4.0e-10 /
3.5e-10 at scale 1.8e-3 / 6.9e-4 (golden the same)."""
import pytest
import torch

import pointconv_ref as R
from seeded_fill import keys_of


@pytest.fixture(scope="module")
def gold():
    return R.golden()


def _models():
    from vtaco_amd.conv_onet.models import decoder_dict
    from vtaco_amd.encoder import encoder_dict
    return encoder_dict, decoder_dict


def _close(got, r64, r32, what):
    e32 = float((r32.double() - r64).abs().max())
    err = float((got.double().reshape(r64.shape) - r64).abs().max())
    print(f"{what}: |golden - f64| = {err:.3e}, e32 = {e32:.3e}")
    assert e32 > 0 and err <= R.MARGIN * e32, f"{what}: {err:.3e} > {R.MARGIN} x {e32:.3e}"


def test_registries_hold_both_names():
    encoder_dict, decoder_dict = _models()
    from vtaco_amd._lib import VtError
    enc = encoder_dict["pointnet_plus_plus"](dim=3, c_dim=32, padding=0.1)
    dec = decoder_dict["simple_local_point"](dim=3, c_dim=32, hidden_size=32, padding=0.1, with_contact=False, gaussian_val=0.1)
    assert type(enc).__name__ == "PointNetPlusPlus" and type(dec).__name__ == "LocalPointDecoder"
    decoder_dict["simple_local_point"](sample_mode="inverse")                    # the class defaults 128 / 256, no gaussian_val needed
    for bad in (dict(dim=2, gaussian_val=0.1), dict(c_dim=0, gaussian_val=0.1), dict(hidden_size=48, gaussian_val=0.1),
                dict(c_dim=288, gaussian_val=0.1), dict()):
        with pytest.raises(VtError):
            decoder_dict["simple_local_point"](**bad)
    with pytest.raises(VtError):                                                 # no CPU path
        dec(torch.zeros(1, 4, 3), (torch.zeros(1, 5, 3), torch.zeros(1, 5, 32)))
    with pytest.raises(VtError):
        dec.forward_img(None, None, None)
    with pytest.raises(VtError):
        dec.forward_contact(None, None)
    with pytest.raises(VtError):
        enc(torch.zeros(1, 600, 3))
    with pytest.raises(KeyError):
        decoder_dict["simple_local_crop"]
    with pytest.raises(KeyError):
        encoder_dict["pointnet_crop_local_pool"]


def test_state_dict_keys_and_shapes(gold):
    encoder_dict, decoder_dict = _models()
    assert keys_of(encoder_dict["pointnet_plus_plus"](dim=3, c_dim=32, padding=0.1)) == gold["enc.keys"]
    for tag, kw in R.MODES:
        assert keys_of(decoder_dict["simple_local_point"](dim=3, c_dim=32, hidden_size=32, **kw)) == gold[f"dec.{tag}.keys"]


def test_get_model_builds_the_pair():
    from vtaco_amd.conv_onet import config
    cfg = {"data": {"dim": 3, "padding": 0.1},
           "model": {"encoder": "pointnet_plus_plus", "decoder": "simple_local_point", "c_dim": 32, "encoder_kwargs": {},
                     "decoder_kwargs": {"hidden_size": 32, "sample_mode": "gaussian", "gaussian_val": 0.1}}}
    model = config.get_model(cfg, device=None)
    assert type(model.encoder).__name__ == "PointNetPlusPlus" and type(model.decoder).__name__ == "LocalPointDecoder"


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_encoder_restatement_reproduces_golden(gold, mode):
    from vtaco_amd.encoder import encoder_dict
    sd = R.fill(encoder_dict["pointnet_plus_plus"](dim=3, c_dim=32), R.SEED_ENC).state_dict()
    starts = gold[f"enc.{mode}.starts"]
    f64, tr64 = R.encoder(sd, gold["cloud"], starts, train=mode == "train", dtype=torch.float64)
    f32, tr32 = R.encoder(sd, gold["cloud"], starts, train=mode == "train", dtype=torch.float32)
    assert all(torch.equal(a, b) for a, b in zip(tr64, tr32))                    # the geometry does not hinge on the precision
    _close(gold[f"enc.{mode}.fea"], f64, f32, f"encoder features ({mode})")


@pytest.mark.parametrize("tag,kw", R.MODES)
def test_decoder_restatement_reproduces_golden(gold, tag, kw):
    from vtaco_amd.conv_onet.models import decoder_dict
    sd = R.fill(decoder_dict["simple_local_point"](dim=3, c_dim=32, hidden_size=32, **kw), R.SEED_DEC).state_dict()
    args = (sd, gold["queries"], gold["cloud"], gold["enc.eval.fea"], gold["occ"], kw["sample_mode"], kw.get("gaussian_val"))
    r64, r32 = R.decoder(*args, dtype=torch.float64), R.decoder(*args, dtype=torch.float32)
    _close(gold[f"dec.{tag}.logits"], r64["logits"], r32["logits"], f"logits ({tag})")
    _close(gold[f"dec.{tag}.grad.fea"], r64["grad_fea"], r32["grad_fea"], f"feature gradient ({tag})")
    for name in sd:
        _close(gold[f"dec.{tag}.grad.{name}"], r64["grads"][name], r32["grads"][name], f"grad {name} ({tag})")


def test_unshifted_form_agrees_where_finite_and_is_nan_far_away(gold):
    q, cloud, fea = gold["queries"][:, :64], gold["cloud"], gold["enc.eval.fea"]
    ref, s = R.sample_unshifted(q, cloud, fea, "gaussian", 0.1, torch.float64)
    assert float(s.min()) > 0
    assert float((ref - R.sample(q, cloud, fea, "gaussian", 0.1, torch.float64)).abs().max()) < 1e-12
    far = q + 5.0
    bad, s = R.sample_unshifted(far, cloud, fea, "gaussian", 0.1, torch.float32)
    assert float(s.max()) == 0 and bool(torch.isnan(bad).all())
    assert bool(torch.isfinite(R.sample(far, cloud, fea, "gaussian", 0.1, torch.float32)).all())
