"""What tests/test_train_overlap_gpu.py shares: the seeded models and batches of the Trainer's forking branches (the shipped module
types at the smallest shapes each branch accepts), the probes put around the model's encoders, the runner that collects a run's
losses, gradients, parameters and buffers, and the rule that holds an overlapped run to the one-stream runs."""
import copy
import os
import types

import numpy as np
import torch

import synth_mano
from conftest import GOLDEN

GATE = 8.0                    # the project's gate factor: d(O, A) <= GATE * d(A', A) where the one-stream runs A, A' differ
DEV = "cuda:0"
MANO_KW = dict(center_idx=9, flat_hand_mean=False, ncomps=45, side="right", use_pca=False, root_rot_mode="axisang",
               joint_rot_mode="axisang", robust_rot=False, return_transf=False)
SMALL_IMG = (40, 30)          # tactile images where only the Resnet18 reads them: odd planes after the third stride (40 -> 20 -> 10 -> 5 -> 3 -> 2)
FULL_IMG = (320, 240)         # where the t2d net trains: its depth prediction is compared with the 320 x 240 depth readings


def _model_cfg(mano_root, tactile, t2d):
    # (start_filts 32 and c_dim 32: the narrowest plane U-Net that runs on the HIP kernels, forward and backward, with a fresh workspace
    #  per forward -- for the hand encoder and for the t2d net's digit-pose regressor below, which then runs the hand encoder's kernels at
    #  the hand encoder's shapes on the caller's stream; MIOpen's weight gradients under the nn modules are not reproducible)
    hand = {"hidden_dim": 32, "plane_type": ["xz", "xy", "yz"], "plane_resolution": 32, "unet": True,
            "unet_kwargs": {"depth": 2, "merge_mode": "concat", "start_filts": 32}, "out_mano": True}
    m = {"c_dim": 32, "decoder": "simple_local", "decoder_kwargs": {"sample_mode": "bilinear", "hidden_size": 32},
         "encoder": "pointnet_local_pool",
         "encoder_kwargs": {"hidden_dim": 32, "plane_type": "grid", "grid_resolution": 32, "unet3d": True,
                            "unet3d_kwargs": {"num_levels": 3, "f_maps": 32, "in_channels": 32, "out_channels": 32}},
         "encoder_hand": "pointnet_local_pool",
         "encoder_hand_kwargs": dict(hand, out_dim=51, manolayer_kwargs=dict(MANO_KW, mano_root=mano_root))}
    if tactile:
        m.update({"with_img": True, "encoder_img": "Resnet18", "encoder_img_kwargs": {"num_classes": 32}})
    if t2d:
        m.update({"encoder_t2d": True,
                  "encoder_t2d_kwargs": {"pretrained": False, "encoder_img": "UNet",
                                         "encoder_img_kwargs": {"num_classes": 1, "in_channel": 3, "start_filts": 8, "depth": 2},
                                         "encoder_hand": "pointnet_local_pool", "encoder_hand_kwargs": dict(hand, c_dim=32, out_dim=30)}})
    return {"data": {"dim": 3, "padding": 0.1, "input_type": "pointcloud", "num_sample": 640}, "test": {"threshold": 0.5}, "model": m}


def _batch(seed, img_hw=None, n_query=900):
    """2 scenes, 300 input points; ``img_hw``: the t2d keys as well (the fixtures' depth images, sensor poses and meshes)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(2, 300, 3, generator=g)
    b = {"inputs": 0.3 * d / d.norm(dim=-1, keepdim=True), "points": (torch.rand(2, n_query, 3, generator=g) - 0.5) * 1.1,
         "points.mano": torch.randn(2, 51, generator=g) * 0.2, "points.pc_hand": torch.randn(2, 778, 3, generator=g) * 0.05}
    b["points.occ"] = (torch.rand(2, n_query, generator=g) < 0.4).float()
    if img_hw is not None:
        z12 = np.load(os.path.join(GOLDEN, "g12_t2d.npz"))
        z13 = np.load(os.path.join(GOLDEN, "g13_trainer_t2d.npz"))
        b.update({"points.name": ["cube", "tet"], "points.cam_pos": torch.from_numpy(z13["cam_pos"]), "points.cam_rot": torch.from_numpy(z13["cam_rot"]),
                  "inputs.pc_ply": torch.from_numpy(z13["pc_ply"]), "inputs.img": torch.rand(2, 5, 3, *img_hw, generator=g),
                  "inputs.depth": torch.from_numpy(np.stack([z12["depths"], np.roll(z12["depths"], 7, axis=0)])),
                  "inputs.touch_success": torch.from_numpy(z13["touch"])})
    return b


#   name: (Trainer's step, tactile encoder, t2d net, t2d net under training, tactile image size, query points)
CASES = {"a": ("compute_loss", False, False, None, None, 203),
         "b": ("compute_loss_t2d", False, True, True, FULL_IMG, 900),
         "c_joint": ("compute_loss_t2d_img", True, True, True, FULL_IMG, 900),
         "c_pretrained": ("compute_loss_t2d_img", True, True, False, SMALL_IMG, 900)}


def build_case(name, tmp):
    """The seeded model (never stepped: every run works on a deepcopy), the batches by seed and what makes a Trainer for a copy."""
    from vtaco_amd.conv_onet import config as cfgmod
    step, tactile, t2d, joint, img_hw, n_query = CASES[name]
    mano_root = os.path.join(str(tmp), "mano")
    if not os.path.isdir(mano_root):
        synth_mano.write_pkl(synth_mano.make_asset(0), mano_root)
    cfg = _model_cfg(mano_root, tactile, t2d)
    torch.manual_seed(0)
    model0 = cfgmod.get_model(cfg, device=torch.device(DEV))
    vf = depth_origin = None
    if t2d:
        z13 = np.load(os.path.join(GOLDEN, "g13_trainer_t2d.npz"))
        vf = {"cube": {"v": z13["cube_v"], "f": z13["cube_f"]}, "tet": {"v": z13["tet_v"], "f": z13["tet_f"]}}
        depth_origin = np.load(os.path.join(GOLDEN, "g12_t2d.npz"))["depth_origin"]
    trainer_cfg = copy.deepcopy(cfg)
    if t2d:
        trainer_cfg["model"]["encoder_t2d_kwargs"]["pretrained"] = not joint       # (the Trainer's flag alone: a frozen t2d net is not run)

    def trainer_for(model, grad_sync=None):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        trainer = cfgmod.get_trainer(model, opt, trainer_cfg, torch.device(DEV), depth_origin=depth_origin)
        assert trainer.encode_t2d == t2d and trainer.with_img == tactile and (not t2d or trainer.pretrained_t2d == (not joint))
        trainer.grad_sync = grad_sync
        return trainer
    return types.SimpleNamespace(name=name, step=step, model0=model0, vf=vf, tactile=tactile, trainer_for=trainer_for,
                                 batch=lambda seed=2: _batch(seed, img_hw, n_query))


class Probes:
    """Wrappers around ``model.encode_inputs`` (the caller's stream), ``encode_hand_inputs`` and ``encode_img_inputs`` (the side
    sections): each notes the stream it runs on; ``sleep_side`` / ``sleep_caller`` hold that stream back by so many cycles before
    the encoder runs; ``raise_in`` names the method ('decode', 'decode_img', 'encode_hand_inputs') whose next call raises ``error``."""

    def __init__(self, sleep_side=0, sleep_caller=0, raise_in=None):
        self.sleep_side, self.sleep_caller, self.raise_in = int(sleep_side), int(sleep_caller), raise_in
        self.streams = {"encode_inputs": [], "encode_hand_inputs": [], "encode_img_inputs": []}
        self.error = RuntimeError("raised by the test between fork and join")

    def install(self, model):
        def wrap(name, sleep):
            inner = getattr(model, name)

            def call(*args, **kw):
                if name in self.streams:
                    self.streams[name].append(torch.cuda.current_stream().cuda_stream)
                if self.raise_in == name:
                    self.raise_in = None
                    raise self.error
                if sleep:
                    torch.cuda._sleep(sleep)
                return inner(*args, **kw)
            setattr(model, name, call)
        wrap("encode_inputs", self.sleep_caller)
        wrap("encode_hand_inputs", self.sleep_side)
        wrap("encode_img_inputs", self.sleep_side)
        if self.raise_in in ("decode", "decode_img"):
            wrap(self.raise_in, 0)


def snapshot(model, what):
    """{name: CPU copy} of every gradient ('grad': None where a parameter has none) or of every parameter and buffer ('state')."""
    if what == "grad":
        return {"grad/" + n: None if p.grad is None else p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    out = {"param/" + n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    out.update({"buffer/" + n: b.detach().cpu().clone() for n, b in model.named_buffers()})
    return out


def seed_all(seed=0):
    np.random.seed(seed)                          # the contact clouds' draws
    torch.manual_seed(seed)


def run_steps(case, batch, steps, probes=None, stream=None, grad_sync=None):
    """``steps`` train_steps with Adam on a copy of the case's seeded model, under whatever VTACO_TRAIN_OVERLAP says now -> (record,
    trainer).  The record: every step's returned losses, every gradient after step 1, every parameter and buffer after the last step.
    ``stream``: the steps run with it as the current stream, behind everything the default stream has queued."""
    model = copy.deepcopy(case.model0)
    if probes is not None:
        probes.install(model)
    trainer = case.trainer_for(model, grad_sync)
    rec = {}
    default = torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(default)
    state = np.random.get_state()
    try:
        seed_all()
        with torch.cuda.stream(stream if stream is not None else default):
            for k in range(steps):
                losses = trainer.train_step(batch, case.vf) if case.vf is not None else trainer.train_step(batch)
                rec[f"losses/step{k + 1}"] = torch.tensor(losses, dtype=torch.float64)
                if k == 0:
                    rec.update(snapshot(model, "grad"))
            rec.update(snapshot(model, "state"))
        if stream is not None:
            default.wait_stream(stream)
    finally:
        np.random.set_state(state)
    return rec, trainer


def same_bits(x, y):
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    return torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))


def rel(x, y):
    """d(X, Y) = ||X - Y||_2 / ||Y||_2 in float64 (inf where Y is zero and X is not)."""
    x, y = x.double().reshape(-1), y.double().reshape(-1)
    num, den = float((x - y).norm()), float(y.norm())
    if not (np.isfinite(num) and np.isfinite(den)):
        return float("inf")
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def hold_to_one_stream(case, A, A2, O, strict=False):
    """The rule per tensor: where the one-stream runs A and A' are equal bit for bit, O equals A bit for bit; otherwise
    d(O, A) <= GATE * d(A', A), integer tensors equal regardless.  ``strict``: the one-stream runs must themselves be equal bit for
    bit everywhere.  Prints the RATIO lines and the BITS line; returns the names of the tensors under the looser rule."""
    assert A.keys() == A2.keys() == O.keys() and len(A) > 0
    loose, failures, equal = [], [], 0
    for name in A:
        a, a2, o = A[name], A2[name], O[name]
        if a is None or a2 is None or o is None:
            if not (a is None and a2 is None and o is None):
                failures.append(f"{name}: present in one run and missing in another")
            equal += a is None and o is None
            continue
        if same_bits(a, a2) or not a.dtype.is_floating_point:
            if not same_bits(a, a2):
                failures.append(f"{name}: integer tensor differs between the one-stream runs")
            if same_bits(o, a):
                equal += 1
            else:
                failures.append(f"{name}: one-stream runs equal bit for bit, overlapped run differs, d(O,A) = {rel(o, a):.3e}")
            continue
        loose.append(name)
        d_ref, d_got = rel(a2, a), rel(o, a)
        equal += same_bits(o, a)
        print(f"RATIO {case} {name}: {d_got:.3e} / {d_ref:.3e} = {d_got / d_ref if d_ref > 0 else float('inf'):.3f}")
        if not d_got <= GATE * d_ref:
            failures.append(f"{name}: d(O,A) = {d_got:.3e} > {GATE} * d(A',A) = {GATE * d_ref:.3e}")
    print(f"BITS {case}: {equal} of {len(A)} tensors equal bit for bit ({len(loose)} differ between the one-stream runs)")
    assert not failures, f"{case}: " + "; ".join(failures[:12]) + (f" ... {len(failures)} in all" if len(failures) > 12 else "")
    if strict:
        assert not loose, f"{case}: the one-stream step is not reproducible bit for bit in {loose[:12]} ({len(loose)} tensors)"
    return loose
