"""Multi-touch reconstruction (drop-in for reference src/conv_onet/inferencing.py: ``Inferencer.inference_img`` :82-183 for VTacOH,
``inference_img_t2d`` :185-325 for VTacO): an object is reconstructed from the first touch and refined touch after touch.

The reference keeps a dense ``c_img_all [1, nx^3, C]`` across the touches, fills it through CPU cdist passes and decodes all nx^3
points again after every touch.  Here the session lives on the device as one byte per lattice point (the row of a feature table,
``vt_touch_merge``), and -- a concat decoder's logit at a point depends on the point, ``c`` and that point's row only -- a later
touch decodes just the points whose row it changed (a few thousand of 2 M) through the point path and scatters them into the
value lattice it keeps.
"""
from __future__ import annotations

import torch

from .. import ops
from .._lib import VtError
from .generation import _range_guarded

ROWS_PER_TOUCH = 5                       # the reference's five fingers (inferencing.py:162, 281)


@_range_guarded
def _guarded(generator, run):
    """``run()`` under the generator's half-precision range guard: the guard may move ``generator.decode_precision`` and call again."""
    return run()


class _Session(object):
    """Device state of one object: ``c`` (touch 0's), the id lattice, the row table, the value lattice, the merge's buffers."""
    __slots__ = ("c", "nx", "ids", "feats", "values", "touches", "precision", "capacity", "changed_ids", "changed_pts", "n_changed",
                 "workspace", "changed")


class Inferencer(object):
    """Constructor arguments as the reference (inferencing.py:36-38), plus ``incremental`` (keyword, default True): False decodes the
    whole lattice from the merged ids on every touch -- the fall-back, and the yardstick of the incremental path.

    ``inference_step(data_vis_class) -> (mesh_list_obj, mesh_list_hand)`` takes the reference's list of ``{'data': sample, ...}``,
    one entry per touch, and returns one object ``Mesh`` and one hand ``Mesh`` per touch (``generation.Mesh``: ``export`` as
    trimesh's).  It is ``reset()`` plus ``add_touch(data) -> (mesh_obj, mesh_hand)`` per entry; a robot that gets its touches one at
    a time calls those two itself.  ``inference()`` returns None, as the reference's.

    Reference behaviour that is kept:
      - ``c`` is encoded once, from the FIRST touch's ``inputs``; later touches never re-encode the shape (:155-158, :274-277);
      - the VTacO (t2d) route unprojects the DATASET's depth images, not the predicted ones (:286 overwrites :284-285);
      - its ``np.random.randint`` draws (contact clouds above 128 points) come from numpy's global generator and run on through
        the sequence: seed once in front of ``inference_step``, not per touch;
      - a finger whose touch failed writes nothing: the rows earlier touches left at those points stay in place;
      - the lattice is ``nx = resolution0 * 4`` points per axis, whatever ``upsampling_steps`` says (:92);
      - marching cubes at scikit-image's default level (the mean of the field's extremes), ``gradient_direction='ascent'``, then
        ``-nx/2, (1+padding)/nx`` (:174-178).
    The hand mesh of a touch is ``Generator3D.generate_hand_mesh``'s arithmetic; in the VTacOH route the hand encoder runs once per
    touch and serves both the fingertips and the mesh.  A model without a hand encoder (the t2d route does not need one for the
    object) gives ``None`` as that touch's hand mesh.

    The session holds at most 254 rows, five per touch: a 51st touch raises VtError before anything is launched (``reset()`` starts
    over; rows that no point refers to any more are not recycled).

    Refused with VtError: a generator with ``extraction="mise"`` (the session's lattice is the dense one); ``group=`` (the sharded
    entry points: the lattices of a session live on one device); a batch of more than one scene; a configuration without
    ``with_img`` (the reference has no such route: it fails there with an unbound name).  The attention decoder
    (``attention_local``) couples the points of a chunk, so its session decodes the whole lattice from the merged ids on every touch
    (``Generator3D._eval_lattice_fused``), whatever ``incremental`` says.

    Each touch's decode runs under the generator's half-precision range guard; when the guard (or the caller) moves
    ``decode_precision`` between touches, the next touch decodes the whole lattice again in the new arithmetic, so a value lattice
    never mixes two.  With ``decode_precision="f32"`` the incremental session is bit for bit the whole-lattice decode (the f32 point
    path is the lattice kernel's arithmetic); with the split-f16 forms the two paths agree to 1e-4, the project's standing contract,
    so entries decoded by different touches may differ from a whole-lattice decode in the last bits."""

    def __init__(self, model, optimizer, generator, device=None, input_type='pointcloud', vis_dir=None, threshold=0.5,
                 eval_sample=False, num_sample=2048, with_img=False, with_contact=False, train_tactile=False, encode_t2d=False,
                 *, incremental=True):
        self.model, self.optimizer, self.generator, self.device = model, optimizer, generator, device
        self.input_type, self.vis_dir, self.threshold = input_type, vis_dir, threshold
        self.eval_sample, self.num_sample = eval_sample, num_sample
        self.with_img, self.with_contact, self.train_tactile, self.encode_t2d = with_img, with_contact, train_tactile, encode_t2d
        self.incremental = incremental
        self.resolution0, self.padding = generator.resolution0, generator.padding
        self._check_generator()
        self._session = None
        self.changed_points = []             # per touch of the current session: length of its changed list (-1: whole lattice decoded, not read)

    # -- public interface -----------------------------------------------------------------------------------------------------
    def inference(self, data_vis_class):
        return None

    def inference_step(self, data_vis_class, group=None):
        """One object: ``data_vis_class`` is a list of ``{'data': sample dict, ...}``, one per touch, in the order they were made."""
        self._check_route(group)
        self.reset()
        mesh_list_obj, mesh_list_hand = [], []
        for data_vis in data_vis_class:
            mesh_obj, mesh_hand = self.add_touch(data_vis['data'])
            mesh_list_obj.append(mesh_obj)
            mesh_list_hand.append(mesh_hand)
        return mesh_list_obj, mesh_list_hand

    def reset(self):
        """Forget the object: the next ``add_touch`` is touch 0 (it encodes ``c`` and starts from an empty lattice)."""
        self._session = None
        self.changed_points = []

    def add_touch(self, data, group=None):
        """The next touch of the current object -> (object mesh, hand mesh) after it."""
        self._check_route(group)
        gen = self.generator
        k = 0 if self._session is None else self._session.touches
        if ROWS_PER_TOUCH * (k + 1) > ops.TOUCH_MAX_ROWS:           # before any launch
            raise VtError(f"Inferencer: a session holds {ops.TOUCH_MAX_ROWS // ROWS_PER_TOUCH} touches ({ops.TOUCH_MAX_ROWS} rows of "
                          f"{ROWS_PER_TOUCH}); this is touch {k + 1}.  reset() starts a new session")
        inputs = data.get('inputs', torch.empty(1, 0))
        if inputs.shape[0] != 1:
            raise VtError(f"Inferencer: one scene at a time (got a batch of {inputs.shape[0]})")
        gen._eval_mode()
        if k == 0:
            c, setup = gen._tactile_encode(data)                    # shape, tactile and hand encoders overlapped
            self._session = self._new_session(c, setup)
        else:
            setup = self._setup_only(data)                          # no shape encoder: c stays touch 0's
        mesh_hand = self._hand_mesh(data, setup)
        s = self._session
        with torch.no_grad():
            self._merge(s, setup, k)
            mesh_obj = _guarded(gen, lambda: self._decode(s, k))
        s.touches = k + 1
        self.changed_points.append(s.changed)
        return mesh_obj, mesh_hand

    # -- checks -----------------------------------------------------------------------------------------------------------------
    def _check_generator(self):
        if getattr(self.generator, "extraction", "dense") != "dense":
            raise VtError("Inferencer: the session keeps the dense nx^3 lattice; the generator has extraction='mise' "
                          "(use a generator with extraction='dense')")
        from .models.decoder import LocalPointDecoder
        if isinstance(getattr(self.model, "decoder", None), LocalPointDecoder):
            raise VtError("Inferencer: the PointConv baseline (pointnet_plus_plus / simple_local_point) has no tactile variant, and the "
                          "session's touches are tactile features merged into the lattice")
        enc = getattr(self.model, "encoder", None)
        if enc is not None and getattr(enc, "planes", ['grid']) != ['grid']:
            raise VtError(f"Inferencer: the encoder returns plane features {enc.planes}; the session's incremental decodes read the finger "
                          "features in vt_decode_fwd_ids, which samples the 'grid' volume only")

    def _check_route(self, group):
        if not self.with_img:
            raise VtError("Inferencer: only the with_img routes exist (VTacOH, and VTacO with encode_t2d), as in the reference")
        if group is not None:
            raise VtError("Inferencer: a session's lattices live on one device; there is no sharded form (group must be None)")
        self._check_generator()
        gen = self.generator
        if not gen.with_img or bool(gen.encode_t2d) != bool(self.encode_t2d):
            raise VtError("Inferencer: the generator must be built for the same route (with_img, encode_t2d) as the inferencer")

    # -- one touch ------------------------------------------------------------------------------------------------------------
    def _setup_only(self, data):
        """``Generator3D._tactile_setup`` with the encoders on the side streams, as ``_tactile_encode`` runs them, minus the shape encoder."""
        gen = self.generator
        sides = gen._side_streams()
        if sides is None:
            return gen._tactile_setup(data)
        cur = torch.cuda.current_stream(gen.device)
        for side in sides:
            side.wait_stream(cur)
        setup = gen._tactile_setup(data, sides)()
        for side in sides:
            cur.wait_stream(side)
        return setup

    def _hand_mesh(self, data, setup):
        gen = self.generator
        if getattr(gen.model, 'encoder_hand', None) is None:
            return None
        if setup.get('c_hand') is not None:                         # VTacOH: the hand encoder has just run for the fingertips
            return gen._hand_mesh_of(setup['c_hand'], data.get('inputs.pc_ply').to(gen.device))
        return gen.generate_hand_mesh(data)

    def _new_session(self, c, setup):
        gen = self.generator
        dev = gen.device
        s = _Session()
        # (the encoder's output lives in a captured graph's static buffers: the session keeps its own copy)
        s.c = {key: val.clone() for key, val in c.items()} if isinstance(c, dict) else c.clone()
        s.nx = nx = gen.resolution0 * 4                             # inferencing.py:92
        s.ids = torch.full((nx ** 3,), 255, dtype=torch.uint8, device=dev)
        s.feats = torch.zeros((ops.TOUCH_MAX_ROWS, int(setup['feats'].shape[-1])), dtype=torch.float32, device=dev)
        s.values, s.touches, s.precision, s.changed = None, 0, None, 0
        s.capacity = 1 << 16
        s.changed_ids = torch.empty(s.capacity, dtype=torch.int32, device=dev)
        s.changed_pts = torch.empty((s.capacity, 3), dtype=torch.float32, device=dev)
        s.n_changed = torch.zeros(1, dtype=torch.int32, device=dev)
        s.workspace = ops.touch_workspace(nx, dev)
        return s

    def _merge(self, s, setup, k):
        """Touch k's rows into the table, its assignment into the id lattice; ``s.changed`` = the length of the changed list
        (touch 0 decodes the whole lattice and does not read it back: -1)."""
        gen = self.generator
        dev = gen.device
        anchors = setup['anchors'].to(dev)
        if anchors.shape[0] != ROWS_PER_TOUCH:
            raise VtError(f"Inferencer: a touch has {ROWS_PER_TOUCH} fingers (got {anchors.shape[0]})")
        base = ROWS_PER_TOUCH * k
        s.feats[base:base + ROWS_PER_TOUCH].copy_(setup['feats'].to(dev).float().reshape(ROWS_PER_TOUCH, -1))
        args = (s.ids, anchors, setup['success'].to(dev), setup['mode'], setup['radius'], s.nx, 1 + gen.padding, base)
        kw = dict(count=setup['count'].to(dev), n_changed=s.n_changed, workspace=s.workspace)
        ops.touch_merge(*args, s.capacity, changed_ids=s.changed_ids, changed_pts=s.changed_pts, **kw)
        if k == 0 or not self._incremental():
            s.changed = -1
            return
        n = int(s.n_changed.item())                                 # the one host read of a later touch
        if n > s.capacity:                                          # a longer list than any so far: size up, list again (the
            s.capacity = n                                          # merge itself is done and gives the same list)
            s.changed_ids = torch.empty(n, dtype=torch.int32, device=dev)
            s.changed_pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
            ops.touch_merge(*args, s.capacity, changed_ids=s.changed_ids, changed_pts=s.changed_pts, **kw)
        s.changed = n

    def _incremental(self):
        return bool(self.incremental) and not hasattr(self.generator.model.decoder, 'fuser')

    def _rows(self, s, k):
        return s.feats[:ROWS_PER_TOUCH * (k + 1)]

    def _decode_whole(self, s, k):
        """The whole value lattice from the merged ids and the table."""
        gen = self.generator
        dec = gen.model.decoder
        nx = s.nx
        if hasattr(dec, 'fuser'):
            return gen._eval_lattice_fused(s.c, nx, s.ids.view(1, -1), self._rows(s, k), 0, nx ** 3)
        grid = s.c['grid'] if isinstance(s.c, dict) else s.c
        return dec.decode_lattice_ids(grid, nx, s.ids.view(1, -1), self._rows(s, k), box=1 + gen.padding,
                                      precision=gen.decode_precision).reshape(-1)

    def _decode(self, s, k):
        """Touch k's value lattice and mesh.  Runs again when the range guard has moved the precision: then (as whenever the
        precision is not the one the kept lattice was decoded in) the whole lattice is decoded."""
        gen = self.generator
        whole = s.changed < 0 or s.values is None or s.precision != gen.decode_precision
        if whole:
            s.values = self._decode_whole(s, k)
            s.precision = gen.decode_precision
        elif s.changed > 0:
            n = s.changed
            dec = gen.model.decoder
            grid = s.c['grid'] if isinstance(s.c, dict) else s.c
            prec = gen._mise_precision()
            idx = s.changed_ids[:n]
            pts = s.changed_pts[:n].view(1, n, 3)
            fid = s.ids[idx.long()].view(1, n)                      # the rows of the listed points, from the lattice
            if dec._wide:
                logits = dec._wide_fwd(grid, precision=prec, pts=pts, finger_ids=fid, finger_feats=self._rows(s, k))
            else:
                logits = ops.decode_fwd_ids(grid, dec._blob(img=True, precision=prec), fid, self._rows(s, k), pts=pts,
                                            padding=dec.padding, precision=prec)
            ops.mise_scatter(s.values, idx, logits.reshape(-1))
        return gen.extract_mesh(s.values.view(s.nx, s.nx, s.nx), with_normals=False)     # (the Inferencer ignores with_normals)

    # -- what the tests and tools read --------------------------------------------------------------------------------------
    @property
    def session(self):
        """The current session's device state (None before the first touch): ``ids`` u8 [nx^3], ``feats`` [254, C], ``values`` f32
        [nx^3], ``changed_ids`` / ``changed_pts`` (the last touch's list, ``changed_points[-1]`` entries), ``touches``."""
        return self._session
