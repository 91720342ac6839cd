"""CPU: the touch session's accumulation rule against the real reference Inferencer (g23_touch.npz: both routes, four touches
of one object, the carried-over c_img_all after every touch), the get_inferencer factory, and the header's new symbols."""
import os
import re

import numpy as np
import pytest

import touch_rule as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("route", ["h", "d"])
def test_numpy_rule_reproduces_the_reference_lattice_after_every_touch(route):
    z = tr.fixture()
    nx = int(z["nx"])
    prev = np.full(nx ** 3, 255, dtype=np.uint8)
    rows_seen = set()
    for k, (anchors, count, success, ids, changed) in enumerate(tr.walk(z, route)):
        ref = tr.expected(z, route, k)
        assert np.array_equal(ids, ref), (route, k, int((ids != ref).sum()))
        assert np.array_equal(changed, np.nonzero(ref != prev)[0])            # the list = the points whose id differs
        assert success.any() and changed.size > 0
        assert set(np.unique(ref[changed]).tolist()) <= set(range(5 * k, 5 * k + 5))
        prev = ref
    # the fixture exercises what the session is for: later touches overwrite parts of earlier ones, every successful row survives
    # somewhere, and the last touch is sparse (the incremental decode's case)
    rows_seen = set(np.unique(prev[prev != 255]).tolist())
    ok_rows = {5 * k + t for k in range(tr.touches(z)) for t in range(5) if z[f"{route}.touch"][k, t]}
    assert rows_seen == ok_rows and len(ok_rows) == 17
    first = tr.expected(z, route, 0)
    assert int(((first != 255) & (prev != first)).sum()) > 0                   # an earlier row was overwritten
    assert changed.size < 0.01 * nx ** 3


def test_order_of_touches_matters_in_the_rule():
    z = tr.fixture()
    a = tr.walk(z, "h", [0, 1, 2])[-1][3]
    b = tr.walk(z, "h", [0, 2, 1])[-1][3]
    assert np.array_equal(a != 255, b != 255) and not np.array_equal(a, b)


def test_get_inferencer_builds_an_inferencer_from_a_config():
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config as cfgmod
    from vtaco_amd.conv_onet.inferencing import Inferencer

    class Gen(object):
        resolution0, padding, extraction, device = 8, 0.1, "dense", "cpu"

    cfg = {"test": {"threshold": 0.4}, "training": {"out_dir": "out/x", "eval_sample": False},
           "data": {"input_type": "pointcloud", "num_sample": 1024},
           "model": {"with_img": True, "with_contact": False, "train_tactile": False, "encoder_t2d": True}}
    gen = Gen()
    inf = cfgmod.get_inferencer(object(), None, gen, cfg, "cpu")
    assert isinstance(inf, Inferencer) and inf.generator is gen
    assert inf.with_img and inf.encode_t2d and not inf.with_contact and not inf.train_tactile
    assert inf.threshold == 0.4 and inf.num_sample == 1024 and inf.input_type == "pointcloud" and inf.incremental
    assert inf.vis_dir == os.path.join("out/x", "vis") and not os.path.exists(inf.vis_dir)     # nothing is created before it is needed
    assert inf.resolution0 == 8 and inf.padding == 0.1
    assert inf.inference([]) is None
    gen.extraction = "mise"
    with pytest.raises(VtError, match="mise"):
        cfgmod.get_inferencer(object(), None, gen, cfg, "cpu")
    gen.extraction = "dense"
    cfg["model"]["with_img"] = False
    with pytest.raises(VtError, match="with_img"):
        cfgmod.get_inferencer(object(), None, gen, cfg, "cpu").inference_step([])


def test_header_declares_the_touch_entry_points():
    text = open(os.path.join(ROOT, "include", "vtaco_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", text))
    assert {"vt_touch_merge", "vt_touch_workspace_bytes"} <= names           # tests/test_abi.py checks that they are exported and bound
    from vtaco_amd import _lib
    assert {"vt_touch_merge", "vt_touch_workspace_bytes"} <= set(_lib.SIGNATURES)
