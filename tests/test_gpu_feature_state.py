"""tests/feature_state_cases.py through the C ABI: every sequence on a context of its own, the flags read back through what the API shows
(the refusals of gbuffer_read, gbuffer_objects_read, mk_active_read, read_pixels(6) and reproject).  The same table runs through
csrc/flx_feature_state.h on the CPU in tests/test_feature_state.py.  No call here is refused by anything but an argument check on the host."""
import types
import numpy as np
import pytest
import common
import pose_cases as pc
import feature_state_cases as fs
from fluctus_amd import wire

pytestmark = pytest.mark.gpu
NO = 0xFFFFFFFF
POSES = {"I": pc.IDENTITY, "T": pc.affine(None, (0.1, 0.0, 0.0))}


@pytest.fixture(scope="module")
def scene():
    d = common.mixed_material_scene()
    d.tris.setflags(write=False)
    return d


def _objects(d, n):
    """mixed_material_scene's first n spheres (matId 3 + k) as objects 0 .. n-1"""
    m = d.tris["matId"].astype(np.int64)
    o = np.full(d.tris.size, NO, np.uint32)
    sel = (m >= 3) & (m < 3 + n)
    o[sel] = (m[sel] - 3).astype(np.uint32)
    return o


def _refuses(call, message):
    """False when the call goes through, True when it is refused with this message; any other refusal is an error"""
    try:
        call()
    except RuntimeError as e:
        assert message in str(e), str(e)
        return True
    return False


def _refusal(call):
    try:
        call()
    except RuntimeError as e:
        return str(e)
    return ""


class Run:
    def __init__(self, d):
        from fluctus_amd.device import HipContext
        self.d, self.g = d, HipContext(256)
        self.g.upload_scene(d)
        self.size(fs.W0, fs.H0)

    def size(self, W, H):
        self.p = common.scene_params(self.d, W, H)
        self.g.set_params(self.p)
        self.blank = np.zeros((W * H, 8), np.float32)
        self.blank[:, 3] = np.array([-1], np.int32).view(np.float32)[0]          # every pixel a miss

    def event(self, e):
        g, d, k = self.g, self.d, e[0]
        if k == "refused":
            with pytest.raises(RuntimeError, match=e[2]):
                self.event(e[1])
        elif k == "opt": g.set_option(e[1], e[2])
        elif k == "define": g.objects_define(d.tris, _objects(d, e[1]), e[1])
        elif k == "pose": g.objects_pose(sorted(e[1]), [POSES[e[1][o]] for o in sorted(e[1])])
        elif k == "gbuffer": g.gbuffer()
        elif k == "capture": g.history_capture()
        elif k == "gb_write": g.gbuffer_write(e[1], self.blank, self.p["camera"])
        elif k == "obj_write": g.gbuffer_objects_write(e[1], np.full(self.blank.shape[0], NO, np.uint32))
        elif k == "upload": g.upload_scene(d)
        elif k == "upload_refused":
            g.upload_scene(types.SimpleNamespace(tris=np.zeros(0, wire.TRIANGLE), indices=d.indices, nodes=d.nodes, materials=d.materials,
                                                 texdesc=d.texdesc, texdata=d.texdata))
        elif k == "update": g.update_triangles(d.tris)
        elif k == "subset": g.update_triangles_subset(d.tris[:e[1]], np.arange(e[1], dtype=np.uint32))
        elif k == "resize": self.size(e[1], e[2])
        elif k == "partition": g.set_partition(0, 1)
        elif k == "mk_reset": g.mk_reset()
        elif k == "adaptive_clear": g.mk_adaptive_clear()
        elif k == "adaptive_update": g.mk_adaptive_update()
        elif k == "active_write": g.mk_active_write(np.arange(e[1], dtype=np.uint32))
        elif k == "denoise": g.denoise()
        else: raise ValueError(e)

    def flags(self):
        """(T0, T1, O0, O1, H, L), D, moved.  H last, it changes the state: with the option off and both slots written, flx_reproject is
        refused for the want of a history, or for a posed object (moved), or runs"""
        g = self.g
        T = [int(not _refuses(lambda: g.gbuffer_read(s), "the slot holds no G-buffer")) for s in (0, 1)]
        O = [int(not _refuses(lambda: g.gbuffer_objects_read(s), "no object plane")) for s in (0, 1)]
        L = int(not _refuses(g.mk_active_read, "no list of active pixels"))
        D = int(not _refuses(lambda: g.read_pixels(6), "which = 6"))
        g.set_option("motion_history", 0)
        for s in (0, 1):
            g.gbuffer_write(s, self.blank, self.p["camera"])
        why = _refusal(g.reproject)
        g.finish()
        H, moved = int("no captured history" not in why), int("objects were posed since the capture" in why)
        assert not why or (not H) != moved, why
        return (T[0], T[1], O[0], O[1], H, L), D, moved


@pytest.mark.parametrize("case", fs.CASES, ids=[c["name"] for c in fs.CASES])
def test_sequence(scene, case):
    r = Run(scene)
    try:
        for e in case["events"]:
            r.event(e)
        got, D, moved = r.flags()
    finally:
        r.g.close()
    print(case["name"], got, D, moved)
    assert got == case["expect"]
    if "D" in case:
        assert D == case["D"]
    if "moved" in case:
        assert got[4] == 1 and moved == case["moved"]
