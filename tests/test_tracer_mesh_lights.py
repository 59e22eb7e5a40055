"""Tracer::setMeshLights / meshLightCount: while emissive triangles light the scene the Tracer stays on the microkernel
integrator -- the only one that sees them -- and refuses to leave it.  The Tracer owns a device context, so these need a GPU."""
import numpy as np
import pytest
import mesh_light_reference as MR
from fluctus_amd import host

pytestmark = pytest.mark.gpu

MTL = "newmtl wall\nKd 0.6 0.6 0.6\nnewmtl lamp_a\nKd 0 0 0\nKe 20 18 15\nnewmtl lamp_b\nKd 0 0 0\nKe 0 5 9\n"
# a floor, a lamp of two triangles 1.5 above it facing down, a second one of a single triangle
OBJ = ("mtllib room.mtl\n"
       "v -2 0 -2\nv 2 0 -2\nv 2 0 2\nv -2 0 2\n"
       "v -0.5 1.5 -0.5\nv 0.5 1.5 -0.5\nv 0.5 1.5 0.5\nv -0.5 1.5 0.5\n"
       "v 1 1 0\nv 1.5 1 0\nv 1 1 0.5\n"
       "usemtl wall\nf 1 3 2\nf 1 4 3\n"
       "usemtl lamp_a\nf 5 6 7\nf 5 7 8\n"
       "usemtl lamp_b\nf 9 10 11\n")


def test_tracer_mesh_lights(tmp_path):
    from fluctus_amd.tracer import Tracer
    (tmp_path / "room.mtl").write_text(MTL)
    (tmp_path / "room.obj").write_text(OBJ)
    path = str(tmp_path / "room.obj")
    w, h = 48, 32
    t = Tracer(w, h, 0, w * h)
    t.init(w, h, path)
    assert t.uses_wavefront
    with pytest.raises(RuntimeError, match="mesh_lights"):
        t.mesh_light_count()
    for _ in range(3):
        t.update()
    t.set_mesh_lights(True)
    assert not t.uses_wavefront, "update() takes its microkernel branch while mesh lights are on"
    assert t.mesh_light_count() == MR.lights(host.load_scene(path)).size == 3
    with pytest.raises(RuntimeError, match="mesh lights"):
        t.toggle_renderer()
    assert not t.uses_wavefront
    p = t.params
    p["useAreaLight"], p["useEnvMap"] = 0, 0
    t.params = p
    for _ in range(6):
        t.update()
    assert not t.uses_wavefront
    lit = t.read_pixels(0)
    assert np.isfinite(lit).all() and lit[:, :3].sum() > 0, "the lamps light the floor"
    t.set_mesh_lights(False)
    t.toggle_renderer()
    assert t.uses_wavefront
