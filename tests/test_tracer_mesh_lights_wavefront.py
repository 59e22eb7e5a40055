"""Tracer::setMeshLightsWavefront: with it the Tracer may take its wavefront loop while emissive triangles light the scene.
On the small room of tests/test_tracer_mesh_lights.py.  The Tracer owns a device context, so these need a GPU."""
import numpy as np
import pytest
import mesh_light_reference as MR

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


def test_tracer_mesh_lights_wavefront(tmp_path):
    from fluctus_amd.tracer import Tracer
    (tmp_path / "room.mtl").write_text(MTL)
    (tmp_path / "room.obj").write_text(OBJ)
    path = str(tmp_path / "room.obj")
    w, h = 48, 32
    t = Tracer(w, h, 0, w * h)
    t.init(w, h, path)
    t.set_option("moments", 1)                                  # the luminance moments: the standard errors below
    p = t.params
    p["useAreaLight"], p["useEnvMap"] = 0, 0
    t.params = p
    with pytest.raises(RuntimeError, match="setMeshLights"):
        t.set_mesh_lights_wavefront(True)
    assert not t.mesh_lights_wavefront
    t.set_mesh_lights(True)
    assert not t.uses_wavefront and not t.mesh_lights_wavefront, "setMeshLights(true) alone behaves as ever"
    with pytest.raises(RuntimeError, match="mesh lights"):
        t.toggle_renderer()
    for _ in range(24):
        t.update()
    assert not t.uses_wavefront
    ref = t.read_pixels(0), t.read_pixels(7)
    t.set_mesh_lights_wavefront(True)
    assert t.mesh_lights_wavefront and not t.uses_wavefront, "the integrator in use stays: toggle_renderer() switches"
    t.toggle_renderer()
    assert t.uses_wavefront
    for _ in range(6):
        t.update()
    assert t.uses_wavefront
    lit = t.read_pixels(0)
    assert np.isfinite(lit).all() and lit[:, :3].sum() > 0, "the lamps light the floor on the wavefront loop"
    for _ in range(90):
        t.update()
    got = t.read_pixels(0), t.read_pixels(7)
    t.set_mesh_lights_wavefront(True)                           # the same value again: nothing changes, the accumulation stays
    assert t.uses_wavefront and np.array_equal(t.read_pixels(0), got[0])
    t.update()
    assert t.read_pixels(0)[:, 3].sum() > got[0][:, 3].sum(), "the accumulation went on, it did not restart"
    assert got[0][:, 3].min() >= 4 and ref[0][:, 3].min() >= 4
    z, ma, mb = MR.tile_z(ref, got, w, h)
    print(f"tracer, wavefront vs microkernel branch: largest |A - B| / SE {z.max():.2f} over {z.size} tiles; samples per pixel "
          f"{ref[0][:, 3].min():.0f} .. {ref[0][:, 3].max():.0f} against {got[0][:, 3].min():.0f} .. {got[0][:, 3].max():.0f}")
    assert ma.max() > 0 and (z <= 5.0).all(), f"tiles {np.argwhere(z > 5.0).tolist()} differ by {z[z > 5.0]} standard errors"
    # the way back
    t.toggle_renderer()
    assert not t.uses_wavefront
    t.toggle_renderer()
    assert t.uses_wavefront
    t.set_mesh_lights_wavefront(False)                          # switched off on the wavefront loop: back to the integrator that sees the lamps
    assert not t.uses_wavefront and not t.mesh_lights_wavefront
    with pytest.raises(RuntimeError, match="mesh lights"):
        t.toggle_renderer()
    t.set_mesh_lights_wavefront(True)
    t.toggle_renderer()
    assert t.uses_wavefront
    t.set_mesh_lights(False)
    assert not t.mesh_lights_wavefront, "setMeshLights(false) clears the flag"
    t.set_mesh_lights(True)
    assert not t.uses_wavefront
    with pytest.raises(RuntimeError, match="mesh lights"):
        t.toggle_renderer()
    t.close()
