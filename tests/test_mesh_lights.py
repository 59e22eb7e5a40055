"""Emissive triangles as lights without a GPU: the shared header csrc/flx_mesh_light.h, run through libfluctus_host.so
(host_capi.cpp: fh_mesh_light_*), against the numpy restatement tests/mesh_light_reference.py; and the two loaders that bring Ke."""
import os
import numpy as np
import pytest
import mesh_light_cases as MC
import mesh_light_reference as MR
from fluctus_amd import host

F = np.float32
BELOW1 = np.nextafter(F(1.0), F(0.0))


@pytest.fixture(scope="module")
def tab():
    d = MC.table_scene()
    return d, host.mesh_light_table(d)


def test_table_against_float64(tab):
    d, (tris, cdf, pick, total) = tab
    idx, cdf_ref, total_ref = MR.table(d)
    assert 38 <= tris.size <= 48 and np.array_equal(tris, idx), "the list is every triangle whose material emits, ascending"
    w32, area32 = MR.weights32(d, idx)
    live = w32[w32 > 0]
    assert live.max() / live.min() >= 1e6, "the scene's weights must span six orders of magnitude"
    assert (w32 == 0).sum() == 1 and (area32 == 0).sum() == 1, "one zero-area light"
    assert (d.materials["Ke"]["x"][d.tris["matId"]] == 0).sum() > tris.size // 4        # Ke = 0 triangles in between (matId 0 and 3)
    # the fp32 weight against float64: area and luminance are well conditioned here (random, not thin, triangles)
    w64, _ = MR.weights64(d, idx)
    assert np.allclose(w32[w32 > 0], w64[w32 > 0], rtol=1e-5, atol=0.0)
    assert abs(total - total_ref) <= 1e-15 * total_ref
    assert MR.ulp_diff(cdf, cdf_ref).max() <= 1, "cdf within 1 ulp of the rounded float64 value"
    assert np.array_equal(pick.view(np.uint32), (cdf - np.concatenate([[F(0)], cdf[:-1]]).astype(F)).view(np.uint32)), "pick = cdf[k] - cdf[k - 1] in fp32"
    assert (np.diff(cdf) >= 0).all() and (pick >= 0).all()
    last_live = np.nonzero(w32 > 0)[0][-1]
    assert cdf[last_live] == 1.0 and (cdf[last_live:] == 1.0).all()
    zero_pick = np.nonzero((pick == 0) & (w32 > 0))[0]
    assert zero_pick.size >= 1, "the scene must hold a light too small for its pick to survive the rounding"
    assert pick[np.nonzero(area32 == 0)[0][0]] == 0


def test_table_is_deterministic_and_crosses_a_run_seam():
    d, _, lamps = MC.lamp_field()
    a, b = host.mesh_light_table(d), host.mesh_light_table(d)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3] == b[3]
    assert np.array_equal(a[0], lamps) and lamps.size == MC.SCAN_BLOCK + 3
    _, cdf_ref, total_ref = MR.table(d)
    assert MR.ulp_diff(a[1], cdf_ref).max() <= 1 and abs(a[3] - total_ref) <= 1e-15 * total_ref


@pytest.mark.parametrize("make", [MC.no_lamp_scene, MC.degenerate_lamps_scene])
def test_no_lights(make):
    tris, cdf, pick, total = host.mesh_light_table(make())
    assert tris.size == cdf.size == pick.size == 0 and total == 0.0


def test_pick(tab):
    _, (tris, cdf, pick, _) = tab
    r = np.concatenate([[F(0.0), F(1.0), BELOW1], cdf, np.nextafter(cdf, F(-1.0)), np.nextafter(cdf, F(2.0))]).astype(F)
    r = r[(r >= 0) & (r <= 1)]
    k = host.mesh_light_pick(cdf, pick, r)
    assert np.array_equal(k, MR.pick(cdf, pick, r)), "ml_pick is searchsorted(cdf, r, 'right'), clamped to the last light with pick > 0"
    assert (pick[k] > 0).all(), "a light with pick = 0 is never returned"
    assert k[1] == np.nonzero(pick > 0)[0][-1], "r = 1.0f takes the clamp"
    # every light that can be picked is picked by some r below its cdf
    assert set(k.tolist()) == set(np.nonzero(pick > 0)[0].tolist())


def test_sample_triangle(tab):
    d, (tris, cdf, pick, _) = tab
    n = 4096
    r12 = MR.edge_randoms(n, 7)
    r3 = np.concatenate([np.random.RandomState(8).random_sample((n, 1)).astype(F), r12], 1)
    light, out8, bary = host.mesh_light_sample(d, r3)
    assert np.array_equal(light, MR.pick(cdf, pick, r3[:, 0]))
    P = MR.positions(d.tris[tris[light]])
    ref, bref = MR.sample64(P, r3[:, 1], r3[:, 2])
    bound = 8.0 * 2.0 ** -24 * np.abs(P).max((1, 2))
    assert (np.abs(out8[:, :3] - ref) <= bound[:, None]).all(), "P within 8 * 2^-24 * max |p_i| per component"
    assert (bary >= 0).all() and (bary <= 1).all() and np.abs(bary.astype(np.float64).sum(1) - 1.0).max() <= 3 * 2.0 ** -24, "inside the triangle"
    assert np.abs(bary - bref).max() <= 3 * 2.0 ** -24
    _, area32 = MR.weights32(d, tris)
    assert np.array_equal(out8[:, 7], area32[light]) and np.array_equal(out8[:, 3], pick[light] / area32[light])
    n_g = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]); n_g /= np.linalg.norm(n_g, axis=1, keepdims=True)
    assert np.abs(out8[:, 4:7] - n_g).max() <= 2e-4        # (a 1e-3 triangle's fp32 cross product cancels to ~1e-4 relative)


def test_find(tab):
    d, (tris, _, _, _) = tab
    assert np.array_equal(host.mesh_light_find(tris, tris), np.arange(tris.size))
    near = np.setdiff1d(np.concatenate([tris.astype(np.int64) - 1, tris.astype(np.int64) + 1, [0, d.tris.size - 1, d.tris.size + 5]]), tris)
    near = near[near >= 0].astype(np.uint32)
    assert near.size > tris.size // 2
    assert (host.mesh_light_find(tris, near) == MR.NONE).all()
    assert (host.mesh_light_find(tris[:0], near) == MR.NONE).all()


# ---- the loaders
def test_obj_ke_gives_an_emissive_material(tmp_path):
    (tmp_path / "l.mtl").write_text("newmtl wall\nKd 0.5 0.5 0.5\nnewmtl lamp\nKd 0 0 0\nKe 4 3 2\n")
    (tmp_path / "l.obj").write_text("mtllib l.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nusemtl wall\nf 1 2 3\nusemtl lamp\nf 1 2 4\nf 2 3 4\n")
    d = host.load_scene(str(tmp_path / "l.obj"))
    ke = MR.ke_of(d)
    assert ke.shape[0] == 3 and (ke[0] == 0).all() and np.allclose(ke[1:], [4, 3, 2])
    tris, _, pick, total = host.mesh_light_table(d)
    assert np.array_equal(tris, [1, 2]) and total > 0 and abs(float(pick.sum()) - 1.0) < 1e-6


PBRT = """
LookAt 0 1 3  0 0 0  0 1 0
Camera "perspective" "float fov" [50]
WorldBegin
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "point P" [0 0 0  1 0 0  0 0 1] "integer indices" [0 1 2]
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [4 3 2] "float scale" [2.5] "bool twosided" "true"
  Shape "trianglemesh" "point P" [0 2 0  1 2 0  0 2 1  1 2 1] "integer indices" [0 1 2  1 3 2]
  AttributeBegin
    Material "plastic" "rgb Kd" [0.1 0.2 0.3]
    Shape "trianglemesh" "point P" [0 3 0  1 3 0  0 3 1] "integer indices" [0 1 2]
  AttributeEnd
AttributeEnd
Shape "trianglemesh" "point P" [0 1 0  1 1 0  0 1 1] "integer indices" [0 1 2]
WorldEnd
"""


def test_pbrt_area_light_source_is_attribute_state(tmp_path):
    (tmp_path / "s.pbrt").write_text(PBRT)
    d = host.load_scene(str(tmp_path / "s.pbrt"))
    ke = MR.ke_of(d)
    assert ke.shape[0] == 5
    assert (ke[0] == 0).all() and (ke[4] == 0).all(), "shapes before AttributeBegin and after AttributeEnd do not emit"
    assert np.allclose(ke[1:4], [10.0, 7.5, 5.0]), "Ke = L * scale on every shape inside, the nested attribute block included"
    m = d.materials[d.tris["matId"]]
    assert m["type"][1] == m["type"][0] and np.allclose(m["Kd"]["x"][[0, 1, 4]], 0.5), "the lamp keeps its material's BSDF; the material itself is not touched"
    assert d.tris["matId"][1] == d.tris["matId"][2] != d.tris["matId"][0] == d.tris["matId"][4]
    assert np.isclose(m["Kd"]["z"][3], 0.3) and d.tris["matId"][3] != d.tris["matId"][1]
    assert np.array_equal(host.mesh_light_table(d)[0], [1, 2, 3])
