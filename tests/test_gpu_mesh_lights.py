"""Emissive triangles as lights on the device (option "mesh_lights"): off is off, the device's table equals the host's byte
for byte wherever triangles move, the sampling hook against float64, and the renders -- against the parametric quad they can replace, and the
three sampling modes against each other -- by a 5-sigma test on tile means whose standard errors come from the luminance moments."""
import numpy as np
import pytest
import common
import mesh_light_cases as MC
import mesh_light_reference as MR
from common import COL
from fluctus_amd import driver, host, wire

pytestmark = pytest.mark.gpu
F = np.float32
VERTS = ("v0", "v1", "v2")
W, H, SPP = 48, 32, 256
MODES = [(1, 1), (1, 0), (0, 1)]                 # (sampleExpl, sampleImpl): MIS, next event estimation only, implicit hits only


def ctx(n, **options):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    for k, v in options.items():
        g.set_option(k, v)
    return g


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. off is off
@pytest.mark.parametrize("option,emissive", [(0, True), (1, False)])
def test_off_is_off(option, emissive):
    """option 0 on a scene WITH emissive materials, option 1 on a scene WITHOUT: one sample of the microkernel lockstep sequence stays
    bit-identical to the oracle, which knows nothing of Ke"""
    from oracle.binding import OracleContext
    d = common.mixed_material_scene()
    if emissive:
        for m in (1, 3, 4):
            d.materials[m]["Ke"]["x"], d.materials[m]["Ke"]["y"], d.materials[m]["Ke"]["z"] = 3.0, 2.0, 1.0
    w, h = 64, 48
    n = w * h + 100
    p = common.scene_params(d, w, h, maxBounces=4, useAreaLight=1, useEnvMap=1, envMapStrength=1.5)
    g, o = ctx(n, mesh_lights=option), OracleContext(n, threads=8)
    env = host.synthetic_sky(64, 32)
    for c in (g, o):
        c.upload_scene(d); c.upload_envmap(env); c.set_params(p); c.mk_reset()
    assert g.get_option("mesh_lights") == option
    steps = [("raygen", lambda c: c.mk_raygen())] + [(k, f) for _ in range(5) for k, f in (("next_vertex", lambda c: c.mk_next_vertex()),
                                                                                        ("sample_bsdf", lambda c: c.mk_sample_bsdf()))]
    for name, fn in steps + [("splat", lambda c: c.mk_splat())]:
        g.state_import(o.state_export())
        fn(g); fn(o)
        sa, sb = g.state_export(), o.state_export()
        fails = common.state_diff(sa, sb, 0.0, 0.0)
        assert not fails, f"{name}: " + "; ".join(fails[:4])
        assert np.array_equal(sa.view(np.uint32)[COL.PHASE], sb.view(np.uint32)[COL.PHASE])
    assert np.array_equal(bits(g.read_pixels(0)), bits(o.read_pixels(0)))
    assert np.array_equal(g.mk_stats(), o.mk_stats())
    if option:
        assert g.mesh_lights_read()[0].size == 0


# ---- 2. the table on the device is the table on the host
def same_table(g, d, what):
    dev, ref = g.mesh_lights_read(), host.mesh_light_table(d)
    assert dev[0].size == ref[0].size > MC.SCAN_BLOCK, what
    for name, a, b in zip(("tris", "cdf", "pick"), dev, ref):
        assert a.tobytes() == b.tobytes(), f"{what}: {name} differs"
    assert np.float64(dev[3]).tobytes() == np.float64(ref[3]).tobytes(), f"{what}: total {dev[3]!r} vs {ref[3]!r}"
    return dev


def scaled(tris, s, about=(0.0, 0.0, 0.0)):
    out = tris.copy()
    for v in VERTS:
        for k, c in zip("xyz", about):
            out[v]["p"][k] = (F(c) + F(s) * (tris[v]["p"][k] - F(c))).astype(F)
    return out


def test_device_table_equals_host_table_wherever_triangles_move():
    d, obj, lamps = MC.lamp_field()
    g = ctx(4096, mesh_lights=1)
    g.upload_scene(d)
    t0 = same_table(g, d, "after upload")
    assert np.array_equal(t0[0], lamps)
    # every triangle scaled by 2: all weights x 4, the same cdf up to rounding, another total
    d.tris = scaled(d.tris, 2.0)
    g.update_triangles(d.tris)
    t1 = same_table(g, d, "after flx_update_triangles")
    assert t1[3] > 3.9 * t0[3]
    # one lamp, just behind the seam between two runs of the prefix sums, grows ninefold
    k = MC.SCAN_BLOCK + 1
    i = int(lamps[k])
    c = [float(d.tris[i]["v0"]["p"][a]) for a in "xyz"]
    d.tris[i:i + 1] = scaled(d.tris[i:i + 1], 3.0, about=c)
    g.update_triangles_subset(d.tris[i:i + 1], [i])
    t2 = same_table(g, d, "after flx_update_triangles_subset")
    assert t2[2][k] > 2.0 * t1[2][k] and t2[1][0] < t1[1][0]
    # the lamps of one object scaled through their transform
    g.objects_define(d.tris, obj, 4)
    X = np.array([[1.5, 0, 0, 0.1], [0, 2.0, 0, -0.2], [0, 0, 0.5, 0.0]], F)
    members = np.nonzero(obj == 1)[0]
    g.objects_pose([1], X)
    d.tris[members] = host.pose_triangles(d.tris[members], X)
    t3 = same_table(g, d, "after flx_objects_pose")
    assert t3[1].tobytes() != t2[1].tobytes()
    # and built again from the same inputs: the same bytes
    g.set_option("mesh_lights", 0); g.set_option("mesh_lights", 1)
    same_table(g, d, "after switching the option off and on")


# ---- 3. the sampling hook
def test_sampling_probe_against_float64():
    d, _, lamps = MC.lamp_field()
    g = ctx(4096, mesh_lights=1)
    g.upload_scene(d)
    tris, cdf, pick, _ = g.mesh_lights_read()
    n = 4096
    r0 = np.random.RandomState(9).random_sample(n).astype(F)
    edge = np.concatenate([[F(0.0), F(1.0), np.nextafter(F(1.0), F(0.0))], cdf[:64], np.nextafter(cdf[:64], F(-1.0))]).astype(F)
    r0[:edge.size] = np.clip(edge, 0.0, 1.0)
    r3 = np.concatenate([r0[:, None], MR.edge_randoms(n, 10)], 1)
    light, out8 = g.mesh_lights_sample(r3)
    assert np.array_equal(light, MR.pick(cdf, pick, r3[:, 0])), "the light index is exact"
    P = MR.positions(d.tris[tris[light]])
    ref, _ = MR.sample64(P, r3[:, 1], r3[:, 2])
    bound = 8.0 * 2.0 ** -24 * np.abs(P).max((1, 2))
    err = np.abs(out8[:, :3] - ref) / bound[:, None]
    print(f"P: largest error {err.max():.3f} of the bound")
    assert (err <= 1.0).all()
    _, area64 = MR.weights64(d, tris)
    pdf_ref = (pick[light].astype(np.float64) / area64[light]).astype(F)
    ulps = MR.ulp_diff(out8[:, 3], pdf_ref)
    print(f"pdfA: largest distance {ulps.max()} ulp")
    assert ulps.max() <= 4
    # the CPU side runs the same functions: bit for bit
    hl, h8, _ = host.mesh_light_sample(d, r3)
    assert np.array_equal(hl, light) and np.array_equal(bits(h8), bits(out8))


# ---- 4. / 5. renders
def render(d, p, mesh, prepare=None, spp=SPP):
    g = ctx(int(p["width"]) * int(p["height"]), moments=1, mesh_lights=int(mesh))
    g.upload_scene(d)
    if prepare is not None:
        prepare(g)
    driver.render_single(g, p, spp)
    px, mom = g.read_pixels(0), g.read_pixels(7)
    assert (px[:, 3] == spp).all() and np.isfinite(px).all()
    return px, mom


def compare(a, b, what):
    """|A - B| <= 5 SE on every 8 x 8 tile; SE^2 = sum of the two tile means' variances, from the moments"""
    z, ma, mb = MR.tile_z(a, b, W, H)
    print(f"{what}: largest |A - B| / SE {z.max():.2f} over {z.size} tiles; tile means {ma.min():.4f} .. {ma.max():.4f}, {(ma > 0).sum()} tiles lit")
    assert ma.max() > 0.05 and (ma > 0).sum() >= z.size // 2, "the scene must be lit"
    assert (z <= 5.0).all(), f"{what}: tiles {np.argwhere(z > 5.0).tolist()} differ by {z[z > 5.0]} standard errors"
    return float(z.max())


@pytest.mark.parametrize("expl,impl", MODES)
def test_two_emissive_triangles_equal_the_quad(expl, impl):
    """render A: the parametric quad, option off.  Render B: no quad, two black triangles with Ke = E covering it exactly, option on."""
    da, db = MC.quad_scene(False), MC.quad_scene(True)
    a = render(da, MC.render_params(da, W, H, (expl, impl), useAreaLight=1), mesh=False)
    b = render(db, MC.render_params(db, W, H, (expl, impl), useAreaLight=0), mesh=True)
    compare(a, b, f"quad vs triangles, sampleExpl {expl} sampleImpl {impl}")


@pytest.fixture(scope="module")
def lamps_scene():
    return MC.three_lamps_scene()


@pytest.fixture(scope="module")
def lamps_truth(lamps_scene):
    """implicit hits only: reads no table, no pick and no pdfA -- the independent truth"""
    return render_lamps(lamps_scene, (0, 1))


def render_lamps(lamps_scene, mode, **kw):
    d, obj = lamps_scene

    def prepare(g):
        g.objects_define(d.tris, obj, 1)
        g.objects_pose([0], MC.LAMP_POSE)                    # after the upload: the render depends on the rebuilt table
    return render(d, MC.render_params(d, W, H, mode), mesh=True, prepare=prepare, **kw)


@pytest.mark.parametrize("expl,impl", [(1, 0), (1, 1)])
def test_sampling_modes_agree(lamps_scene, lamps_truth, expl, impl):
    compare(lamps_truth, render_lamps(lamps_scene, (expl, impl)), f"implicit only vs sampleExpl {expl} sampleImpl {impl}")


# ---- 6. adaptive
def test_adaptive_equals_uniform_at_each_pixels_count(lamps_scene):
    d, obj = lamps_scene
    w, h, LO, HI = 32, 24, 4, 16
    N = w * h
    p = MC.render_params(d, w, h, (1, 1))

    def fresh():
        g = ctx(N, moments=1, mesh_lights=1)
        g.upload_scene(d)
        g.objects_define(d.tris, obj, 1); g.objects_pose([0], MC.LAMP_POSE)
        g.set_params(p)
        return g
    g = fresh()
    g.mk_reset()
    uni = np.zeros((2, HI + 1, N, 4), F)
    for s in range(1, HI + 1):
        driver.render_single_pass(g, p["maxBounces"])
        uni[0, s], uni[1, s] = g.read_pixels(0), g.read_pixels(7)
    g = fresh()
    _, total = driver.render_adaptive(g, p, LO, HI)
    px = g.read_pixels(0)
    n = px[:, 3].astype(np.int64)
    assert n.min() >= LO and n.max() <= HI and total == n.sum()
    assert len(np.unique(n)) >= 2, "the scene must produce distinct counts"
    ar = np.arange(N)
    assert np.array_equal(bits(px), bits(uni[0][n, ar])) and np.array_equal(bits(g.read_pixels(7)), bits(uni[1][n, ar]))
    print(f"adaptive: {total} samples, counts {np.unique(n).tolist()}")


# ---- 7. ABI edges
def test_abi_edges():
    d, _, lamps = MC.lamp_field(8, seed=6)
    g = ctx(1024)
    g.upload_scene(d)
    for call in (g.mesh_lights_read, lambda: g.mesh_lights_sample(np.zeros((1, 3), F))):
        with pytest.raises(RuntimeError, match="mesh_lights"):
            call()
    with pytest.raises(RuntimeError):
        g.set_option("mesh_lights", 2)
    g.set_option("mesh_lights", 1)
    assert g.get_option("mesh_lights") == 1 and np.array_equal(g.mesh_lights_read()[0], lamps)
    # the option survives an upload, and the table then belongs to the new scene
    d2, _, lamps2 = MC.lamp_field(5, seed=7)
    g.upload_scene(d2)
    assert g.get_option("mesh_lights") == 1
    dev, ref = g.mesh_lights_read(), host.mesh_light_table(d2)
    assert np.array_equal(dev[0], lamps2) and dev[1].tobytes() == ref[1].tobytes() and dev[3] == ref[3]
    # a scene without a light: an empty table, and nothing to sample
    g.upload_scene(common.simple_scene())
    assert g.mesh_lights_read()[0].size == 0 and g.mesh_lights_read()[3] == 0.0
    with pytest.raises(RuntimeError, match="no light"):
        g.mesh_lights_sample(np.zeros((1, 3), F))
    g.set_option("mesh_lights", 0)
    with pytest.raises(RuntimeError, match="mesh_lights"):
        g.mesh_lights_read()
