"""Scenes of tests/test_mesh_lights.py (CPU) and tests/test_gpu_mesh_lights.py: emissive triangles as lights.
Everything is built in numpy in wire format with the helpers of tests/common.py; the ones that are rendered get an SBVH."""
import numpy as np
import common
from fluctus_amd import host, wire
from fluctus_amd.wire import BXDF

F = np.float32
NO_OBJECT = 0xFFFFFFFF
SCAN_BLOCK = 256                                 # ML_SCAN_BLOCK of csrc/flx_mesh_light.h: the lights of one run of the prefix sums


def tri(p0, p1, p2, m):
    """one wire triangle with its geometric normal (p1 - p0) x (p2 - p0) at the three vertices ((0, 1, 0) when it has none)"""
    t = np.zeros((), wire.TRIANGLE)
    p = np.asarray([p0, p1, p2], np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    ln = np.linalg.norm(n)
    n = n / ln if ln > 0 else np.array([0.0, 1.0, 0.0])
    for v, q in zip(("v0", "v1", "v2"), p):
        t[v]["p"]["x"], t[v]["p"]["y"], t[v]["p"]["z"] = q
        t[v]["n"]["x"], t[v]["n"]["y"], t[v]["n"]["z"] = n
    t["matId"] = m
    return t


def quad(c, right, up, sx, sy, m, normal):
    """two triangles covering c +- sx right +- sy up whose geometric normal is `normal` (the corner order is turned round when it is not)"""
    c, r, u = (np.asarray(v, np.float64) for v in (c, right, up))
    a, b, cc, d = c + sx * r + sy * u, c - sx * r + sy * u, c - sx * r - sy * u, c + sx * r - sy * u
    if np.dot(np.cross(b - a, cc - a), normal) < 0:
        a, b, cc, d = a, d, cc, b
    return [tri(a, b, cc, m), tri(a, cc, d, m)]


def box(c, h, m):
    """twelve triangles, normals outwards"""
    c, h = np.asarray(c, np.float64), np.asarray(h, np.float64)
    out = []
    for ax in range(3):
        for s in (-1.0, 1.0):
            n = np.zeros(3); n[ax] = s
            r = np.zeros(3); r[(ax + 1) % 3] = 1.0
            u = np.zeros(3); u[(ax + 2) % 3] = 1.0
            out += quad(c + n * h[ax], r, u, h[(ax + 1) % 3], h[(ax + 2) % 3], m, n)
    return out


def emissive(ke, kd=(0.0, 0.0, 0.0)):
    m = common.make_material(BXDF.DIFFUSE, kd=kd, ks=(0.0, 0.0, 0.0))
    m["Ke"]["x"], m["Ke"]["y"], m["Ke"]["z"] = ke
    return m


def scene(tris, mats, bvh=True):
    d = host.SceneData()
    d.tris = np.array(tris, wire.TRIANGLE)
    d.materials = np.array(mats, wire.MATERIAL)
    d.texdesc = np.zeros(0, wire.TEXDESC)
    d.texdata = np.zeros(0, np.uint8)
    if bvh:
        host.build_bvh(d, "sbvh")
    return d


def _random_tri(rng, size, m, lo=(-2.0, 0.5, -2.0), hi=(2.0, 2.5, 2.0), right_angle=False):
    c = rng.uniform(lo, hi)
    e = rng.normal(size=(2, 3))
    if right_angle:
        e[1] -= e[0] * np.dot(e[0], e[1]) / np.dot(e[0], e[0])
    e = size * e / np.linalg.norm(e, axis=1, keepdims=True)
    return tri(c, c + e[0], c + e[1], m)


TABLE_MATS = [common.default_material(), emissive((5.0, 4.0, 3.0)), emissive((0.0, 0.5, 0.0)), emissive((0.0, 0.0, 0.0), kd=(0.5, 0.5, 0.5)),
              emissive((2e-3, 1e-3, 1e-3))]


def table_scene():
    """about 40 lights between triangles that are none: edge lengths over three decades (areas over six, the weights further by Ke), a zero-area
    emissive triangle, triangles of a material whose Ke is 0, and -- third from the end, where the cdf is near 1 and its ulp 6e-8 -- a light of
    relative weight ~1e-11, whose pick rounds to 0.  No hierarchy: the table needs triangles and materials only."""
    rng = np.random.RandomState(11)
    tris, n = [], 0
    while n < 38:
        tris.append(_random_tri(rng, 0.5, 0))
        if rng.rand() < 0.3:
            tris.append(_random_tri(rng, 0.5, 3))                       # Ke = 0: no light
        tris.append(_random_tri(rng, 10.0 ** rng.uniform(-3.0, 0.0), 1 + int(rng.randint(0, 2)) if n % 5 else 4))
        n += 1
        if n == 17:
            p = rng.uniform(-1, 1, 3)
            tris.append(tri(p, p, p + 0.3, 1))                          # zero area, emissive material: listed, weight 0
    tris.append(_random_tri(rng, 1e-5, 1))                              # pick rounds to 0
    tris.append(_random_tri(rng, 0.2, 2))
    tris.append(_random_tri(rng, 0.4, 1))
    tris.append(_random_tri(rng, 0.5, 0))
    return scene(tris, TABLE_MATS, bvh=False)


def no_lamp_scene():
    rng = np.random.RandomState(3)
    return scene([_random_tri(rng, 0.5, m) for m in (0, 3, 0, 3)], TABLE_MATS, bvh=False)


def degenerate_lamps_scene():
    """emissive materials on zero-area triangles only"""
    rng = np.random.RandomState(4)
    tris = [_random_tri(rng, 0.5, 0) for _ in range(3)]
    for m in (1, 2):
        p = rng.uniform(-1, 1, 3)
        tris += [tri(p, p, p + 0.5, m), tri(p, p + 0.25, p, m)]
    return scene(tris, TABLE_MATS, bvh=False)


FLOOR = quad((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 2.0, 2.0, 0, (0.0, 1.0, 0.0))


# the materials of lamp_field(steps=...): TABLE_MATS, two more emitters and a receiver of every BSDF type but the floor's
STEP_DIM, STEP_DOMINANT, STEP_GLOSSY, STEP_GGX_REFL, STEP_GGX_REFR, STEP_MIRROR, STEP_DIELECTRIC = range(5, 12)
STEP_MATS = TABLE_MATS + [emissive((1e-6, 1e-6, 1e-6)), emissive((40.0, 50.0, 30.0)),
                          common.make_material(BXDF.GLOSSY, kd=(0.2, 0.5, 0.7), ks=(0.3, 0.3, 0.3), ns=300.0, ni=1.5),
                          common.make_material(BXDF.GGX_ROUGH_REFLECTION, ks=(0.9, 0.8, 0.5), ns=60.0, ni=1.5),
                          common.make_material(BXDF.GGX_ROUGH_DIELECTRIC, ks=(0.95, 0.9, 0.85), ns=40.0, ni=1.5),
                          common.make_material(BXDF.IDEAL_REFLECTION, ks=(0.9, 0.9, 0.9)),
                          common.make_material(BXDF.IDEAL_DIELECTRIC, ks=(0.9, 0.95, 1.0), ni=1.5)]
STEP_RECEIVER_MATS = (0, STEP_GLOSSY, STEP_GGX_REFL, STEP_GGX_REFR, STEP_MIRROR, STEP_DIELECTRIC)


def _step_extras(tris, obj, lamps, names):
    """the part of lamp_field that tests/mesh_light_step_cases.py aims at, beside the floor (x in 2.4 .. 6.2): six receiver quads at y = 0,
    one per BSDF type, under lamps that face down unless said otherwise.  `names` receives the triangle indices by name."""
    def add(name, new, lamp):
        names[name] = list(range(len(tris), len(tris) + len(new)))
        if lamp:
            lamps.extend(names[name])
        tris.extend(new); obj.extend([NO_OBJECT] * len(new))
    X, Z, DOWN, UP = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0)
    for j, m in enumerate(STEP_RECEIVER_MATS):
        add(f"receiver{j}", quad((2.75 + 0.6 * j, 0.0, 0.0), X, Z, 0.25, 0.6, m, UP), False)
    add("back", quad((2.8, 1.4, 0.1), X, Z, 0.2, 0.2, 1, UP), True)                  # shows the receivers its back
    add("half", quad((3.5, 1.5, 0.0), X, Z, 0.25, 0.25, 2, DOWN), True)               # half of it (x > 3.5) behind a plate that is no light
    add("half_plate", quad((3.8, 1.2, 0.0), X, Z, 0.3, 0.5, 0, DOWN), False)
    add("front", quad((4.3, 1.3, 0.0), X, Z, 0.15, 0.15, 1, DOWN), True)              # a lamp in front of a larger lamp
    add("behind", quad((4.3, 1.6, 0.0), X, Z, 0.3, 0.3, 2, DOWN), True)
    add("veiled", quad((5.0, 1.5, 0.0), X, Z, 0.2, 0.2, 1, DOWN), True)               # a plate 3 mm before it: past 0.995 |L| from the receivers
    add("veil", quad((5.0, 1.497, 0.0), X, Z, 0.4, 0.4, 0, DOWN), False)
    add("gains", [tri((5.4, 1.2, 0.3), (5.4, 1.2, -0.3), (5.9, 1.2, 0.0), 0)], False)  # gets an emissive matId after the upload: seen, never listed
    add("quad_lamp", quad((5.7, 1.7, 0.0), X, Z, 0.2, 0.2, 2, DOWN), True)            # the parametric quad is put before this one
    add("tiny", [tri((3.0, 1.8, 0.5), (3.05, 1.8, 0.5), (3.0, 1.8, 0.45), STEP_DIM)], True)             # pick rounds to 0 ...
    add("dominant", quad((3.1, 1.8, -0.1), X, Z, 0.5, 0.5, STEP_DOMINANT, DOWN), True)                   # ... beside the light that outweighs the field
    add("last", [tri((4.0, 1.9, 0.5), (4.05, 1.9, 0.5), (4.0, 1.9, 0.45), STEP_DIM)], True)             # the last light: cdf 1, pick 0
    for name in ("half", "front", "veiled", "quad_lamp", "dominant"):                 # shading normals that lean 30 degrees off n_g: a light's side,
        for i in names[name]:                                                         # cosine and pdf are the GEOMETRIC normal's business
            for v in ("v0", "v1", "v2"):
                tris[i][v]["n"]["x"], tris[i][v]["n"]["y"], tris[i][v]["n"]["z"] = 0.5, float(tris[i][v]["n"]["y"]) * np.sqrt(0.75), 0.0


def lamp_field(nlights=SCAN_BLOCK + 3, seed=5, steps=None):
    """a floor under `nlights` emissive triangles of four objects (lamp j belongs to object j % 4; the floor and the Ke = 0 triangles to none),
    sizes over two decades; one run of the prefix sums plus three lights by default, so that the seam between two runs is crossed.  The lamps
    are right-angled: their fp32 area is then within an ulp or two of the real one, which the sampling test's 4 ulp on pdfA presumes (a thin
    triangle's cross product cancels, and no fp32 area is close to the float64 one; tests/test_mesh_lights.py has those).
    steps (a dict, filled with name -> triangle indices): the same field with STEP_MATS and, behind it in the list, the arrangements of
    _step_extras -- the scene of the per-path tests of the integrator's two vertex steps.
    Returns (scene with hierarchy, object_of_triangle, lamp triangle indices)."""
    rng = np.random.RandomState(seed)
    tris, obj, lamps = list(FLOOR), [NO_OBJECT, NO_OBJECT], []
    for j in range(nlights):
        if j % 7 == 3:
            tris.append(_random_tri(rng, 0.2, 3)); obj.append(NO_OBJECT)
        lamps.append(len(tris))
        tris.append(_random_tri(rng, 10.0 ** rng.uniform(-2.0, -0.3), 1 + j % 2, right_angle=True)); obj.append(j % 4)
    if steps is not None:
        _step_extras(tris, obj, lamps, steps)
    return scene(tris, TABLE_MATS if steps is None else STEP_MATS), np.array(obj, np.uint32), np.array(lamps, np.uint32)


# ---- the rendered scenes: a floor, a box that shadows part of it, one diffuse and one glossy material, no singular one
QUAD_E = (20.0, 18.0, 15.0)
RENDER_MATS = [common.make_material(BXDF.DIFFUSE, kd=(0.6, 0.55, 0.5), ks=(0.0, 0.0, 0.0)),
               common.make_material(BXDF.GLOSSY, kd=(0.3, 0.4, 0.5), ks=(0.4, 0.4, 0.4), ns=60.0, ni=1.5)]
BOX = box((0.35, 0.25, 0.1), (0.35, 0.25, 0.3), 1)
QUAD = dict(pos=(-0.2, 1.6, 0.0), N=(0.0, -1.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), size=(0.5, 0.4))


def render_params(d, W, H, spp_modes, **kw):
    """the camera of the rendered scenes: above the floor's edge, looking down at the box; everything at y >= 1.3 is outside its view"""
    sample_expl, sample_impl = spp_modes
    p = wire.default_params(W, H, d.world_radius, d.tris.size)
    wire.look_at(p, (0.0, 1.0, 3.0), (0.0, 0.0, 0.0), fov=50.0)
    al = p["areaLight"]
    for k in ("pos", "N", "right", "up"):
        al[k]["x"], al[k]["y"], al[k]["z"] = QUAD[k]
    al["E"]["x"], al["E"]["y"], al["E"]["z"] = QUAD_E
    al["size"] = QUAD["size"]
    p["useEnvMap"], p["useAreaLight"], p["useRoulette"], p["maxBounces"] = 0, 0, 0, 3
    p["sampleExpl"], p["sampleImpl"] = sample_expl, sample_impl
    for k, v in kw.items():
        p[k] = v
    return p


def quad_scene(mesh):
    """render A (mesh False): floor and box, lit by the parametric quad (useAreaLight = 1).  Render B (mesh True): the same plus two black
    triangles with Ke = E that cover exactly the quad and face its way (useAreaLight = 0, option "mesh_lights")."""
    tris = list(FLOOR) + list(BOX)
    if mesh:
        tris += quad(QUAD["pos"], QUAD["right"], QUAD["up"], QUAD["size"][0], QUAD["size"][1], 2, QUAD["N"])
    return scene(tris, RENDER_MATS + [emissive(QUAD_E)])


LAMP_POSE = np.array([[1.5, 0.0, 0.0, 0.9], [0.0, 1.0, 0.0, 0.1], [0.0, 0.0, 1.5, -0.2]], F)       # object 0: scaled by 1.5 in x and z, moved


def three_lamps_scene(back_lamp=False):
    """floor and box under three lamps of different size and Ke: a large dim one overhead facing down, a small bright one low beside the box
    facing it (the box hides half of the floor from it), and a third that the test POSES after the upload (object 0, LAMP_POSE) -- the
    render depends on the rebuilt table.  back_lamp adds a fourth that shows the floor its BACK (used once, to see that the side test can fail
    the comparison: DESIGN.md 4.2.2).  Returns (scene, object_of_triangle)."""
    mats = RENDER_MATS + [emissive((6.0, 6.0, 5.0)), emissive((60.0, 40.0, 20.0)), emissive((10.0, 20.0, 30.0)), emissive((30.0, 30.0, 30.0))]
    tris = list(FLOOR) + list(BOX)
    obj = [NO_OBJECT] * len(tris)
    tris += quad((-0.6, 1.7, 0.2), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.7, 0.5, 2, (0.0, -1.0, 0.0)); obj += [NO_OBJECT] * 2
    tris += quad((1.3, 0.3, 0.1), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 0.2, 0.15, 3, (-1.0, 0.0, 0.0)); obj += [NO_OBJECT] * 2
    tris += quad((-1.0, 1.4, -0.6), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.2, 0.2, 4, (0.0, -1.0, 0.0)); obj += [0, 0]
    if back_lamp:
        tris += quad((0.0, 1.5, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.4, 0.4, 5, (0.0, 1.0, 0.0)); obj += [NO_OBJECT] * 2
    return scene(tris, mats), np.array(obj, np.uint32)
