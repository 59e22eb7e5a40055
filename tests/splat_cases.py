"""Inputs and drivers shared by tests/test_gpu_splat.py (device vs oracle) and tests/test_splat_inputs.py (the oracle against itself, CPU).

The fused logic pass adds a terminating path's pixel -- and, with the options on, its luminance moments and the two denoiser features -- through
flx_splat.h's wave_add4: four adjacent lanes carry the four words of one path's record.  The cases here put the wave shapes that matter in front of
it: every lane terminating (four rounds, a partial last wave), none, a mix, the `first` launch bounded by the pixel count, and the regrouped instance."""
import numpy as np
import common
from common import COL, Q
from fluctus_amd import host, wire, driver


def _params(d, w, h, pos, target, **kw):
    p = wire.default_params(w, h, d.world_radius, d.tris.size)
    wire.look_at(p, pos, target)
    p["wfSeparateQueues"], p["useAreaLight"], p["useEnvMap"] = 1, 0, 1
    for k, v in kw.items():
        p[k] = v
    return p


def sky_case(w, h):
    """simple_scene with the camera above it, looking up and away: every primary ray misses and takes the environment"""
    d = common.simple_scene()
    return d, _params(d, w, h, (0.0, 3.0, 0.0), (0.0, 10.0, -3.0), maxBounces=4), host.synthetic_sky(64, 32)


def box_scene():
    """a closed, diffuse box [-6, 6]^3 seen from inside: no ray leaves it"""
    c = np.array([[x, y, z] for x in (-6.0, 6.0) for y in (-6.0, 6.0) for z in (-6.0, 6.0)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.zeros(12, wire.TRIANGLE)
    for q, (a, b, cc, dd) in enumerate(quads):
        n = -np.sign(c[a] + c[b] + c[cc] + c[dd])                  # inward
        for k, idx in enumerate(((a, b, cc), (a, cc, dd))):
            t = tris[2 * q + k]
            for v, i in zip(("v0", "v1", "v2"), idx):
                t[v]["p"]["x"], t[v]["p"]["y"], t[v]["p"]["z"] = c[i]
                t[v]["n"]["x"], t[v]["n"]["y"], t[v]["n"]["z"] = n
            t["matId"] = 0
    d = host.SceneData()
    d.tris = tris
    d.materials = np.array([common.default_material()], wire.MATERIAL)
    d.texdesc = np.zeros(0, wire.TEXDESC); d.texdata = np.zeros(0, np.uint8)
    host.build_bvh(d, "sbvh")
    return d


def box_case(w, h):
    d = box_scene()
    return d, _params(d, w, h, (0.0, 1.6, 3.2), (0.0, 0.5, 0.0), maxBounces=6), host.synthetic_sky(64, 32)


def proc_case(kind, w, h, **kw):
    """the small procedural kitchen / conference room of the other GPU tests (3000 triangles), under a sky and its area light"""
    d = host.generate_scene(kind, 3000, 7 if kind == "kitchen" else 43)
    host.build_bvh(d, "binned")
    return d, _params(d, w, h, (0.0, 1.2, 2.6), (0.0, 0.2, 0.0), maxBounces=2, useAreaLight=1, **kw), host.synthetic_sky(64, 32)


def setup(c, d, p, env, denoiser=False, **options):
    if denoiser:
        c.set_option("denoiser", 1)
    for k, v in options.items():
        c.set_option(k, v)
    c.upload_scene(d); c.upload_envmap(env); c.set_params(p)
    driver.reset_renderer(c)
    return c


def lum(ei):
    """flx_denoise.h: flx_lum, in fp32 and in its order"""
    ei = ei.astype(np.float32)
    return (np.float32(0.2126) * ei[0] + np.float32(0.7152) * ei[1]) + np.float32(0.0722) * ei[2]


def oracle_iteration(o, npix, moments=None, first=False):
    """driver.benchmark_iteration's calls on the oracle, stopping after the extension launch (the caller compares hit records there).  `moments`
    ((npix, 4) float64, updated in place): what option "moments" accumulates, restated from the oracle's own state right after its logic step --
    (sum l, sum l^2, 0, n) over the paths logic terminated with pathLen > 0, at the pixel and with the radiance the path then holds."""
    o.wf_logic(first)
    cnt = np.array(o.get_counters(), copy=True)
    if moments is not None:
        st = o.state_export()
        ids = o.queue_read(Q.RAYGEN)[:int(cnt[Q.RAYGEN])]
        iu = st.view(np.uint32)
        ids = ids[iu[COL.PATH_LEN][ids] > 0]
        l = lum(st[20:23, ids])
        pix = iu[COL.PIXEL_INDEX][ids]
        np.add.at(moments[:, 0], pix, l.astype(np.float64))
        np.add.at(moments[:, 1], pix, (l * l).astype(np.float64))
        np.add.at(moments[:, 3], pix, 1.0)
    o.wf_raygen(); o.wf_materials()
    cnt = np.array(o.get_counters(), copy=True)
    o.wf_extend()
    return cnt


def lockstep_free_run(g, o, npix, iterations, moments=None):
    """Whole iterations of the device's default path (fused logic + material pass on RAW hit records) beside the oracle, tests/test_gpu_wide.py's way:
    counters after every logic / genRays / material step, and should the 4-wide closest hit have resolved an exact tie the other way, the device
    continues from the oracle's hit records so that one flip cannot fork the runs.  Returns the counters of every iteration."""
    out = []
    for it in range(iterations):
        g.wf_logic(False); g.wf_raygen(); g.wf_materials()
        cg = g.get_counters()
        g.wf_extend(); g.finish()
        cg = np.array(cg, copy=True)
        co = oracle_iteration(o, npix, moments)
        assert (cg == co).all(), f"iteration {it}: counters {cg} vs {co}"
        sg, so = g.state_export(), o.state_export()
        if (sg.view(np.uint32)[COL.HIT_I] != so.view(np.uint32)[COL.HIT_I]).any():
            g.state_import(so)
        for c in (g, o):
            c.wf_shadow(); c.clear_queues()
        g.finish()
        for c in (g, o):
            c.pixel_index_update(npix, int(co[Q.RAYGEN]))
        out.append(co)
    fails = common.state_diff(g.state_export(), o.state_export(), 0.0, 0.0)
    assert not fails, "; ".join(fails[:5])
    return out
