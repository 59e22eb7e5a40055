"""GPU parity: libfluctus_hip.so (through the C ABI) vs the CPU oracle, BIT-EXACT.

Integers and floats alike must be identical: device and oracle share the arithmetic contract of
include/flx_math.h, compaction is stable, so the whole path state, every queue and every counter are
compared with == after every kernel (lockstep) and after free-running multi-iteration renders.
Tolerance: 0 ulp for path state; the framebuffer allows 1e-6 rel because several paths can splat the
same pixel within one iteration and fp32 atomic adds commute but do not associate.
"""
import numpy as np
import pytest
import common
from common import COL, Q
from fluctus_amd import host, wire, driver

pytestmark = pytest.mark.gpu


TRACE_MODE = {"ext": 2, "shadow": 4, "xcd": 0, "overlap": 2, "fuse": 1, "fuse_set": 0, "ext_order": -1}


# (extend_tree, shadow_tree, xcd_remap, overlap): every tree / stream schedule that claims bit-exactness must give the same bits.
# extend_tree is 2 throughout (the reference's visit order); the 4-wide closest-hit kernel is order-dependent in exact ties and
# has its own tests with a flip count (tests/test_gpu_wide.py).  shadow_tree 4 (the default) is exact by construction.
# fuse: logic + material kernels as one pass whenever flx_wf_materials follows flx_wf_logic with at most genRays between them (the
# default; api_wavefront.hip) vs always the separate kernels.
# fuse_set: the BSDF types that pass inlines -- 0 = what flx_upload_scene picked for the scene, 1 diffuse only (the rest through their
# queues), 31 all.
# ext_order: -1 = what the suite always used (1 with fuse_set 31, else 0 / the scene's), 2 = regenerated + continuing paths merged by path id.
MODES = [(2, 4, 0, 2, 1, 0, -1), (2, 2, 1, 1, 1, 31, -1), (2, 2, 0, 0, 0, 0, -1), (2, 4, 0, 0, 1, 1, -1), (2, 4, 0, 1, 0, 0, -1), (2, 4, 0, 2, 1, 31, 2),
         (2, 4, 0, 2, 1, 1, 2)]
MODE_KEYS = ("ext", "shadow", "xcd", "overlap", "fuse", "fuse_set", "ext_order")
DEFAULT_MODE = MODES[0]             # the product's defaults (with the bit-exact closest hit); id "wide-shadow"


def is_default_mode():
    """Derived from the fixture's own first parameter set, key by key -- round 4 compared TRACE_MODE against a hand-written dict, a key was
    added to one and not the other, and 21 full-size oracle tests skipped silently."""
    assert tuple(TRACE_MODE) == MODE_KEYS
    return tuple(TRACE_MODE[k] for k in MODE_KEYS) == DEFAULT_MODE


@pytest.fixture(params=MODES,
                ids=["wide-shadow", "binary-shadow-xcdremap-overlap1-fuseall", "binary-shadow-serial-unfused", "wide-shadow-serial-fusediffuse",
                     "wide-shadow-overlap1-unfused", "wide-shadow-fuseall-merged-queue", "wide-shadow-fusediffuse-merged-queue"], autouse=True)
def trace_mode(request):
    (TRACE_MODE["ext"], TRACE_MODE["shadow"], TRACE_MODE["xcd"], TRACE_MODE["overlap"], TRACE_MODE["fuse"],
     TRACE_MODE["fuse_set"], TRACE_MODE["ext_order"]) = request.param
    yield


def _ctxs(d, p, n, env=None):
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    g, o = HipContext(n), OracleContext(n, threads=8)
    g.set_option("extend_tree", TRACE_MODE["ext"])
    g.set_option("shadow_tree", TRACE_MODE["shadow"])
    g.set_option("overlap", TRACE_MODE["overlap"])
    g.set_option("xcd_remap", TRACE_MODE["xcd"])
    g.set_option("fuse", TRACE_MODE["fuse"])
    for c in (g, o):
        c.upload_scene(d)
        if env is not None:
            c.upload_envmap(env)
        c.set_params(p)
        driver.reset_renderer(c)
    if TRACE_MODE["fuse_set"]:
        g.set_option("fuse_set", TRACE_MODE["fuse_set"])          # after the upload, which picks one for the scene
        g.set_option("ext_order", TRACE_MODE["ext_order"] if TRACE_MODE["ext_order"] >= 0 else (1 if TRACE_MODE["fuse_set"] == 31 else 0))
    return g, o


def _compare(g, o, what, check_queues=True, ext_set=False):
    cg, co = g.get_counters(), o.get_counters()
    g.finish()
    assert (cg == co).all(), f"{what}: counters {cg} vs {co}"
    if check_queues:
        for q in range(8):
            n = int(co[q])
            qa, qb = g.queue_read(q)[:n], o.queue_read(q)[:n]
            if q == Q.EXTENSION and ext_set:
                # the fused pass lists the continuing paths in path-id order where the separate material kernels append one segment
                # per material queue: the same SET (the reference's own order is whatever its atomic_inc produces), the regenerated
                # paths' block where the call order puts it
                assert np.array_equal(np.sort(qa), np.sort(qb)), f"{what}: extension queue holds different paths"
                if g.get_option("ext_order") == 2 and (ext_set == "merged" or (ext_set != "blocks" and n > 1 and (np.diff(qa.astype(np.int64)) > 0).all())):
                    # ext_order 2 with genRays between logic and the material kernels: regenerated and continuing paths as ONE list in path-id order
                    assert (np.diff(qa.astype(np.int64)) > 0).all(), f"{what}: merged extension queue not in path-id order"
                    continue
                r = int(co[Q.RAYGEN])
                regen = o.queue_read(Q.RAYGEN)[:r]
                if r and n > r and np.array_equal(qb[:r], regen):              # genRays was enqueued before the material kernels
                    assert np.array_equal(qa[:r], regen), f"{what}: regenerated block of the extension queue"
                    assert (np.diff(qa[r:].astype(np.int64)) > 0).all(), f"{what}: continuing paths not in path-id order"
                elif r and n > r and np.array_equal(qb[n - r:], regen):        # ... or after them
                    assert np.array_equal(qa[n - r:], regen), f"{what}: regenerated block of the extension queue"
                    assert (np.diff(qa[:n - r].astype(np.int64)) > 0).all(), f"{what}: continuing paths not in path-id order"
                continue
            # all queues, the extension queue included, are in canonical order (stable compaction + computed slots)
            assert np.array_equal(qa, qb), f"{what}: queue {q} differs"
    fails = common.state_diff(g.state_export(), o.state_export(), 0.0, 0.0)
    assert not fails, f"{what}: " + "; ".join(fails[:5])


def _lockstep(g, o, npix, iters):
    for it in range(iters):
        for name, fn in (("logic", lambda c: c.wf_logic(False)), ("raygen", lambda c: c.wf_raygen()),
                         ("materials", lambda c: c.wf_materials())):
            common.sync(g, o)
            fn(g); fn(o)
            _compare(g, o, f"it{it} {name}")
        cnt = o.get_counters().copy()
        for name, fn in (("extend", lambda c: c.wf_extend()), ("shadow", lambda c: c.wf_shadow())):
            common.sync(g, o)
            fn(g); fn(o)
            _compare(g, o, f"it{it} {name}")
        for c in (g, o):
            c.clear_queues()
            c.pixel_index_update(npix, int(cnt[0]))


def _lockstep_iterations(g, o, npix, iters, order=("logic", "raygen", "materials"), separate_queues=1):
    """Whole-iteration lockstep: logic / genRays / materials enqueued back to back as the reference's host does
    (src/tracer.cpp:247-251), which is when the device runs logic and the material kernels as ONE fused pass (api_wavefront.hip); state,
    counters and every queue -- the extension queue's order included -- compared after the three calls, then after the two
    traversals.  `_lockstep` above looks at the state after every single call and therefore always gets the separate kernels."""
    fns = {"logic": lambda c: c.wf_logic(False), "raygen": lambda c: c.wf_raygen(), "materials": lambda c: c.wf_materials()}
    g.profile_enable(1); g.profile_reset()
    for it in range(iters):
        common.sync(g, o)
        for c in (g, o):
            c.clear_queues()                        # the state sync above rewrote the counters: the queues are empty, say so
            for name in order:
                fns[name](c)
        fused_now = bool(TRACE_MODE["fuse"] and (separate_queues or g.get_option("fused_queue_mask") == 0xF8)) and g.get_option("ext_order") >= 1
        # ext_order 2 merges the regenerated paths in only when genRays sits between logic and the material kernels (api_wavefront.hip: extOrderFor)
        merged = fused_now and g.get_option("ext_order") == 2 and tuple(order) == ("logic", "raygen", "materials")
        _compare(g, o, f"it{it} {'+'.join(order)}", ext_set=("merged" if merged else fused_now))
        cnt = o.get_counters().copy()
        for c in (g, o):
            c.wf_extend(); c.wf_shadow()
        _compare(g, o, f"it{it} extend+shadow", ext_set=fused_now)
        for c in (g, o):
            c.clear_queues()
            c.pixel_index_update(npix, int(cnt[0]))
    g.finish()
    prof = g.profile_get()
    g.profile_enable(0)
    # the fused pass is what ran (with separate queues, or when it inlines every BSDF type; never with the option off)
    fused = TRACE_MODE["fuse"] and (separate_queues or g.get_option("fused_queue_mask") == 0xF8)
    assert prof["logic_fused"][1] == (iters if fused else 0) and prof["logic"][1] == (0 if fused else iters), prof


def _free_run(g, o, npix, iters):
    for it in range(iters):
        cg = driver.benchmark_iteration(g, npix)
        co = driver.benchmark_iteration(o, npix)
        assert (cg == co).all(), f"iteration {it}: counters {cg} vs {co}"
    fails = common.state_diff(g.state_export(), o.state_export(), 0.0, 0.0)
    assert not fails, "; ".join(fails[:5])
    pg, po = g.read_pixels(0), o.read_pixels(0)
    assert np.array_equal(pg[:, 3], po[:, 3]), "sample counts differ"
    assert common.fb_close(pg, po), "radiance sums differ"
    g.postprocess(); o.postprocess()
    assert np.allclose(g.read_pixels(1), o.read_pixels(1), rtol=4e-6, atol=1e-6)      # resolved + tone-mapped: derived from the sums above


def test_lockstep_simple_area_light():
    d = common.simple_scene()
    w, h, n = 48, 32, 2048
    p = common.scene_params(d, w, h, maxBounces=4)
    g, o = _ctxs(d, p, n)
    _lockstep(g, o, w * h, 6)
    _lockstep_iterations(g, o, w * h, 4, separate_queues=int(p["wfSeparateQueues"]))


@pytest.mark.parametrize("area,env,expl,impl,sep,roulette", [
    (1, 0, 1, 1, 1, 0), (0, 1, 1, 1, 1, 0), (1, 1, 1, 1, 0, 1), (1, 1, 1, 0, 1, 0), (1, 1, 0, 1, 1, 0), (0, 0, 1, 1, 1, 1)])
def test_lockstep_all_bsdfs_flag_matrix(area, env, expl, impl, sep, roulette):
    d = common.mixed_material_scene()
    w, h, n = 64, 48, 4096
    p = common.scene_params(d, w, h, maxBounces=5, useAreaLight=area, useEnvMap=env, sampleExpl=expl, sampleImpl=impl,
                            wfSeparateQueues=sep, useRoulette=roulette, envMapStrength=1.5)
    g, o = _ctxs(d, p, n, env=host.synthetic_sky(64, 32))
    _lockstep(g, o, w * h, 7)
    _lockstep_iterations(g, o, w * h, 5, separate_queues=sep)
    _lockstep_iterations(g, o, w * h, 3, order=("logic", "materials", "raygen"), separate_queues=sep)


def test_deferred_logic_call_patterns():
    """flx_wf_logic is deferred until the next call shows whether the material kernels follow (api_wavefront.hip).  Call sequences that break the
    logic -> [genRays ->] materials pattern, ask for something in between or repeat a call must give what the oracle gives for the
    same sequence, and the fused pass must run exactly when the pattern is complete."""
    d = common.mixed_material_scene()
    w, h, n = 64, 48, 4096 + 37                      # not a multiple of the block sizes
    p = common.scene_params(d, w, h, maxBounces=5, useAreaLight=1, useEnvMap=1, wfSeparateQueues=1)
    g, o = _ctxs(d, p, n, env=host.synthetic_sky(64, 32))
    _free_run(g, o, w * h, 3)                        # some mixed steady state
    p2 = p.copy(); p2["maxBounces"] = 3

    def tail(c):
        c.wf_extend(); c.wf_shadow()

    patterns = {
        "plain": (lambda c: (c.wf_logic(False), c.wf_raygen(), c.wf_materials(), tail(c)), 1),
        "materials first": (lambda c: (c.wf_logic(False), c.wf_materials(), c.wf_raygen(), tail(c)), 1),
        "no raygen": (lambda c: (c.wf_logic(False), c.wf_materials(), tail(c)), 1),
        "counters in between": (lambda c: (c.wf_logic(False), np.array(c.get_counters()), c.finish(), c.wf_raygen(), c.wf_materials(), tail(c)), 0),
        "counters after raygen": (lambda c: (c.wf_logic(False), c.wf_raygen(), c.get_counters(), c.wf_materials(), tail(c)), 0),
        "params in between": (lambda c: (c.wf_logic(False), c.set_params(p2), c.wf_raygen(), c.wf_materials(), c.set_params(p), tail(c)), 0),
        "export in between": (lambda c: (c.wf_logic(False), c.state_export(), c.wf_raygen(), c.wf_materials(), tail(c)), 0),
        "logic without materials": (lambda c: (c.wf_logic(False), c.wf_raygen(), tail(c)), 0),
        # material counters not known to be zero (set_counters by the sync below, no clear since): the fused scatter could not number the
        # lists from zero, so the plain kernels must run
        "counters unknown": (lambda c: (c.wf_logic(False), c.wf_raygen(), c.wf_materials(), tail(c)), 0),
    }
    for name, (seq, fused_passes) in patterns.items():
        common.sync(g, o)
        if name != "counters unknown":
            for c in (g, o):
                c.clear_queues()
        g.profile_enable(1); g.profile_reset()
        seq(g); seq(o)
        want = fused_passes if TRACE_MODE["fuse"] else 0
        _compare(g, o, name, ext_set=bool(want) and g.get_option("ext_order") >= 1)
        prof = g.profile_get(); g.profile_enable(0)
        assert prof["logic_fused"][1] == want, (name, prof)
        for c in (g, o):
            c.clear_queues()
            c.pixel_index_update(w * h, 100)


@pytest.mark.parametrize("sep", [0, 1])
def test_free_running_render_bit_identical(sep):
    """40 benchmark-style iterations without re-synchronising: counters per iteration, final state and image."""
    d = common.mixed_material_scene()
    w, h, n = 96, 64, 8192           # numTasks > numPixels: several paths per pixel in flight
    p = common.scene_params(d, w, h, maxBounces=6, useAreaLight=1, useEnvMap=1, wfSeparateQueues=sep)
    g, o = _ctxs(d, p, n, env=host.synthetic_sky(64, 32))
    _free_run(g, o, w * h, 40)


@pytest.mark.parametrize("area,env,expl,impl,sep,roulette", [
    (1, 0, 1, 1, 1, 0), (0, 1, 1, 1, 1, 0), (1, 1, 1, 1, 0, 1), (1, 1, 1, 0, 1, 0), (1, 1, 0, 1, 1, 0), (0, 0, 1, 1, 1, 1)])
def test_free_running_flag_matrix(area, env, expl, impl, sep, roulette):
    """The six flag sets of the lockstep matrix, FREE-running for 30 iterations (no state import in between): this is where the
    regenerated-path flag bits (flx_device.h: k_raygen stores only the live records) live through logic / materials / extend and
    where the export fix-up has to reproduce genRays' reset values -- final state, counters and image against the oracle."""
    d = common.mixed_material_scene()
    w, h, n = 72, 50, 8192
    p = common.scene_params(d, w, h, maxBounces=5, useAreaLight=area, useEnvMap=env, sampleExpl=expl, sampleImpl=impl,
                            wfSeparateQueues=sep, useRoulette=roulette, envMapStrength=1.5)
    g, o = _ctxs(d, p, n, env=host.synthetic_sky(64, 32))
    for it in range(30):
        cg = driver.benchmark_iteration(g, w * h)
        co = driver.benchmark_iteration(o, w * h)
        assert (cg == co).all(), f"iteration {it}: counters {cg} vs {co}"
        if it in (0, 1, 7, 29):                       # incl. the states right after the first regenerations
            fails = common.state_diff(g.state_export(), o.state_export(), 0.0, 0.0)
            assert not fails, f"iteration {it}: " + "; ".join(fails[:5])
    pg, po = g.read_pixels(0), o.read_pixels(0)
    assert common.fb_close(pg, po)


def test_first_frame_preview_path():
    d = common.simple_scene()
    w, h, n = 40, 30, 2048
    p = common.scene_params(d, w, h, maxBounces=6)
    g, o = _ctxs(d, p, n)
    cg = driver.first_frame(g, p, w * h)
    co = driver.first_frame(o, p, w * h)
    assert (cg == co).all()
    _compare(g, o, "first frame", check_queues=False)
    _free_run(g, o, w * h, 6)


def test_golden_fixture_teapot():
    """tests/golden/teapot_*.npz: scene arrays + per-iteration counters + final image produced in the build
    container by the REFERENCE's own kernels (scripts/make_golden.py)."""
    import os
    path = os.path.join(common.GOLDEN, "teapot_wf.npz")
    if not os.path.exists(path):
        pytest.skip("golden fixture missing")
    from fluctus_amd.device import HipContext
    z = np.load(path)
    d = host.SceneData()
    d.tris = z["tris"].view(wire.TRIANGLE).reshape(-1)
    d.nodes = z["nodes"].view(wire.NODE).reshape(-1)
    d.indices = z["indices"]
    d.materials = z["materials"].view(wire.MATERIAL).reshape(-1)
    d.texdesc = np.zeros(0, wire.TEXDESC); d.texdata = np.zeros(0, np.uint8)
    p = z["params"].view(wire.RENDER_PARAMS).reshape(())
    w, h = int(p["width"]), int(p["height"])
    g = HipContext(int(z["num_tasks"]))
    g.set_option("extend_tree", TRACE_MODE["ext"]); g.set_option("shadow_tree", TRACE_MODE["shadow"])
    g.upload_scene(d); g.set_params(p); driver.reset_renderer(g)
    cnts = z["counters"]
    for it in range(cnts.shape[0]):
        c = driver.benchmark_iteration(g, w * h)
        # hit/miss decisions of the reference kernels (libm) and ours (flx_math) agree on all but grazing rays
        assert np.all(np.abs(c.astype(np.int64) - cnts[it].astype(np.int64)) <= max(4, int(2e-3 * w * h))), (it, c, cnts[it])
    # a FREE run against the reference's libm build forks at the first flipped grazing ray (see tests/test_oracle_golden.py); the exact
    # device-vs-reference comparison is test_device_resynchronised_iterations_vs_reference_fixture below -- here the conserved quantities
    pg = g.read_pixels(0)
    ref = z["pixels"]
    assert np.abs(pg[:, 3] - ref[:, 3]).max() <= 3
    assert abs(pg[:, 3].sum() - ref[:, 3].sum()) <= 2e-3 * ref[:, 3].sum()
    assert abs(pg[:, :3].sum() / pg[:, 3].sum() - ref[:, :3].sum() / ref[:, 3].sum()) <= 5e-3 * ref[:, :3].sum() / ref[:, 3].sum()


def test_device_resynchronised_iterations_vs_reference_fixture():
    """tests/golden/teapot_resync.npz (BASELINE.json configs[0] geometry, reference kernels): every iteration restarted from the
    REFERENCE's state, so the device is compared with the reference exactly, iteration by iteration: counters ==, integers ==,
    floats within the libm-vs-flx_math tolerance, framebuffer deltas, hit-index flips counted (<= 1 of 49 152 rays)."""
    import os
    import test_oracle_golden as og
    from fluctus_amd.device import HipContext
    path = os.path.join(common.GOLDEN, "teapot_resync.npz")
    if not os.path.exists(path):
        pytest.skip("golden fixture missing")
    z = np.load(path)
    g = HipContext(int(z["num_tasks"]))
    g.set_option("extend_tree", TRACE_MODE["ext"]); g.set_option("shadow_tree", TRACE_MODE["shadow"])
    g.set_option("overlap", TRACE_MODE["overlap"])
    g.upload_scene(og._load_scene(z)); g.set_params(z["params"].view(wire.RENDER_PARAMS).reshape(()))
    rays, flips = og.resync_check(g, z, flip_budget=1)
    assert rays == 12 * 4096


def test_large_queue_properties():
    """Full-size sanity on a bigger procedural scene (no oracle run): conservation laws of the wavefront loop."""
    from fluctus_amd.device import HipContext
    d = host.generate_scene("conference", 60000, 43)
    host.build_bvh(d, "binned")
    w, h, n = 640, 360, 1 << 18
    p = wire.default_params(w, h, d.world_radius, d.tris.size)
    wire.look_at(p, (0.0, 1.2, 2.6), (0.0, 0.2, 0.0))
    p["maxBounces"], p["wfSeparateQueues"] = 8, 1
    g = HipContext(n)
    g.upload_scene(d); g.set_params(p); driver.reset_renderer(g)
    total_new = 0
    for it in range(24):
        c = driver.benchmark_iteration(g, w * h)
        # every live path is either regenerated or continued through exactly one material queue
        assert int(c[Q.RAYGEN]) + int(c[3:8].sum()) == n
        assert int(c[Q.EXTENSION]) == n
        assert int(c[Q.SHADOW]) <= int(c[3:8].sum())
        if it > 0:
            total_new += int(c[Q.RAYGEN])
    px = g.read_pixels(0)
    assert np.isfinite(px).all()
    # each splat adds exactly 1 to a pixel's sample count; paths regenerated in iterations 1..23 splatted once each
    assert int(px[:, 3].sum()) == total_new
    st = g.state_export().view(np.uint32)
    assert (st[COL.PATH_LEN] <= int(p["maxBounces"]) + 1).all()


@pytest.mark.parametrize("workload", ["kitchen", "conference", "courtyard-1440p", "courtyard-2160p"])
def test_full_size_properties_and_determinism(workload):
    """BASELINE.json configs[1..4] at full size (kitchen-proc ~0.5 M triangles 1920x1080 8 bounces env-map MIS; conference-proc
    GGX + area light; courtyard-proc 8.9 M triangles 2560x1440 12 bounces and 3840x2160 16 bounces, all BSDFs), 1 M paths: too big for the oracle, so
    size-independent properties are checked, and two independent runs -- different stream schedules AND different any-hit trees
    (4-wide quantised vs the reference's binary tree) -- must agree bit for bit."""
    from fluctus_amd.device import HipContext
    import bench
    if workload != "kitchen" and (TRACE_MODE["shadow"] != 4 or TRACE_MODE["xcd"] or TRACE_MODE["overlap"] != 2):
        pytest.skip("the A/B variants are exercised at full size on the kitchen scene only")
    d, p, env = bench.build_workload(name=workload)
    n, npix = 1 << 20, int(p["width"]) * int(p["height"])
    outs = []
    for run in range(2):
        g = HipContext(n)
        g.set_option("extend_tree", TRACE_MODE["ext"])
        # second run: the BINARY any-hit traversal and a fully serial schedule -- same bits as the 4-wide / overlapped first run
        g.set_option("shadow_tree", TRACE_MODE["shadow"] if run == 0 else 2)
        g.set_option("overlap", TRACE_MODE["overlap"] if run == 0 else 0)
        g.upload_scene(d); g.upload_envmap(env); g.set_params(p); driver.reset_renderer(g)
        cnts = []
        for it in range(12):
            c = driver.benchmark_iteration(g, npix)
            cnts.append(c)
            assert int(c[Q.RAYGEN]) + int(c[3:8].sum()) == n           # regenerate or continue, exactly once
            assert int(c[Q.EXTENSION]) == n and int(c[Q.SHADOW]) <= int(c[3:8].sum())
        st = g.state_export()
        px = g.read_pixels(0)
        assert np.isfinite(px).all() and (px[:, 3] >= 0).all()
        assert int(px[:, 3].sum()) == sum(int(c[Q.RAYGEN]) for c in cnts[1:])
        iu = st.view(np.uint32)
        assert (iu[COL.PATH_LEN] <= int(p["maxBounces"]) + 1).all() and (iu[COL.PIXEL_INDEX] < npix).all()
        hit = iu[COL.HIT_I].view(np.int32)
        assert ((hit >= -1) & (hit < d.tris.size)).all()
        nrm = np.sqrt(st[COL.DIR] ** 2 + st[COL.DIR + 1] ** 2 + st[COL.DIR + 2] ** 2)
        live = iu[COL.PATH_LEN] > 0
        assert np.allclose(nrm[live & (st[COL.T] + st[COL.T + 1] + st[COL.T + 2] > 0)], 1.0, atol=1e-3)
        outs.append((np.stack(cnts), st, px))
        g.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert not common.state_diff(outs[0][1], outs[1][1], 0.0, 0.0)
    assert common.fb_close(outs[0][2], outs[1][2])


@pytest.mark.parametrize("workload", ["kitchen", "conference", "courtyard-1440p"])
def test_full_size_free_run_vs_oracle(workload):
    """The bench scenes themselves (kitchen-proc 0.5 M triangles 1080p env-map MIS; conference-proc area light, GGX / glossy / diffuse;
    courtyard-proc 8.9 M triangles 1440p 12 bounces, all six BSDFs) with
    1 M paths in flight, 10 free-running iterations on the product's default path (fused logic pass, 4-wide any-hit, two streams) and
    the bit-exact closest hit, against the oracle: counters after every iteration, the final path state bit for bit, the framebuffer."""
    if not is_default_mode():
        pytest.skip("default configuration only (the variants run on the small scenes)")
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    import bench
    d, p, env = bench.build_workload(name=workload)
    n, npix = 1 << 20, int(p["width"]) * int(p["height"])
    g, o = HipContext(n), OracleContext(n, threads=16)
    g.set_option("extend_tree", 2)
    for c in (g, o):
        c.upload_scene(d); c.upload_envmap(env); c.set_params(p); driver.reset_renderer(c)
    for it in range(10):
        cg = driver.benchmark_iteration(g, npix)
        co = driver.benchmark_iteration(o, npix)
        assert (cg == co).all(), f"iteration {it}: counters {cg} vs {co}"
    fails = common.state_diff(g.state_export(), o.state_export(), 0.0, 0.0)
    assert not fails, "; ".join(fails[:5])
    assert common.fb_close(g.read_pixels(0), o.read_pixels(0))
    g.close()


def test_c_abi_error_paths():
    """Errors come back as return codes + flx_last_error, never as crashes or silent fallbacks."""
    import ctypes as C
    from fluctus_amd import device
    L = device.lib()
    h = C.c_void_p()
    assert L.flx_create(0, C.c_uint32(0), C.byref(h)) != 0 and b"num_tasks" in L.flx_last_error(None)
    assert L.flx_create(99, C.c_uint32(1024), C.byref(h)) != 0 and b"device" in L.flx_last_error(None)
    g = device.HipContext(1024)
    with pytest.raises(RuntimeError, match="set params first"):
        g.wf_reset()
    d = common.simple_scene()
    p = common.scene_params(d, 16, 16)
    g.set_params(p)
    with pytest.raises(RuntimeError, match="upload a scene first"):
        g.wf_extend()
    bad = host.SceneData()
    bad.tris, bad.nodes, bad.materials, bad.texdesc, bad.texdata = d.tris, d.nodes, d.materials, d.texdesc, d.texdata
    bad.indices = d.indices.copy(); bad.indices[3] = d.tris.size + 7
    with pytest.raises(RuntimeError, match="index out of range"):
        g.upload_scene(bad)
    bad.indices = d.indices
    bad.tris = d.tris.copy(); bad.tris["matId"][0] = 5
    with pytest.raises(RuntimeError, match="material id out of range"):
        g.upload_scene(bad)
    with pytest.raises(RuntimeError, match="unknown option"):
        g.set_option("no_such_option", 1)
    p0 = p.copy(); p0["width"] = 0
    with pytest.raises(RuntimeError, match="zero-sized"):
        g.set_params(p0)
    g.upload_scene(d); g.set_params(p)
    driver.reset_renderer(g)
    driver.benchmark_iteration(g, 256)          # still usable after the errors


def test_single_leaf_scene_and_deep_stack_spill():
    """Edge cases of the traversal layout: a scene that is ONE leaf (synthetic root) and a degenerate, very deep tree (a right-leaning
    chain of 40 levels): the upload sizes the spill area for it and the kernels walk it.  The name is historical: no ray of this test
    spills -- the tree's depth bounds the stack, it does not fill it; over these six iterations no binary stack holds more than 1 entry
    (tests/test_stack_spill.py::test_the_older_chain_tests_never_leave_the_lds_levels states the figures).  The spill paths are tested on
    rays that provably reach them in tests/test_gpu_stack_spill.py."""
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    # (a) two triangles -> the whole BVH is a single leaf node
    d = common.small_mesh_scene(n=6)
    d.tris = d.tris[:2].copy()
    d.materials = np.array([common.default_material()], wire.MATERIAL)
    d.texdesc = np.zeros(0, wire.TEXDESC); d.texdata = np.zeros(0, np.uint8)
    host.build_bvh(d, "sbvh")
    assert d.nodes.size == 1 and d.nodes[0]["nPrims"] == 2
    p = common.scene_params(d, 32, 32, maxBounces=3)
    g, o = _ctxs(d, p, 1024)
    _free_run(g, o, 32 * 32, 6)
    # (b) hand-built right-leaning chain of 40 levels: every inner node = {leaf with 1 triangle, rest}
    d = common.small_mesh_scene(n=6)
    d.tris = d.tris[:41].copy()
    d.materials = np.array([common.default_material()], wire.MATERIAL)
    d.texdesc = np.zeros(0, wire.TEXDESC); d.texdata = np.zeros(0, np.uint8)
    nt = d.tris.size
    P = np.stack([np.stack([d.tris[v]["p"][k] for k in "xyz"], 1) for v in ("v0", "v1", "v2")], 1)   # (nt, 3, 3)
    tmin, tmax = P.min(1), P.max(1)
    nodes = np.zeros(2 * nt - 1, wire.NODE)
    sufmin = np.minimum.accumulate(tmin[::-1], 0)[::-1]; sufmax = np.maximum.accumulate(tmax[::-1], 0)[::-1]
    def setbox(n, mn, mx):
        for k, a in enumerate("xyz"):
            nodes[n]["bmin"][a] = mn[k]; nodes[n]["bmax"][a] = mx[k]
    idx = 0
    for t in range(nt - 1):                       # inner node idx: left = leaf(t) at idx+1, right = idx+2
        setbox(idx, sufmin[t], sufmax[t]); nodes[idx]["parent"] = idx - 2 if t else -1; nodes[idx]["nPrims"] = 0
        nodes[idx]["iStartOrRight"] = idx + 2
        setbox(idx + 1, tmin[t], tmax[t]); nodes[idx + 1]["parent"] = idx; nodes[idx + 1]["nPrims"] = 1; nodes[idx + 1]["iStartOrRight"] = t
        idx += 2
    setbox(idx, tmin[nt - 1], tmax[nt - 1]); nodes[idx]["parent"] = idx - 2; nodes[idx]["nPrims"] = 1; nodes[idx]["iStartOrRight"] = nt - 1
    d.nodes, d.indices = nodes, np.arange(nt, dtype=np.uint32)
    d.world_radius = float(0.5 * np.linalg.norm(sufmax[0] - sufmin[0]))
    p = common.scene_params(d, 32, 32, maxBounces=3)
    g, o = _ctxs(d, p, 1024)
    _free_run(g, o, 32 * 32, 6)


@pytest.mark.parametrize("tag", ["area_sep", "env_area_single_rr", "denoiser_env_area_sep", "egyptcat"])
def test_device_vs_reference_kernel_outputs(tag):
    """The HIP path directly against the REFERENCE kernels' own outputs (tests/golden/steps_*.npz, produced by
    oracle/_ref): every kernel of two iterations, from the reference's input state.  Integers exact, floats within the
    libm-vs-flx_math tolerance (rtol 1e-4; 1e-3 for GGX pdf values, see tests/test_oracle_golden.py)."""
    import os
    from fluctus_amd.device import HipContext
    path = os.path.join(common.GOLDEN, f"steps_{tag}.npz")
    if not os.path.exists(path):
        pytest.skip("golden fixture missing")
    z = np.load(path)
    n = int(z["num_tasks"])
    p = z["params"].view(wire.RENDER_PARAMS).reshape(())
    d = common.fixture_scene(z)
    e = host.EnvMap(int(z["env_wh"][0]), int(z["env_wh"][1]), z["env_rgb"], z["env_prob"], z["env_alias"], z["env_pdf"])
    g = HipContext(n)
    g.set_option("extend_tree", TRACE_MODE["ext"]); g.set_option("shadow_tree", TRACE_MODE["shadow"])
    den = "aov" in z.files                         # fixture made with the reference's USE_OPTIX_DENOISER kernel builds
    if den:
        g.set_option("denoiser", 1)
    g.upload_scene(d); g.upload_envmap(e); g.set_params(p)
    if den:
        g.wf_reset()                               # feature buffers to their reset values
    names = [str(s) for s in z["names"]]
    fn = {"logic": lambda: g.wf_logic(False), "raygen": g.wf_raygen, "materials": g.wf_materials, "extend": g.wf_extend, "shadow": g.wf_shadow}
    npix = int(p["width"]) * int(p["height"])
    for k in range(1, len(names)):
        if names[k] not in fn:
            continue
        g.pixel_index_reset(); g.pixel_index_update(npix, int(z["pixel_cursor"][k - 1]))       # the reference's pixel cursor at that point
        g.state_import(z["states"][k - 1])
        for q in range(8):
            g.queue_write(q, z["queues"][k - 1][q])
        g.set_counters(z["counters"][k - 1])
        if den:
            before = np.stack([g.read_pixels(4), g.read_pixels(5)])
        fn[names[k]]()
        cnt = g.get_counters(); g.finish()
        if den:                                    # what this kernel ADDED to the albedo / normal accumulators vs what the reference's added
            after = np.stack([g.read_pixels(4), g.read_pixels(5)])
            want = z["aov"][k] - z["aov"][k - 1]
            assert np.array_equal((after - before)[..., 3], want[..., 3]), (names[k], "feature counts")
            assert np.allclose(after - before, want, rtol=1e-4, atol=1e-4), (names[k], "feature sums")
            assert names[k] == "logic" or not want.any()
        assert np.array_equal(cnt, z["counters"][k]), (k, names[k])
        for q in range(8):
            m = int(z["counters"][k][q])
            assert np.array_equal(g.queue_read(q)[:m], z["queues"][k][q][:m]), (names[k], q)
        sa, sb = g.state_export(), z["states"][k]
        mask = None
        if names[k] == "materials":
            mask = ~((sa[COL.T] == 0) & (sa[COL.T + 1] == 0) & (sa[COL.T + 2] == 0))
        col_rtol = {COL.LAST_PDF_W: np.where(common.sharp_lobe_paths(d, sb), 2e-2, 1e-3)} if names[k] == "materials" else None      # (ill-conditioned in the reference itself: common.sharp_lobe_paths)
        fails = common.state_diff(sa, sb, 1e-3 if names[k] == "materials" else 1e-4, 1e-5, mask=mask, col_rtol=col_rtol)
        assert not fails, f"step {k} {names[k]}: " + "; ".join(fails[:4])


def test_env_sample_table_bit_identical():
    """Round 5: the fused logic pass reads what next-event estimation derives from an importance-sampled texel -- direction of its centre, solid-angle pdf,
    radiance looked up along it -- from a per-texel table the library builds at flx_upload_envmap.  EVERY entry of that table equals, bit for
    bit, what the oracle computes inline with the reference kernel's calls in its order (orc_env_sample_table), for the reference's night.hdr and for a synthetic sky."""
    import bench
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    for env in (bench.night_env(), host.synthetic_sky(64, 32)):
        g, o = HipContext(256), OracleContext(256)
        g.upload_envmap(env); o.upload_envmap(env)
        tg, to = g.env_sample_table(env.w, env.h), o.env_sample_table()
        assert tg.shape == to.shape == (env.w * env.h, 8)
        bad = np.nonzero((tg.view(np.uint32) != to.view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, f"{bad.size} of {tg.shape[0]} texels differ, first {bad[:4]}: {tg[bad[:2]]} vs {to[bad[:2]]}"
        g.close()


def test_arithmetic_contract_device_vs_oracle():
    """include/flx_math.h is the arithmetic contract both sides compile: every function of it (own sin / cos / tan / atan2 / acos / asin /
    atan / pow / log / exp, IEEE division and sqrt, fmin / fmax with their ordering of signed zeros) evaluated on the device
    (flx_math_probe) and on the host (orc_math_array) over random operands, the special values and every pairing of +-0, +-inf, NaN:
    identical bit patterns.  (Round 4: the host spelling of fmax returned -0 for max(0, -0), v_max_f32 returns +0 -- invisible to every
    comparison in the path, visible as a sign bit in a stored lastPdfImplicit for ~1 path in 10^6.)"""
    from fluctus_amd.device import HipContext
    from oracle import binding as ob
    g = HipContext(1024)
    rng = np.random.RandomState(7)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 0.5, -0.5, 2.0, 1e-20, 1e20],
                       np.float32)
    sa, sb = [x.reshape(-1) for x in np.meshgrid(special, special)]
    names = {0: "sin", 1: "cos", 2: "tan", 3: "atan2", 4: "acos", 5: "pow", 6: "log", 7: "exp", 8: "asin", 9: "atan", 10: "fmin", 11: "fmax",
             12: "div", 13: "sqrt", 14: "mul", 15: "add"}
    dom = {0: (-8000, 8000), 1: (-8000, 8000), 2: (-1.5, 1.5), 3: (-4, 4), 4: (-1, 1), 5: (1e-3, 4), 6: (1e-6, 1e6), 7: (-80, 80), 8: (-1, 1), 9: (-50, 50),
           10: (-3, 3), 11: (-3, 3), 12: (-100, 100), 13: (0, 1e6), 14: (-1e3, 1e3), 15: (-1e3, 1e3)}
    for fn, name in names.items():
        lo, hi = dom[fn]
        a = np.concatenate([rng.uniform(lo, hi, 200000).astype(np.float32), sa]) if fn in (10, 11, 12, 14, 15) else rng.uniform(lo, hi, 200000).astype(np.float32)
        b = np.concatenate([rng.uniform(lo, hi, 200000).astype(np.float32), sb]) if fn in (10, 11, 12, 14, 15) else (rng.uniform(-4, 4, a.size) if fn == 3 else rng.uniform(0.2, 3.0, a.size)).astype(np.float32)
        if fn in (10, 11):                           # plenty of equal operands and zeros of either sign
            b[:50000] = a[:50000]; a[50000:60000] = 0.0; b[50000:55000] = -0.0; b[55000:60000] = 0.0; a[55000:57000] = -0.0
        dv, hv = g.math_probe(fn, a, b), ob.math_array(fn, a, b)
        nan = np.isnan(dv.view(np.float32)) & np.isnan(hv.view(np.float32))      # (NaN payloads / signs are not part of the contract)
        bad = (dv != hv) & ~nan
        assert not bad.any(), f"{name}: {int(bad.sum())} of {a.size} results differ, first: {name}({a[bad][0]!r}, {b[bad][0]!r}) = {dv[bad][0]:#010x} (device) vs {hv[bad][0]:#010x} (host)"
    g.close()
