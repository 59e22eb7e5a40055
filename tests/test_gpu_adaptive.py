"""flx_mk_adaptive_update, the list-driven microkernels and Tracer::renderAdaptive on the device.  The integrator is
deterministic per pixel, so everything here is compared BIT FOR BIT: the classification with the CPU counterpart (tests/adaptive_cpu.cpp), an
adaptive render with the uniform render after each pixel's own count."""
import os
import numpy as np
import pytest
import common
import adaptive_reference as A
import denoise_reference as R
from fluctus_amd import driver, host, wire

pytestmark = pytest.mark.gpu
KW = dict(maxBounces=4, useAreaLight=1, useEnvMap=1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return A.build_cpu(tmp_path_factory.mktemp("adaptive_gpu"))


@pytest.fixture(scope="module")
def scene():
    return common.mixed_material_scene(), host.synthetic_sky(64, 32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_ctx(scene, W, H, denoiser=1, moments=1, n=None):
    d, env = scene
    return R.ctx(d, W, H, n=n or W * H, denoiser=denoiser, moments=moments, env=env, **KW)


def check_update(g, exe, W, H, mom, **P):
    g.write_pixels(7, mom)
    count = g.mk_adaptive_update(**P)
    lst, flags = g.mk_active_read()
    cf, cr, cl = A.run_cpu(exe, W, H, mom, **P)
    assert count == cl.size == lst.size, (count, cl.size)
    assert np.array_equal(flags, cf), f"{(flags != cf).sum()} flag bytes differ"
    assert np.array_equal(lst, cl)
    return count


@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (5, 1), (3, 3), (7, 5), (33, 17), (80, 60), (257, 129), (640, 360), (1920, 1080)])
def test_update_vs_counterpart_synthetic(scene, exe, W, H):
    from test_adaptive import synthetic_moments
    g = make_ctx(scene, W, H, denoiser=0, n=max(W * H, 64))
    for dilate in (0, 1):
        for seed, kw in ((1, {}), (2, dict(threshold=0.2, min_samples=2, max_samples=8)), (3, dict(threshold=0.0, lum_floor=0.0)), (4, dict(min_samples=1, max_samples=1))):
            P = dict(A.DEFAULTS, **kw, dilate=dilate)
            mom = synthetic_moments(W, H, seed * 100 + W, P["min_samples"], P["max_samples"], P["threshold"], P["lum_floor"])
            check_update(g, exe, W, H, mom, **P)
    # all active / none active
    mom = np.zeros((W * H, 4), np.float32)
    assert check_update(g, exe, W, H, mom) == W * H
    mom[:] = [32.0, 32.0, 0.0, 32.0]
    assert check_update(g, exe, W, H, mom) == 0


def test_update_on_the_devices_own_moments(scene, exe):
    W, H = 80, 60
    g = make_ctx(scene, W, H)
    driver.render_single(g, g.params, 6)
    mom = g.read_pixels(7)
    for dilate in (0, 1):
        n = check_update(g, exe, W, H, mom, dilate=dilate)
        assert 0 < n < W * H


def uniform_stack(g, p, S):
    """the accumulation, the moments and both feature accumulators after every one of S uniform passes: 4 x (S + 1, N, 4), index = the count"""
    q = p.copy(); q["useRoulette"] = 0
    g.set_params(q); g.mk_reset()
    N = int(p["width"]) * int(p["height"])
    out = [np.zeros((S + 1, N, 4), np.float32) for _ in range(4)]
    for k, which in enumerate((0, 7, 4, 5)):
        out[k][0] = g.read_pixels(which)
    for s in range(1, S + 1):
        driver.render_single_pass(g, q["maxBounces"])
        for k, which in enumerate((0, 7, 4, 5)):
            out[k][s] = g.read_pixels(which)
    return out


def egyptcat():
    z = np.load(os.path.join(common.GOLDEN, "steps_egyptcat.npz"))
    p = z["params"].view(wire.RENDER_PARAMS).reshape(()).copy()
    return common.fixture_scene(z), p


@pytest.mark.parametrize("which", ["mixed", "egyptcat"])
def test_adaptive_equals_uniform_at_each_pixels_count(scene, exe, which):
    """THE property: pixel p of an adaptive render with n_p samples equals pixel p of the uniform render after n_p passes, bit for bit, in the
    colour, the moments and both feature accumulators; the colour also against the oracle's per-sample stack"""
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    LO, HI = 4, 32
    if which == "mixed":
        d, env = scene
        W, H = 80, 60
        p = common.scene_params(d, W, H, **KW)
    else:
        d, p = egyptcat()
        env = None
        W, H = int(p["width"]), int(p["height"])
    N = W * H

    def fresh(cls):
        c = cls(N) if cls is HipContext else cls(N, threads=8)
        if cls is HipContext:
            c.set_option("denoiser", 1); c.set_option("moments", 1)
        c.upload_scene(d)
        if env is not None:
            c.upload_envmap(env)
        c.set_params(p)
        return c
    uni = uniform_stack(fresh(HipContext), p, HI)
    o_smp, o_acc = A.per_sample_stack(fresh(OracleContext), p, HI)
    ar = np.arange(N)
    for dilate in (1, 0):
        g = fresh(HipContext)
        lists = []
        q, total = driver.render_adaptive(g, p, LO, HI, dilate=dilate, on_pass=lambda s, a: lists.append(a))
        px = g.read_pixels(0)
        n = px[:, 3].astype(np.int64)
        assert n.min() >= LO and n.max() <= HI and total == n.sum()
        assert len(np.unique(n)) >= 3, "the test scene must produce several distinct counts"
        for k, w in enumerate((0, 7, 4, 5)):
            assert np.array_equal(bits(g.read_pixels(w)), bits(uni[k][n, ar])), f"which = {w}, dilate {dilate}"
        assert np.array_equal(bits(px), bits(o_acc[n - 1, ar])), "colour differs from the oracle's per-sample stack"
        # the moments the oracle does not keep, from its per-sample radiance; and the whole run against the simulation
        spx, smom, hist = A.simulate(exe, W, H, o_smp, LO, HI, dilate=dilate)
        assert np.array_equal(bits(px), bits(spx)) and np.array_equal(bits(g.read_pixels(7)), bits(smom))
        assert lists == [c for c, _ in hist]
        print(f"{which} dilate {dilate}: {total} samples, {np.unique(n).size} distinct counts, {100 * (n == HI).mean():.1f} % at max")


def state_of(g):
    return g.state_export().view(np.uint32).copy(), [g.read_pixels(w).view(np.uint32).copy() for w in (0, 7, 4, 5)]


@pytest.mark.parametrize("name", ["empty", "one", "every_other", "last", "all"])
def test_arbitrary_lists(scene, name):
    W, H = 33, 17
    N = W * H
    lst = {"empty": [], "one": [N // 2], "every_other": list(range(0, N, 2)), "last": [N - 1], "all": list(range(N))}[name]
    lst = np.array(lst, np.uint32)
    a, b = make_ctx(scene, W, H), make_ctx(scene, W, H)
    for g in (a, b):
        driver.render_single(g, g.params, 2)
        g.mk_stats(reset=True)
    s0, f0 = state_of(a)
    a.mk_active_write(lst)
    got, _ = a.mk_active_read()
    assert np.array_equal(got, lst)
    driver.render_single_pass(a, KW["maxBounces"]); a.finish()
    driver.render_single_pass(b, KW["maxBounces"]); b.finish()
    sa, fa = state_of(a)
    sb, fb = state_of(b)
    listed = np.zeros(N, bool); listed[lst] = True
    cols = [c for c in range(64) if c not in common.PAD_COLS]
    for c in cols:
        assert np.array_equal(sa[c, :N][listed], sb[c, :N][listed]), f"listed pixels: column {c}"
        assert np.array_equal(sa[c, :N][~listed], s0[c, :N][~listed]), f"unlisted pixels touched: column {c}"
    for k in range(4):
        assert np.array_equal(fa[k][listed], fb[k][listed]) and np.array_equal(fa[k][~listed], f0[k][~listed]), k
    assert int(a.mk_stats()[3]) == lst.size and int(b.mk_stats()[3]) == N
    a.mk_adaptive_clear()
    with pytest.raises(RuntimeError, match="no list"):
        a.mk_active_read()


def test_errors_and_clearing_events(scene):
    W, H = 16, 12
    g = make_ctx(scene, W, H, moments=0, n=(W + 1) * H)
    p1 = g.params.copy()
    with pytest.raises(RuntimeError, match="needs the luminance moments"):
        g.mk_adaptive_update()
    g.set_option("moments", 1)
    driver.render_single(g, g.params, 2)
    for bad, msg in (([5, 5], "ascending"), ([7, 3], "ascending"), ([W * H], "out of range")):
        with pytest.raises(RuntimeError, match=msg):
            g.mk_active_write(bad)
    for bad in (dict(threshold=float("nan")), dict(threshold=-1.0), dict(max_samples=0), dict(min_samples=9, max_samples=8), dict(dilate=2), dict(lum_floor=float("inf"))):
        with pytest.raises(RuntimeError, match="flx_mk_adaptive_update"):
            g.mk_adaptive_update(**bad)

    def installed():
        try:
            g.mk_active_read()
            return True
        except RuntimeError:
            return False
    d, env = scene
    p2 = common.scene_params(d, W + 1, H, **KW)
    events = {"clear": g.mk_adaptive_clear, "mk_reset": g.mk_reset, "size": lambda: g.set_params(p2), "upload": lambda: g.upload_scene(d),
              "moments off": lambda: g.set_option("moments", 0), "partition": lambda: (g.set_partition(0, 2), g.set_partition(0, 1))}
    for name, ev in events.items():
        g.set_option("moments", 1)
        g.set_params(p1)
        g.mk_active_write([1, 2, 3])
        assert installed()
        ev()
        assert not installed(), name
    g.set_partition(1, 2)
    g.set_option("moments", 1)
    with pytest.raises(RuntimeError, match="single-GPU"):
        g.mk_adaptive_update()
    g.set_partition(0, 1)
    small = R.ctx(d, 16, 12, n=64, denoiser=0, moments=1, env=env, **KW)
    with pytest.raises(RuntimeError, match="num_tasks"):
        small.mk_adaptive_update()


def test_tracer_render_adaptive(scene):
    """Tracer::renderAdaptive equals the C-ABI sequence, restores "moments", and leaves renderSingle as it was"""
    from fluctus_amd.tracer import Tracer
    w, h = 64, 48
    d = host.generate_scene("kitchen", 6000, 3)
    host.build_bvh(d, "sbvh")

    def tracer():
        t = Tracer(w, h, 0, w * h)
        t.init(w, h, "proc:kitchen:6000:3")
        p = t.params
        wire.look_at(p, (0.0, 1.2, 2.6), (0.0, 0.2, 0.0))
        p["maxBounces"] = 3
        t.params = p
        return t
    ref = tracer(); ref.render_single(3)
    before = ref.read_pixels(0).copy()
    t = tracer()
    total = t.render_adaptive(4, 16, 0.05)
    px = t.read_pixels(0)
    assert total == int(px[:, 3].sum()) and px[:, 3].min() >= 4 and px[:, 3].max() <= 16 and len(np.unique(px[:, 3])) >= 3
    with pytest.raises(RuntimeError, match="moments"):
        t.read_pixels(7)
    for bad in ((4, (1 << 24) + 1, 0.05), (0, 4, 0.05), (8, 4, 0.05), (4, 8, float("nan"))):      # rejected before anything is switched on
        with pytest.raises(RuntimeError, match="renderAdaptive"):
            t.render_adaptive(*bad)
        with pytest.raises(RuntimeError, match="moments"):
            t.read_pixels(7)
    from fluctus_amd.device import HipContext
    g = HipContext(w * h)
    g.set_option("moments", 1)
    g.upload_scene(d)
    _, total2 = driver.render_adaptive(g, t.params, 4, 16, threshold=0.05)
    assert total2 == total and np.array_equal(bits(g.read_pixels(0)), bits(px))
    t.render_single(3)
    assert np.array_equal(bits(t.read_pixels(0)), bits(before)), "renderSingle after renderAdaptive differs"


def test_quality_at_equal_budget(scene):
    """80 x 60 against 512 spp: adaptive with S samples against uniform ceil(S / pixels) spp on the metric the stopping rule controls.  Both renders
    are deterministic: adaptive < uniform with no margin.  Values printed with -s."""
    W, H, LO, HI = 80, 60, 4, 32
    d, env = scene
    p = common.scene_params(d, W, H, **KW)
    truth = R.mk_render(d, W, H, 512, env=env).read_pixels(0)
    g = make_ctx(scene, W, H)
    _, S = driver.render_adaptive(g, p, LO, HI)
    spp = -(-S // (W * H))
    u = R.mk_render(d, W, H, spp, env=env).read_pixels(0)
    qa, ra = A.quality(g.read_pixels(0), truth)
    qu, ru = A.quality(u, truth)
    print(f"adaptive {S} samples ({S / (W * H):.2f} spp): metric {qa:.5f} rmse {ra:.5f} | uniform {spp} spp: metric {qu:.5f} rmse {ru:.5f}")
    assert qa < qu, (qa, qu)
