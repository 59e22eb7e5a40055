"""GPU: option "lazy_hit_commit" changes no state any call can see.

With the option on (the default) the fused RAW pass k_logic<USE_DIFFUSE, RAW, LAZY> stores neither the committed hit point nor the uv record: the
ray it consumed survives in the second {ORIG, DIR} pair, and k_settle_hits writes the two records from it when a call could look before the next
extension launch of the intact chain has overwritten them.  Two contexts run the same calls from the same inputs, one with the option off (the
stores of the parent), one with it on, and are compared EXACTLY -- exported path state, all eight queues below their counters, the counters, the
sample counts of the accumulation buffer; its radiance sums see below -- at the points where the dropped stores used to be visible:

  1. between flx_wf_materials and flx_wf_extend, at iterations 1, 3 and 9 (the observation the stores existed for);
  2. after the full step at the same iterations;
  3. after a second flx_wf_logic with no extension launch in between;
  4. after [logic, raygen, materials, clear_queues, extend]: an extension launch whose queue no longer holds the pending paths;
  5. with extend_tree 2 in the chain: no RAW records, so nothing is ever pending;
  6. after an observation as in (1) the run goes on and matches at the next full step too, whose pass is lazy again: settling early does not
     disturb the chain.

Scene: the small procedural kitchen (3 000 triangles; glossy, GGX and delta surfaces beside the diffuse ones, so paths whose BSDF the pass does not
inline -- class C2, served by k_material_rest -- exist, which every test asserts) under the night environment map, 64 x 48 pixels; 4 133 paths (a
partial last wave) and 17 x 256.

(3) has a clear_queues between the chain and the second logic.  The queues hold numTasks entries each; a second logic without a clear appends its
lists behind the first one's, and here the two shadow lists alone are longer than that (three quarters of the paths sample a light in either pass):
the call sequence is outside what the boundary -- and the reference's own queues -- can hold (tests/test_gpu_fuzz.py keeps to "logic once per
clear" for the same reason).  clear_queues is no extension launch and settles nothing (CALL_NEUTRAL): the second logic still finds the hits pending.

The radiance sums of the accumulation buffer are float atomics: paths of different waves that end on one pixel in one pass are added in the order
the waves arrive, which no build fixes -- two contexts with the SAME option differ in a handful of pixels after nine steps here, in the last bit or
two (4 133 paths on 3 072 pixels).  So the sums are compared with common.fb_close, the bound of a sum of N fp32 terms added in any order, like every
framebuffer comparison of this suite; every term of those sums is covered exactly, as the Ei column of the exported states before the pass that
splats it.
"""
import os
import numpy as np
import pytest
import common
from common import Q
from fluctus_amd import host, wire, driver

pytestmark = pytest.mark.gpu

W, H = 64, 48
NPIX = W * H
COUNTS = [4096 + 37, 17 * 256]
PENDING = 32                                           # flx_get_option "phase": bit 5 = previous hits pending
_case = []


def _inputs():
    if not _case:
        d = host.generate_scene("kitchen", 3000, 7)
        host.build_bvh(d, "binned")
        p = wire.default_params(W, H, d.world_radius, d.tris.size)
        wire.look_at(p, (0.0, 1.2, 2.6), (0.0, 0.2, 0.0), fov=60.0)
        p["maxBounces"], p["useEnvMap"], p["useAreaLight"], p["wfSeparateQueues"] = 8, 1, 0, 1
        z = np.load(os.path.join(common.GOLDEN, "night_env.npz"))
        _case.append((d, p, host.envmap_from_rgb(int(z["w"]), int(z["h"]), z["rgb"])))
    return _case[0]


def _pair(n, **options):
    """(eager, lazy): two contexts with the same inputs and options, "lazy_hit_commit" 0 and 1"""
    from fluctus_amd.device import HipContext
    d, p, env = _inputs()
    out = []
    for lazy in (0, 1):
        c = HipContext(n)
        c.upload_scene(d); c.upload_envmap(env); c.set_params(p)
        c.set_option("fuse_set", 1)                    # the diffuse-inlining pass, whatever the upload chose for this small scene
        c.set_option("lazy_hit_commit", lazy)
        for k, v in options.items():
            c.set_option(k, v)
        driver.reset_renderer(c)
        out.append(c)
    return out


def _chain(c):
    c.wf_logic(False); c.wf_raygen(); c.wf_materials()


def _finish_step(c):
    cnt = c.get_counters()
    c.wf_extend(); c.wf_shadow(); c.clear_queues(); c.finish()
    cnt = np.array(cnt, copy=True)
    c.pixel_index_update(NPIX, int(cnt[Q.RAYGEN]))
    return cnt


def _pending(c):
    return bool(c.get_option("phase") & PENDING)


def _same(eager, lazy, what):
    """the exact comparison; returns the counters"""
    cs = []
    for c in (eager, lazy):
        cnt = c.get_counters(); c.finish()
        cs.append(np.array(cnt, copy=True))
    assert (cs[0] == cs[1]).all(), f"{what}: counters {cs[0]} vs {cs[1]}"
    for q in range(Q.NUM):
        m = int(cs[0][q])
        assert np.array_equal(eager.queue_read(q)[:m], lazy.queue_read(q)[:m]), f"{what}: queue {q} differs"
    sa, sb = eager.state_export().view(np.uint32), lazy.state_export().view(np.uint32)
    rows = np.flatnonzero((sa != sb).any(axis=1))
    assert rows.size == 0, f"{what}: exported state differs in columns {[common.colname(int(r)) for r in rows]}, {int((sa != sb).any(axis=0).sum())} paths"
    assert not lazy.get_option("phase") & 8 and not _pending(lazy), f"{what}: an export left RAW or pending records behind"
    pa, pb = eager.read_pixels(0), lazy.read_pixels(0)
    assert np.array_equal(pa[:, 3], pb[:, 3]), f"{what}: the sample counts differ in {int((pa[:, 3] != pb[:, 3]).sum())} pixels"
    assert common.fb_close(pa, pb), f"{what}: the accumulation buffer differs beyond the order of its float atomics"
    return cs[0]


def _not_inlined(cnt):
    return int(cnt[Q.GLOSSY]) + int(cnt[Q.GGX_REFL]) + int(cnt[Q.GGX_REFR]) + int(cnt[Q.DELTA])


def _warm(eager, lazy, steps):
    """whole steps with nobody looking: from the second on the lazy context's pass leaves its hits pending and the extension launch takes them over"""
    for it in range(steps):
        for c in (eager, lazy):
            _chain(c)
        assert not _pending(eager)
        assert _pending(lazy) == (it > 0), f"step {it + 1}: the pass with lazy_hit_commit {'did not leave' if it > 0 else 'left'} its hits pending"
        for c in (eager, lazy):
            _finish_step(c)
        assert not _pending(lazy), "the extension launch of the intact chain takes the pending hits over"


@pytest.mark.parametrize("n", COUNTS)
def test_between_materials_and_extend_and_after_the_step(n):
    """points 1 and 2.  (Every comparison commits what is RAW, so the pass after one is not a RAW pass: iterations 3 and 9 are, iteration 1 -- the
    first after the reset, nothing traced yet -- cannot be.)"""
    eager, lazy = _pair(n)
    c2 = 0
    for it in range(1, 10):
        for c in (eager, lazy):
            _chain(c)
        if it in (1, 3, 9):
            assert _pending(lazy) == (it > 1)
            c2 += _not_inlined(_same(eager, lazy, f"n {n}, iteration {it}, between materials and extend"))
        for c in (eager, lazy):
            _finish_step(c)
        if it in (1, 3, 9):
            _same(eager, lazy, f"n {n}, after the full step {it}")
    assert c2 > 0, "no path of a BSDF type the pass does not inline: the test does not reach k_material_rest's commit"


@pytest.mark.parametrize("n", COUNTS)
def test_settling_early_does_not_disturb_the_chain(n):
    """point 6: the records settled for an observer between materials and extend, the extension launch behind it, then a step whose pass is lazy again"""
    eager, lazy = _pair(n)
    _warm(eager, lazy, 3)
    for c in (eager, lazy):
        _chain(c)
    assert _pending(lazy)
    _same(eager, lazy, f"n {n}, between materials and extend")
    for c in (eager, lazy):
        _finish_step(c)
    for c in (eager, lazy):
        _chain(c)
    assert _pending(lazy), "the extension launch behind the observation left RAW records, and the pass over them is the lazy one"
    for c in (eager, lazy):
        _finish_step(c)
    _same(eager, lazy, f"n {n}, after the full step that follows the observation")


@pytest.mark.parametrize("n", COUNTS)
def test_second_logic_without_an_extension_launch(n):
    """point 3 (module docstring: why a clear_queues stands in front of the second logic)"""
    eager, lazy = _pair(n)
    _warm(eager, lazy, 3)
    for c in (eager, lazy):
        _chain(c)
    assert _pending(lazy)
    cnt = lazy.get_counters(); lazy.finish()
    c2 = _not_inlined(np.array(cnt, copy=True))
    for c in (eager, lazy):
        c.clear_queues()
    assert _pending(lazy), "clear_queues settles nothing"
    for c in (eager, lazy):
        c.wf_logic(False)
    assert not _pending(lazy), "the second logic pass starts from settled records"
    _same(eager, lazy, f"n {n}, [logic, raygen, materials, clear_queues, logic]")
    assert c2 > 0


@pytest.mark.parametrize("n", COUNTS)
def test_queues_cleared_before_the_extension_launch(n):
    """point 4"""
    eager, lazy = _pair(n)
    _warm(eager, lazy, 3)
    for c in (eager, lazy):
        _chain(c)
    assert _pending(lazy)
    for c in (eager, lazy):
        c.clear_queues(); c.wf_extend()
    assert not _pending(lazy)
    _same(eager, lazy, f"n {n}, [logic, raygen, materials, clear_queues, extend]")
    for c in (eager, lazy):                             # ... and the run goes on from there
        c.wf_shadow(); c.clear_queues(); c.finish()
    for it in range(2):
        for c in (eager, lazy):
            _chain(c); _finish_step(c)
    _same(eager, lazy, f"n {n}, two steps after the cleared extension launch")


@pytest.mark.parametrize("n", COUNTS)
def test_binary_tree_extension_leaves_nothing_pending(n):
    """point 5"""
    eager, lazy = _pair(n, extend_tree=2)
    for it in range(1, 5):
        for c in (eager, lazy):
            _chain(c)
        assert not _pending(lazy) and not lazy.get_option("phase") & 8, "extend_tree 2 commits its hits: no RAW pass, nothing pending"
        if it == 3:
            _same(eager, lazy, f"n {n}, extend_tree 2, iteration {it}, between materials and extend")
        for c in (eager, lazy):
            _finish_step(c)
    _same(eager, lazy, f"n {n}, extend_tree 2, after four steps")
