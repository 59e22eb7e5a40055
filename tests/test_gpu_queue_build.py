"""The queue build on the GPU (logic.hip: k_queue_build behind k_logic) in lockstep with the CPU oracle.

Scene: the small mixed-material scene of the fuzz and parity tests (all six BSDF types), closest hit and any hit on the binary trees
(extend_tree 2, shadow_tree 2: the bit-exact kernels, as tests/test_gpu_parity.py sets them), so device and oracle cannot fork on a tie and
NO case is excluded from the comparison.  From reset, 2 x maxBounces + 2 iterations; after every flx_wf_materials all eight queues and the
counters are compared with ==.  The extension queue of a fused pass with ext_order 1 / 2 is by design the oracle's SET in path-id order
(api_upload.hip: option "ext_order"), so there the expected queue is derived from the oracle's -- the regenerated paths' block where the call
order puts it, the continuing paths sorted by id; with ext_order 2 and genRays between logic and the material kernels everything sorted -- and
compared with == all the same.

Path counts: 64 and 257 (less than a tile, a tile + 1), 17 x 256 (whole blocks: the regrouped all-types pass), and 2 x 16384 + 337: not a
multiple of 256, three segments, so three persistent blocks, each with a base from the totals of the segments in front of it.
Every case runs twice in fresh contexts and must produce identical queues: the segment totals are integer atomic adds (any order, one sum), and
the two totals buffers alternate from pass to pass (8 iterations use each four times).
"""
import numpy as np
import pytest
import common
from common import Q
from fluctus_amd import host, driver

pytestmark = pytest.mark.gpu

W, H = 48, 40
MAXB = 3
ITERS = 2 * MAXB + 2
BIG = 2 * 16384 + 337


def _device(n, d, env, p, opt):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    g.set_option("extend_tree", 2); g.set_option("shadow_tree", 2)
    g.set_option("fuse", opt["fuse"])
    g.upload_scene(d)
    if env is not None:
        g.upload_envmap(env)
    g.set_params(p)
    g.set_option("fuse_set", opt["fuse_set"]); g.set_option("ext_order", opt["ext_order"])      # after the upload, which picks them for the scene
    return g


def _oracle(n, d, env, p):
    from oracle.binding import OracleContext
    o = OracleContext(n, threads=8)
    o.upload_scene(d)
    if env is not None:
        o.upload_envmap(env)
    o.set_params(p)
    return o


def _start(c, first):
    if first:                                   # Tracer::update's first frame (driver.first_frame): the iteration right after flx_wf_reset
        c.pixel_index_reset(); c.wf_reset(); c.wf_raygen(); c.wf_extend(); c.clear_queues()
    else:
        driver.reset_renderer(c)


def _calls(c, first, raygen_between):
    c.wf_logic(bool(first))
    if raygen_between:
        c.wf_raygen(); c.wf_materials()
    else:
        c.wf_materials(); c.wf_raygen()


def _queues(c):
    cnt = c.get_counters()
    if hasattr(c, "finish"):
        c.finish()
    cnt = np.array(cnt, copy=True)
    return cnt, [np.array(c.queue_read(q)[:int(cnt[q])], copy=True) for q in range(8)]


def _expected_extension(qo, cnt, opt, sep, raygen_between):
    """The oracle's extension queue in the order the device's options ask for (api_wavefront.hip: extOrderFor)."""
    fused = bool(opt["fuse"])                    # (every pass here follows a clear, and with a single material queue the all-types pass serves it)
    order = opt["ext_order"] if fused else 0
    if order == 2 and not raygen_between:
        order = 1
    ext, r, n = qo[Q.EXTENSION], int(cnt[Q.RAYGEN]), int(cnt[Q.EXTENSION])
    if order == 0:
        return ext
    if order == 2:
        return np.sort(ext)
    if raygen_between:
        assert np.array_equal(ext[:r], qo[Q.RAYGEN])
        return np.concatenate([ext[:r], np.sort(ext[r:])])
    assert np.array_equal(ext[n - r:], qo[Q.RAYGEN])
    return np.concatenate([np.sort(ext[:n - r]), ext[n - r:]])


def _run(n, opt, sep=1, lights=True, first_iters=0, raygen_between=True, relogic=False, oracle=True):
    """One case from reset.  Returns the device's counters and queues after every flx_wf_materials (and after the second flx_wf_logic)."""
    d = common.mixed_material_scene()
    p = common.scene_params(d, W, H, maxBounces=MAXB, useAreaLight=int(lights), useEnvMap=int(lights), wfSeparateQueues=sep)
    env = host.synthetic_sky(64, 32) if lights else None
    ctxs = [_device(n, d, env, p, opt)] + ([_oracle(n, d, env, p)] if oracle else [])
    g = ctxs[0]
    for c in ctxs:
        _start(c, first_iters > 0)
    seen = []
    for it in range(ITERS):
        first = it < first_iters
        for c in ctxs:
            _calls(c, first, raygen_between)
        cg, qg = _queues(g)
        seen.append((cg, qg))
        if oracle:
            co, qo = _queues(ctxs[1])
            assert np.array_equal(cg, co), f"iteration {it}: counters {cg} vs {co}"
            if not lights:
                assert int(co[Q.SHADOW]) == 0
            for q in range(8):
                want = _expected_extension(qo, co, opt, sep, raygen_between) if q == Q.EXTENSION else qo[q]
                assert np.array_equal(qg[q], want), f"iteration {it}: queue {q} differs"
        for c in ctxs:
            c.wf_extend(); c.wf_shadow()
        if relogic and it == 1:
            # a second flx_wf_logic with NO clear in between: the lists append behind non-zero counters.  `first` bounds a pass to W x H paths
            # (src/wf_logic.cl:45-48), and 2 x W x H <= n, so the queues (n entries) hold both passes; the counters are looked at right after
            # it -- the pass runs as the separate kernels, a fused pass needs empty material queues -- and nothing consumes the doubled lists
            assert first and 2 * W * H <= n
            for c in ctxs:
                c.wf_logic(True)
            cg, qg = _queues(g)
            seen.append((cg, qg))
            assert int(cg.sum()) > int(seen[-2][0].sum()), "the second pass appended nothing"
            if oracle:
                co, qo = _queues(ctxs[1])
                assert np.array_equal(cg, co), f"second logic: counters {cg} vs {co}"
                for q in range(8):
                    assert np.array_equal(qg[q], qo[q]), f"second logic: queue {q} differs"
            break                                # (the doubled raygen queue names paths twice: nothing defined follows)
        for c in ctxs:
            c.clear_queues()
            c.pixel_index_update(W * H, int(cg[Q.RAYGEN]))
    for c in ctxs:
        if hasattr(c, "close"):
            c.close()
    return seen


def _twice(n, opt, **kw):
    a = _run(n, opt, **kw)
    b = _run(n, opt, oracle=False, **kw)         # a fresh context, the device alone: the same queues, entry by entry
    assert len(a) == len(b)
    for k, ((ca, qa), (cb, qb)) in enumerate(zip(a, b)):
        assert np.array_equal(ca, cb), f"observation {k}: counters differ between two runs"
        for q in range(8):
            assert np.array_equal(qa[q], qb[q]), f"observation {k}: queue {q} differs between two runs"
    return a


DEFAULT = {"fuse": 1, "fuse_set": 31, "ext_order": 2}


@pytest.mark.parametrize("n", [64, 257, 17 * 256, BIG])
def test_path_counts(n):
    seen = _twice(n, DEFAULT)
    assert sum(int(c[Q.SHADOW]) for c, _ in seen) > 0 and sum(int(c[3:8].sum()) for c, _ in seen) > 0


@pytest.mark.parametrize("raygen_between", [True, False], ids=["raygen-between", "materials-first"])
@pytest.mark.parametrize("fuse,fuse_set,ext_order", [(0, 1, 0), (1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 31, 0), (1, 31, 1), (1, 31, 2)])
def test_fuse_sets_and_extension_orders(fuse, fuse_set, ext_order, raygen_between):
    n = BIG if (fuse_set == 1) == raygen_between else 17 * 256
    _twice(n, {"fuse": fuse, "fuse_set": fuse_set, "ext_order": ext_order}, raygen_between=raygen_between)


@pytest.mark.parametrize("n,ext_order", [(BIG, 2), (17 * 256, 0)])
def test_single_material_queue(n, ext_order):
    seen = _twice(n, {"fuse": 1, "fuse_set": 31, "ext_order": ext_order}, sep=0)
    assert all(int(c[4:8].sum()) == 0 for c, _ in seen)


@pytest.mark.parametrize("n", [257, BIG])
def test_empty_shadow_list(n):
    _twice(n, DEFAULT, lights=False)


@pytest.mark.parametrize("n,fuse", [(BIG, 1), (17 * 256, 0)])
def test_first_iterations_after_reset(n, fuse):
    _twice(n, {"fuse": fuse, "fuse_set": 31, "ext_order": 2}, first_iters=3)


@pytest.mark.parametrize("n", [17 * 256, BIG])
def test_second_logic_appends_behind_non_zero_counters(n):
    seen = _twice(n, {"fuse": 0, "fuse_set": 1, "ext_order": 0}, first_iters=2, relogic=True)
    assert len(seen) == 3
