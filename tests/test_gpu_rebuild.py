"""Tracer::setRebuildPolicy on the device (host/tracer.cpp, host/rebuild_job.hpp): when the trees are rebuilt, and that a
rebuilt-then-refitted Tracer holds exactly the trees a fresh upload of the same build would.

The scene is the 3000-triangle procedural kitchen.  Poses: P1 = every triangle thrown about by up to the scene's extent (tests/refit_cases.py:
scramble -- the topology of the rest pose is then worthless, cost ratio far above the threshold of 2); P2 / P3 = P1 under a sine field of 1 % of the
extent (two phases): a tree built for P1 stays well below the threshold at them, which every test that relies on it asserts first.
The reference for the trees is a fresh C-ABI context: upload(build_bvh(pose)) [+ update_triangles(later pose)], all five tree_read arrays byte for
byte -- a refit has no history (tests/test_gpu_refit.py), so how many refits lie between does not show.
Background jobs are HELD (Tracer.hold_rebuild) until wait_for_rebuild: between which two calls a job completes is then the test's decision, not
the scheduler's, and nothing sleeps.
"""
import copy
import math
import numpy as np
import pytest
import refit_cases as rc
from fluctus_amd import host
from fluctus_amd.tracer import Tracer

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENE = ("kitchen", 3000, 7)
THRESHOLD = 2.0


@pytest.fixture(scope="module")
def poses():
    d = host.generate_scene(*SCENE)
    P0 = np.stack([np.stack([d.tris[v]["p"][k] for k in "xyz"], -1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)
    P1 = rc.deform(P0, "scramble")
    lo, hi = P1.min((0, 1)), P1.max((0, 1))
    ext = float((hi - lo).max())

    def gentle(phase):
        u = (P1 - lo) / ext
        return P1 + 0.01 * ext * np.stack([np.sin(5.0 * u[..., 1] + phase), np.sin(4.0 * u[..., 2] + 2.0 * phase), np.sin(6.0 * u[..., 0] + 3.0 * phase)], -1)

    def scene(P):
        m = copy.copy(d)
        m.tris = d.tris.copy()
        for i, v in enumerate(("v0", "v1", "v2")):
            for j, k in enumerate("xyz"):
                m.tris[v]["p"][k] = np.float32(P[:, i, j])
        return m

    return dict(P0=d, P1=scene(P1), P2=scene(gentle(1.0)), P3=scene(gentle(2.0)))


def _tracer(device=0):
    t = Tracer(W, H, device, W * H)
    t.init(W, H, "proc:%s:%d:%d" % SCENE)
    return t


def _trees(t, rank=0):
    return [t.tree_read(w, rank).tobytes() for w in range(5)]


def _fresh(built_for, then=None):
    """the five arrays of a fresh context: upload(build_bvh(built_for)) [+ update_triangles(then)]"""
    from fluctus_amd.device import HipContext
    g = HipContext(256)
    try:
        d = copy.copy(built_for)
        host.build_bvh(d, "sbvh")
        g.upload_scene(d)
        if then is not None:
            g.update_triangles(then)
        return [g.tree_read(w).tobytes() for w in range(5)]
    finally:
        g.close()


def _same(got, want, what):
    for w, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{what}: tree array {w} differs from the fresh context's"


def test_the_tracers_scene_is_the_poses_rest_scene(poses):
    t = _tracer()
    try:
        assert t.triangles().tobytes() == poses["P0"].tris.tobytes()
        _same(_trees(t), _fresh(poses["P0"]), "after init")
        assert math.isnan(t.last_cost_ratio) and t.rebuild_count == 0 and not t.rebuild_pending
        with pytest.raises(RuntimeError, match="threshold must be finite and > 1"):
            t.set_rebuild_policy("blocking", 1.0)
        with pytest.raises(RuntimeError, match="threshold must be finite and > 1"):
            t.set_rebuild_policy("background", float("nan"))
        with pytest.raises(ValueError, match="threshold is required"):
            t.set_rebuild_policy("background")
    finally:
        t.close()


def test_off_only_refits(poses):
    t = _tracer()
    try:
        t.set_rebuild_policy("off")
        t.update_geometry(poses["P1"].tris)
        _same(_trees(t), _fresh(poses["P0"], poses["P1"]), "off / scramble")
        assert t.rebuild_count == 0 and not t.rebuild_pending and math.isnan(t.last_cost_ratio)
    finally:
        t.close()


def test_blocking_rebuilds_inside_the_call_and_refits_below_the_threshold(poses):
    t = _tracer()
    try:
        t.set_rebuild_policy("blocking", THRESHOLD)
        t.update_geometry(poses["P1"].tris)
        assert t.rebuild_count == 1 and not t.rebuild_pending
        _same(_trees(t), _fresh(poses["P1"]), "blocking / scramble")
        assert t.last_cost_ratio == 1.0
        fresh_cost = t.tree_cost()
        t.update_geometry(poses["P2"].tris)
        print(f"cost ratio of the tree built for P1 at P2: {t.last_cost_ratio:.4f}")
        assert 1.0 <= t.last_cost_ratio < THRESHOLD, "P2 is not below the threshold: the test does not reach the refit-only branch"
        assert t.rebuild_count == 1
        _same(_trees(t), _fresh(poses["P1"], poses["P2"]), "blocking / gentle")
        assert t.tree_cost() != fresh_cost
    finally:
        t.close()


def _background_to_p3(t, poses, what):
    """P1 starts a (held) job, P2 only refits while it is in flight, the update to P3 swaps"""
    t.hold_rebuild(True)
    t.set_rebuild_policy("background", THRESHOLD)
    t.update_geometry(poses["P1"].tris)
    print(f"{what}: cost ratio of the rest pose's tree at P1: {t.last_cost_ratio:.3f}")
    assert t.last_cost_ratio > THRESHOLD and t.rebuild_pending and t.rebuild_count == 0
    t.update_geometry(poses["P2"].tris)
    assert t.rebuild_pending and t.rebuild_count == 0, "a second job, or a swap, while the first is in flight"
    return t


def test_background_swaps_at_the_next_update_geometry_and_renders_like_blocking(poses):
    t, b = _tracer(), _tracer()
    try:
        _background_to_p3(t, poses, "background")
        _same(_trees(t), _fresh(poses["P0"], poses["P2"]), "background / in flight")
        t.wait_for_rebuild()
        assert t.rebuild_pending and t.rebuild_count == 0, "wait_for_rebuild swapped something"
        _same(_trees(t), _fresh(poses["P0"], poses["P2"]), "background / after the wait")
        t.update_geometry(poses["P3"].tris)
        assert t.rebuild_count == 1 and not t.rebuild_pending
        assert 1.0 <= t.last_cost_ratio < THRESHOLD, "the ratio after the swap is against the NEW tree's baseline"
        _same(_trees(t), _fresh(poses["P1"], poses["P3"]), "background / swapped")
        b.set_rebuild_policy("blocking", THRESHOLD)
        b.update_geometry(poses["P1"].tris); b.update_geometry(poses["P3"].tris)
        assert b.rebuild_count == 1
        assert b.last_cost_ratio == t.last_cost_ratio
        _same(_trees(t), _trees(b), "background vs blocking")
        t.render_single(4); b.render_single(4)
        pt, pb = t.read_pixels(0), b.read_pixels(0)
        assert pt[:, 3].min() == 4.0 and pt[:, :3].sum() > 0
        assert pt.tobytes() == pb.tobytes(), f"{int((pt != pb).any(1).sum())} pixels differ between the background and the blocking Tracer"
    finally:
        t.close(); b.close()


def _write_hdr(path, w=16, h=8):
    """a small Radiance picture in flat (not run-length) scanlines: a gradient with one bright texel"""
    px = np.zeros((h, w, 4), np.uint8)
    px[..., 0] = 40 + 8 * np.arange(w)[None, :]
    px[..., 1] = 60 + 10 * np.arange(h)[:, None]
    px[..., 2] = 90
    px[..., 3] = 128
    px[2, 5] = (255, 240, 200, 134)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
        f.write(px.tobytes())


def test_background_swap_in_update_keeps_the_environment_map(poses, tmp_path):
    hdr = str(tmp_path / "sky.hdr")
    _write_hdr(hdr)
    t, b, plain = _tracer(), _tracer(), _tracer()
    try:
        t.set_envmap(hdr); b.set_envmap(hdr)
        _background_to_p3(t, poses, "background + env map")
        t.wait_for_rebuild()
        t.update()                                                           # the finished job is picked up here
        assert t.rebuild_count == 1 and not t.rebuild_pending
        _same(_trees(t), _fresh(poses["P1"], poses["P2"]), "background / swapped in update()")
        assert int(t.params["useEnvMap"]) == 1
        b.set_rebuild_policy("blocking", THRESHOLD)
        b.update_geometry(poses["P1"].tris); b.update_geometry(poses["P2"].tris)
        assert b.rebuild_count == 1
        b.update()
        plain.set_rebuild_policy("blocking", THRESHOLD)
        plain.update_geometry(poses["P1"].tris); plain.update_geometry(poses["P2"].tris)
        for x in (t, b, plain):
            x.render_single(4)
        pt, pb, pp = t.read_pixels(0), b.read_pixels(0), plain.read_pixels(0)
        assert pt.tobytes() == pb.tobytes(), f"{int((pt != pb).any(1).sum())} pixels differ between the background and the blocking Tracer"
        assert pt.tobytes() != pp.tobytes(), "the environment map does not show in the image: the test does not see whether it survived"
    finally:
        t.close(); b.close(); plain.close()


def test_swap_keeps_the_first_uploads_options_and_skips_the_refit_when_nothing_moved(poses):
    """flx_upload_scene re-derives fuse_set / ext_order from the triangles it is given (the kitchen is mostly diffuse: 1 and 2); values set by
    the caller before P1 must come back after the swap.  The job is adopted in update() directly after P1: nothing moved since the snapshot, so no
    refit follows the upload and the trees are the fresh upload's."""
    t = _tracer()
    try:
        assert (t.get_option("fuse_set"), t.get_option("ext_order")) == (1, 2), "the upload's own choice changed: pick other values below"
        t.set_option("fuse_set", 31); t.set_option("ext_order", 0)
        t.hold_rebuild(True)
        t.set_rebuild_policy("background", THRESHOLD)
        t.update_geometry(poses["P1"].tris)
        assert t.rebuild_pending
        t.wait_for_rebuild()
        t.update()
        assert t.rebuild_count == 1 and not t.rebuild_pending
        assert (t.get_option("fuse_set"), t.get_option("ext_order")) == (31, 0)
        _same(_trees(t), _fresh(poses["P1"]), "adopted with nothing moved")
        b = _tracer()
        try:
            b.set_option("fuse_set", 31); b.set_option("ext_order", 0)
            b.set_rebuild_policy("blocking", THRESHOLD)
            b.update_geometry(poses["P1"].tris)
            assert b.rebuild_count == 1 and (b.get_option("fuse_set"), b.get_option("ext_order")) == (31, 0)
        finally:
            b.close()
    finally:
        t.close()


def test_a_job_that_outlives_a_switch_to_off_is_refitted_when_adopted(poses):
    t = _tracer()
    try:
        t.hold_rebuild(True)
        t.set_rebuild_policy("background", THRESHOLD)
        t.update_geometry(poses["P1"].tris)
        assert t.rebuild_pending
        t.set_rebuild_policy("off")
        t.update_geometry(poses["P2"].tris)                                  # under Off: only refits, but the job's snapshot is now stale
        t.wait_for_rebuild()
        t.update()
        assert t.rebuild_pending and t.rebuild_count == 0, "Off adopted a job"
        _same(_trees(t), _fresh(poses["P0"], poses["P2"]), "off / job pending")
        t.set_rebuild_policy("background", THRESHOLD)
        t.update()
        assert t.rebuild_count == 1 and not t.rebuild_pending
        _same(_trees(t), _fresh(poses["P1"], poses["P2"]), "adopted after Off")
        assert t.triangles().tobytes() == poses["P2"].tris.tobytes()
    finally:
        t.close()


def test_init_discards_a_job_in_flight(poses):
    t = _tracer()
    try:
        t.hold_rebuild(True)
        t.set_rebuild_policy("background", THRESHOLD)
        t.update_geometry(poses["P1"].tris)
        assert t.rebuild_pending
        t.init(W, H, "proc:%s:%d:%d" % SCENE)
        assert not t.rebuild_pending and t.rebuild_count == 0 and math.isnan(t.last_cost_ratio)
        _same(_trees(t), _fresh(poses["P0"]), "after init")
        t.update()                                                           # nothing to pick up
        assert t.rebuild_count == 0
    finally:
        t.close()


def test_multi_rank_tracer_swaps_every_rank(poses):
    t = _tracer([0, 0])
    try:
        assert t.num_ranks == 2
        _background_to_p3(t, poses, "two ranks")
        t.wait_for_rebuild()
        t.update_geometry(poses["P3"].tris)
        assert t.rebuild_count == 1
        want = _fresh(poses["P1"], poses["P3"])
        for rank in range(2):
            _same(_trees(t, rank), want, f"rank {rank}")
        t.update()
        assert t.read_accumulation()[:, 3].sum() > 0
    finally:
        t.close()
