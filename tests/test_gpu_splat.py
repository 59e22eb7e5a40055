"""The fused logic pass's accumulators (image, luminance moments, the denoiser's normal and albedo features) through flx_splat.h's wave_add4 -- four
adjacent lanes carry the four words of one path's record, 16 records per atomic instruction -- against the oracle, on the wave shapes that can break
it: 64 terminators in a wave (four rounds) with a partial last wave and many paths per pixel, no terminator at all, a mix, a launch bounded by the
pixel count, a dropped component, and the regrouped instance.  Counts are exact, sums within common.fb_close's bound (any order of fp32 additions).
tests/test_splat_inputs.py shows on the CPU that the oracle reproduces itself on these inputs."""
import numpy as np
import pytest
import common
import splat_cases as sc
from common import Q
from fluctus_amd import driver

pytestmark = pytest.mark.gpu


def _pair(case, n, ext=4, denoiser=False, moments=False, **options):
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    d, p, env = case
    g, o = HipContext(n), OracleContext(n, threads=8)
    g.set_option("extend_tree", ext)
    if moments:
        g.set_option("moments", 1)
    sc.setup(g, d, p, env, denoiser=denoiser)
    sc.setup(o, d, p, env, denoiser=denoiser)
    for k, v in options.items():                       # after the upload, which picks its own
        g.set_option(k, v)
    return g, o, int(p["width"]) * int(p["height"])


def _fused_raw(g):
    """the default path: persistent-wave extension kernel leaving RAW hit records, fused logic pass"""
    return g.get_option("extend_tree") == 4 and g.get_option("refill_extend") > 0 and g.get_option("fuse") == 1


@pytest.mark.parametrize("ext", [4, 2], ids=["raw-full-stores", "committed-records"])
@pytest.mark.parametrize("wh", [(4, 4), (3, 3)], ids=["4x4", "3x3"])
def test_every_lane_terminates(wh, ext):
    """1000 paths that all miss and take the environment, on 16 pixels (one round of 16 records is 16 consecutive pixels; ~62 paths per pixel over the
    rounds and waves) and on 9 (the pixels repeat INSIDE every instruction): every wave has 64 terminators, the last one 40 of 40 lanes."""
    n = 1000
    g, o, npix = _pair(sc.sky_case(*wh), n, ext=ext)
    assert _fused_raw(g) == (ext == 4)
    cnts = sc.lockstep_free_run(g, o, npix, 6)
    assert all(int(c[Q.RAYGEN]) == n for c in cnts), "a path did not terminate"
    pg, po = g.read_pixels(0), o.read_pixels(0)
    assert int(po[:, 3].sum()) == 5 * n                # (the first iteration terminates the reset's paths before they were traced: pathLen 0, no splat)
    assert np.array_equal(pg[:, 3], po[:, 3]), "sample counts differ"
    assert common.fb_close(pg, po), np.abs(pg - po).max()
    g.close()


def test_no_lane_terminates():
    """Inside a closed box.  The iteration after the reset terminates every path with pathLen 0 -- a full wave of terminators, none of which may add --
    and the next one finds every path on a wall: nobody terminates.  The framebuffer is never touched."""
    g, o, npix = _pair(sc.box_case(32, 32), 4096)
    before = g.read_pixels(0).copy()
    cnts = sc.lockstep_free_run(g, o, npix, 1)
    assert int(cnts[0][Q.RAYGEN]) == 4096
    assert np.array_equal(g.read_pixels(0).view(np.uint32), before.view(np.uint32))
    cnts = sc.lockstep_free_run(g, o, npix, 1)
    assert int(cnts[0][Q.RAYGEN]) == 0, "the box leaks"
    assert np.array_equal(g.read_pixels(0).view(np.uint32), before.view(np.uint32))
    assert np.array_equal(o.read_pixels(0), before)
    g.close()


def test_mixed():
    """the small kitchen, 4096 paths on 32 x 32 pixels, 2 bounces: terminating and continuing lanes side by side"""
    g, o, npix = _pair(sc.proc_case("kitchen", 32, 32), 4096)
    assert _fused_raw(g)
    cnts = sc.lockstep_free_run(g, o, npix, 2 * 2 + 2)
    assert any(0 < int(c[Q.RAYGEN]) < 4096 for c in cnts)
    assert common.fb_close(g.read_pixels(0), o.read_pixels(0))
    g.close()


def test_mixed_first_launch_bounded_by_the_pixel_count():
    """`first` = 1 with 575 pixels for 4096 paths: the pass runs on paths 0 .. 574 only -- eight full waves and 63 lanes of the ninth"""
    d, p, env = sc.proc_case("kitchen", 25, 23)
    g, o, npix = _pair((d, p, env), 4096)
    cg = driver.first_frame(g, p, npix)
    co = driver.first_frame(o, p, npix)
    assert (cg == co).all()
    assert common.fb_close(g.read_pixels(0), o.read_pixels(0))
    assert int(o.read_pixels(0)[:, 3].sum()) > 0
    g.close()


def test_mixed_with_features_and_moments():
    """options "denoiser" and "moments" on: the normal and albedo accumulators against the oracle's, the moments against their restatement from the
    oracle's state (splat_cases.oracle_iteration); the moments' third word is never written and the fourth is the pixel's sample count"""
    g, o, npix = _pair(sc.proc_case("kitchen", 32, 32), 4096, denoiser=True, moments=True)
    assert _fused_raw(g)
    want = np.zeros((npix, 4), np.float64)
    sc.lockstep_free_run(g, o, npix, 2 * 2 + 2, moments=want)
    pg, po = g.read_pixels(0), o.read_pixels(0)
    assert common.fb_close(pg, po)
    for which, name in ((4, "albedo"), (5, "normal")):
        fg, fo = g.read_pixels(which), o.read_pixels(which)
        assert np.array_equal(fg[:, 3], fo[:, 3]), f"{name}: counts differ"
        assert common.fb_close(fg, fo), (name, np.abs(fg - fo).max())
        assert fo[:, 3].sum() > 0
    mom = g.read_pixels(7)
    assert (mom[:, 2].view(np.uint32) == 0).all(), "the moments' third word was written"
    assert np.array_equal(mom[:, 3], pg[:, 3]) and np.array_equal(mom[:, 3], want[:, 3].astype(np.float32))
    assert common.fb_close(mom, want.astype(np.float32)), np.abs(mom - want).max()
    g.close()


def test_regrouped_instance():
    """the conference room with every BSDF type inlined and 17 x 256 paths: whole blocks, so k_logic<31, true, true> is the pass that runs"""
    g, o, npix = _pair(sc.proc_case("conference", 32, 32), 17 * 256, denoiser=True, moments=True, fuse_set=31, ext_order=1)
    assert _fused_raw(g) and g.get_option("fuse_set_now") == 31 and g.get_option("regroup") == 1
    want = np.zeros((npix, 4), np.float64)
    cnts = sc.lockstep_free_run(g, o, npix, 2 * 2 + 2, moments=want)
    assert any(0 < int(c[Q.RAYGEN]) < 17 * 256 for c in cnts)
    assert common.fb_close(g.read_pixels(0), o.read_pixels(0))
    for which in (4, 5):
        assert common.fb_close(g.read_pixels(which), o.read_pixels(which)), which
    mom = g.read_pixels(7)
    assert (mom[:, 2].view(np.uint32) == 0).all() and common.fb_close(mom, want.astype(np.float32))
    g.close()
