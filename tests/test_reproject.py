"""flx_reproject's definition (fluctus_amd/csrc/flx_reproject.h) on the CPU: the counterpart tests/reproject_cpu.cpp, which
includes the header, against the float64 restatement of tests/reproject_reference.py on synthetic G-buffers made analytically from quads under
two cameras.  Tolerance: the denoiser's own, 1e-4 relative + 1e-6 absolute on c, n' and the moments, on every pixel where both agree on the
counted taps (reproject_reference.tap_sets); the share of pixels left out for that reason is capped at 0.5 % in EVERY compared case
(run_both).  Measured here: no pixel of any case excluded (0.000 % of 39 449), worst error 0.83 of the tolerance."""
import numpy as np
import pytest
import reproject_reference as R

WALL = R.quad((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 50.0)            # z = 0, seen from z > 0
QUAD = R.quad((0.3, 0.1, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.5, 0.4)              # a foreground rectangle 1 unit in front of it
DIST = 4.0
MAX_EXCLUDED = 0.005    # share of a case's pixels that may be left out of the comparison for a tap-set disagreement


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_cpu(tmp_path_factory.mktemp("reproject"))


def cam_at(x=0.0, y=0.0, z=DIST, fov=60.0, tx=None):
    return R.camera((x, y, z), (x if tx is None else tx, y, 0.0), fov)


def px_step(H, fov=60.0, dist=DIST):
    """world-space width of one pixel on the wall"""
    return 2.0 * np.tan(np.radians(fov) / 2.0) * dist / H


def run_both(exe, W, H, cur, prev, camp, hist, mom, fov_cur=60.0, check=True, **params):
    cpu = R.run_cpu(exe, W, H, cur, prev, camp, fov_cur, hist, mom, **params)
    ref = R.reference(W, H, cur, prev, camp, fov_cur, hist, mom, **params)
    if check:
        worst, share, n = R.compare(cpu, ref)
        print(f"{W} x {H}: worst error {worst:.3f} of the tolerance on {n} pixels, {100 * share:.3f} % excluded")
        assert worst <= 1.0, worst
        assert n > 0
        assert share <= MAX_EXCLUDED, f"{100 * share:.3f} % of the pixels disagree on the counted taps (cap {100 * MAX_EXCLUDED} %)"
    return cpu, ref


@pytest.mark.parametrize("W,H", [(64, 48), (33, 17), (7, 5), (1, 1)])
@pytest.mark.parametrize("moments", [True, False])
def test_identity(exe, W, H, moments):
    """the same camera: every pixel gets its own history back (count capped), at every size down to 1 x 1"""
    c = cam_at()
    g = R.synth_gbuffer(c, W, H, [WALL])
    hist, mom = R.random_history(W * H, 1, moments)
    cpu, _ = run_both(exe, W, H, g, g, c, hist, mom)
    n = np.minimum(hist[:, 3], 32.0)
    assert np.allclose(cpu[0][:, 3], n, rtol=1e-4)
    assert np.allclose(cpu[0][:, :3] / cpu[0][:, 3:4], hist[:, :3] / hist[:, 3:4], rtol=1e-3)
    if moments:
        assert np.allclose(cpu[1][:, 0] / cpu[1][:, 3], mom[:, 0] / mom[:, 3], rtol=1e-3) and (cpu[1][:, 2] == 0).all()
        var = cpu[1][:, 1] / cpu[1][:, 3] - (cpu[1][:, 0] / cpu[1][:, 3]) ** 2
        assert (var >= -1e-5).all()
    else:
        assert not cpu[1].any()


@pytest.mark.parametrize("shift", [3.0, 2.37, -5.5])
def test_pan(exe, shift):
    """the camera slides parallel to the wall by a whole number of pixels and by a fraction: the history slides with it"""
    W, H = 80, 45
    a, b = cam_at(), cam_at(x=shift * px_step(H))
    prev, cur = R.synth_gbuffer(a, W, H, [WALL]), R.synth_gbuffer(b, W, H, [WALL])
    hist, mom = R.random_history(W * H, 2)
    cpu, ref = run_both(exe, W, H, cur, prev, a, hist, mom)
    got = cpu[0].reshape(H, W, 4)
    if shift == 3.0:        # pixel x of the new view sees what pixel x + 3 saw
        h = hist.reshape(H, W, 4)
        assert np.allclose(got[:, :W - 4, :3] / got[:, :W - 4, 3:4], h[:, 3:W - 1, :3] / h[:, 3:W - 1, 3:4], rtol=1e-3)
    off = got[:, :, 3] == 0
    assert off.any() and not off.all()                       # the columns that slid out of the previous frame have no history
    assert (ref[0].reshape(H, W, 4)[:, :, 3][off] == 0).all()


def test_disocclusion_never_mixes_surfaces(exe):
    """a translation with a rectangle in front of the wall: wall pixels the rectangle hid come out with n' = 0, no pixel mixes wall and
    rectangle history (ground truth: the surface each tap lies on)"""
    W, H = 96, 64
    a, b = cam_at(), cam_at(x=0.45, tx=0.1)
    surf = [WALL, QUAD]
    prev, cur = R.synth_gbuffer(a, W, H, surf), R.synth_gbuffer(b, W, H, surf)
    hist, mom = R.random_history(W * H, 3)
    pi, ci = prev[:, 3].copy().view(np.int32), cur[:, 3].copy().view(np.int32)
    hist[pi == 1, :3] = 100.0 * hist[pi == 1, 3:4]            # the rectangle's history is far brighter than the wall's
    cpu, ref = run_both(exe, W, H, cur, prev, a, hist, mom)
    taps, wts = cpu[2], cpu[3]
    counted = taps >= 0
    assert (pi[np.where(counted, taps, 0)][counted] == np.repeat(ci[:, None], 4, 1)[counted]).all(), "a tap from another surface was counted"
    # wall pixels whose four taps all lie on the rectangle in the previous view were hidden then
    _, _, rt, _ = R.reference(W, H, cur, prev, a, 60.0, np.ones_like(hist), None, plane_tolerance_px=1e9, normal_cos=-1.0)
    hidden = (ci == 0) & (rt >= 0).all(1) & (pi[np.where(rt >= 0, rt, 0)] == 1).all(1)
    assert hidden.sum() > 20
    assert (cpu[0][hidden] == 0).all() and (cpu[1][hidden] == 0).all()
    wall = (ci == 0) & (cpu[0][:, 3] > 0)
    assert (cpu[0][wall, :3] / cpu[0][wall, 3:4]).max() < 2.0, "rectangle history leaked onto the wall"


def test_behind_and_outside_the_previous_camera(exe):
    W, H = 40, 30
    b = cam_at()
    cur = R.synth_gbuffer(b, W, H, [WALL])
    hist, mom = R.random_history(W * H, 4)
    behind = R.camera((0.0, 0.0, -1.0), (0.0, 0.0, -5.0))                     # beyond the wall, looking away: z <= 0 for every point
    cpu, _ = run_both(exe, W, H, cur, cur, behind, hist, mom)
    assert not cpu[0].any() and not cpu[1].any()
    far = cam_at(x=300.0 * px_step(H))                                         # every point projects outside the previous frame
    cpu, _ = run_both(exe, W, H, cur, R.synth_gbuffer(far, W, H, [WALL]), far, hist, mom)
    assert not cpu[0].any()
    miss = R.synth_gbuffer(b, W, H, [R.quad((0, 0, 0), (1, 0, 0), (0, 1, 0), 0.5, 0.5)])   # a small rectangle: misses around it
    cpu, _ = run_both(exe, W, H, miss, miss, b, hist, mom)
    mi = miss[:, 3].copy().view(np.int32) < 0
    assert mi.any() and (cpu[0][mi] == 0).all() and (cpu[0][~mi, 3] > 0).any()


def test_normal_test_rejects_a_turned_surface(exe):
    W, H = 32, 24
    c = cam_at()
    g = R.synth_gbuffer(c, W, H, [WALL])
    prev = g.copy()
    turned = np.zeros(W * H, bool); turned[::3] = True
    prev[turned, 4:7] = (np.sin(np.radians(40.0)), 0.0, np.cos(np.radians(40.0)))      # cos 40 deg = 0.766 < 0.9, same position
    hist, mom = R.random_history(W * H, 5)
    cpu, _ = run_both(exe, W, H, g, prev, c, hist, mom)
    assert (cpu[0][turned, 3] == 0).all() and (cpu[0][~turned, 3] > 0).all()
    cpu, _ = run_both(exe, W, H, g, prev, c, hist, mom, normal_cos=0.7)
    assert (cpu[0][:, 3] > 0).all()


def test_bad_history_taps_are_skipped(exe):
    """NaN, +-inf and zero-count history taps, zero and non-finite moments: skipped, the weights renormalise"""
    W, H = 48, 36
    a, b = cam_at(), cam_at(x=1.5 * px_step(H), y=0.5 * px_step(H))
    prev, cur = R.synth_gbuffer(a, W, H, [WALL]), R.synth_gbuffer(b, W, H, [WALL])
    hist, mom = R.random_history(W * H, 6)
    rng = np.random.default_rng(7)
    N = W * H
    hist[rng.choice(N, 60), 0] = np.nan; hist[rng.choice(N, 60), 1] = np.inf; hist[rng.choice(N, 60), 2] = -np.inf
    hist[rng.choice(N, 60), 3] = 0.0; hist[rng.choice(N, 30), 3] = np.inf; hist[rng.choice(N, 30), 3] = -2.0
    mom[rng.choice(N, 60), 3] = 0.0; mom[rng.choice(N, 60), 1] = np.inf; mom[rng.choice(N, 60), 0] = np.nan
    cpu, _ = run_both(exe, W, H, cur, prev, a, hist, mom)
    assert np.isfinite(cpu[0]).all() and np.isfinite(cpu[1]).all()
    assert (cpu[0][:, 3] > 0).mean() > 0.8
    m = cpu[1][:, 3] > 0
    assert m.any() and ((cpu[1][m, 1] / cpu[1][m, 3] - (cpu[1][m, 0] / cpu[1][m, 3]) ** 2) >= -1e-5).all()
    assert ((cpu[0][:, 3] > 0) & ~m).any()                    # a pixel with history whose taps all had empty moments: moments 0


@pytest.mark.parametrize("cap,expect", [(4.0, 4.0), (8.0, 8.0), (16.0, 8.0)])
def test_max_history_below_at_and_above(exe, cap, expect):
    W, H = 24, 16
    a, b = cam_at(), cam_at(x=0.5 * px_step(H))
    prev, cur = R.synth_gbuffer(a, W, H, [WALL]), R.synth_gbuffer(b, W, H, [WALL])
    hist, mom = R.random_history(W * H, 8, lo=8, hi=8)
    cpu, _ = run_both(exe, W, H, cur, prev, a, hist, mom, max_history=cap)
    have = cpu[0][:, 3] > 0
    assert have.any() and np.allclose(cpu[0][have, 3], expect, rtol=1e-5) and np.allclose(cpu[1][have, 3], expect, rtol=1e-5)


def test_rotation_and_fov_change(exe):
    """a general move: translation + rotation + another field of view, two surfaces at an angle"""
    W, H = 101, 67
    floor = R.quad((0.0, -1.0, 2.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 50.0, 50.0)
    a, b = R.camera((0.0, 0.5, 4.0), (0.0, 0.0, 0.0), 60.0), R.camera((0.4, 0.7, 3.6), (0.2, -0.1, 0.0), 50.0)
    surf = [WALL, floor]
    prev, cur = R.synth_gbuffer(a, W, H, surf), R.synth_gbuffer(b, W, H, surf)
    hist, mom = R.random_history(W * H, 9)
    cpu, _ = run_both(exe, W, H, cur, prev, a, hist, mom, fov_cur=50.0)
    assert (cpu[0][:, 3] > 0).mean() > 0.7


def test_min_weight(exe):
    W, H = 16, 12
    a, b = cam_at(), cam_at(x=0.97 * px_step(H))
    prev, cur = R.synth_gbuffer(a, W, H, [WALL]), R.synth_gbuffer(b, W, H, [WALL])
    hist, mom = R.random_history(W * H, 10)
    hist.reshape(H, W, 4)[:, 1::2, 3] = 0.0                  # every other column has no history: alternate pixels keep 3 % or 97 % of the weight
    cpu, _ = run_both(exe, W, H, cur, prev, a, hist, mom, min_weight=0.5)
    n = cpu[0].reshape(H, W, 4)[:, :, 3]
    assert (n > 0).any() and (n == 0).any()
    cpu2, _ = run_both(exe, W, H, cur, prev, a, hist, mom, min_weight=0.01)
    assert (cpu2[0][:, 3] > 0).sum() > (n > 0).sum()
