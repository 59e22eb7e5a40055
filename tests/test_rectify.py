"""History rectification without a GPU: tests/rectify_cpu.cpp -- csrc/flx_rectify.h over a whole image, the functions the
kernels of csrc/rectify.hip run -- against the float64 restatement of tests/rectify_reference.py on the analytic inputs of
tests/rectify_cases.py, the pixels that must stay bit for bit, and the statistical behaviour on the prototype's plane.

Tolerance 1e-4 relative + 1e-6 absolute on lambda and A' (S' and the moments: rectify_reference.compare says what lambda's tolerance means for
them), over the pixels where counterpart and restatement agree on the counted taps and on which side of e > 0 they stand; at most 0.5 % of a
case's pixels may be excluded (asserted per case)."""
import numpy as np
import pytest
import rectify_cases as K
import rectify_reference as RC

CAP = 0.005


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return RC.build_cpu(tmp_path_factory.mktemp("rectify"))


def _both(exe, W, H, s, **kw):
    args = (W, H, s["cur"], s["A"], s["S"], K.FOV, s.get("M"), s.get("SM"))
    return RC.run_cpu(exe, *args, **kw), RC.reference(*args, **kw)


def _check(exe, W, H, s, **kw):
    """the comparison every case ends in; -> (counterpart, restatement)"""
    cpu, ref = _both(exe, W, H, s, **kw)
    worst, excluded = RC.compare(cpu, ref, s["S"], s.get("SM") if s.get("M") is not None else None)
    assert excluded <= CAP, excluded
    assert worst <= 1.0, worst
    keep = ~(cpu["lam"] > 0)                                    # lambda = 0 (a NaN would land here too): not written
    assert not np.isnan(cpu["lam"]).any() and (cpu["lam"] >= 0).all() and (cpu["lam"] <= 1).all()
    assert RC.same(cpu["A"][keep], s["A"][keep]) and RC.same(cpu["S"][keep], s["S"][keep])
    if s.get("M") is not None and s.get("SM") is not None:
        assert RC.same(cpu["M"][keep], s["M"][keep]) and RC.same(cpu["SM"][keep], s["SM"][keep])
    return cpu, ref


NONDEFAULT = dict(radius=2, gamma=1.5, sensitivity=0.7, lum_floor=0.2, min_pixels=3, plane_tolerance_px=0.5, normal_cos=0.5)


@pytest.mark.parametrize("kw", [{}, dict(radius=1, min_pixels=4), dict(radius=4, min_pixels=20), NONDEFAULT], ids=["defaults", "r1", "r4", "nondefault"])
@pytest.mark.parametrize("W,H", [(48, 32), (33, 17)])
def test_counterpart_equals_the_restatement(exe, W, H, kw):
    s = K.scene(W, H, W + H)
    cpu, ref = _check(exe, W, H, s, **kw)
    idx, lam = s["idx"], cpu["lam"]
    assert (lam[idx < 0] == 0).all(), "a pixel that misses the scene has a lambda"
    assert (lam[idx == 1] > 0.3).mean() > 0.6, "the changed rectangle keeps its history"
    if "gamma" not in kw:
        assert (lam[idx == 0] == 0).mean() > 0.98, "the unchanged wall loses history"
    # the restatement alone says the inputs stay inside the cap: the windows so close to the threshold that fp32 may stand on the other side
    # of e > 0 (|d| and gamma se are O(1) sums of <= 81 terms: 1e-5 is some thirty times their fp32 error) are fewer than the cap allows
    m = ref["margin"]
    assert (np.abs(m[np.isfinite(m)]) < 1e-5).sum() <= CAP * W * H
    # no tap crosses the two surfaces, nor a turned normal: never more taps than pixels of the centre's own surface in the window
    r = int(dict(RC.DEFAULTS, **kw)["radius"])
    assert (cpu["counted"] <= K.same_surface_count(W, H, idx, r)).all()


def test_clean_input_counts_the_whole_surface_and_no_tap_crosses(exe):
    """without adversarial records every pixel of the centre's surface in the window counts and no other: the rectangle in front of the wall"""
    W, H = 48, 32
    s = K.scene(W, H, 3, adversarial=False)
    for r in (1, 3, 4):
        cpu, _ = _check(exe, W, H, s, radius=r, min_pixels=1)
        assert np.array_equal(cpu["counted"], K.same_surface_count(W, H, s["idx"], r))
    assert set(np.unique(s["idx"])) == {-1, 0, 1}


def test_a_centre_that_is_no_tap_itself_is_decided_by_its_neighbours(exe):
    """no new sample at the centre (its own ok is false): its window still speaks, and the pixel sheds history like its neighbours"""
    W, H = 24, 16
    s = K.scene(W, H, 23, adversarial=False, wide=True, factor=1.0)
    s["A"][:, :3] = s["S"][:, :3] + 0.3 * (s["A"][:, :3] - s["S"][:, :3])
    j = (H // 2) * W + W // 2
    s["A"][j] = s["S"][j]; s["M"][j] = s["SM"][j]
    cpu, _ = _check(exe, W, H, s)
    assert cpu["counted"][j] == 48 and cpu["counted"][j + 1] == 48 and cpu["lam"][j] > 0.5
    assert cpu["A"][j, 3] == np.float32(32.0) - np.float32(cpu["lam"][j]) * np.float32(32.0)


def test_turned_normal_is_no_tap_and_keeps_its_history(exe):
    W, H = 24, 16
    s = K.scene(W, H, 5, adversarial=False, wide=True, factor=1.0)
    j = (H // 2) * W + W // 2
    s["cur"][j, 4:7] = (0.6, 0.0, 0.8)
    s["A"][:, :3] = s["S"][:, :3] + 0.3 * (s["A"][:, :3] - s["S"][:, :3])       # the whole image changed
    cpu, _ = _check(exe, W, H, s)
    full = K.same_surface_count(W, H, s["idx"], 3)
    assert cpu["counted"][j] == 1 and cpu["lam"][j] == 0                         # alone with itself: N < min_pixels
    assert cpu["counted"][j + 1] == full[j + 1] - 1 and cpu["lam"][j + 1] > 0


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (7, 5), (5, 40)])
def test_images_smaller_than_the_window_and_clipped_windows(exe, W, H):
    """a wall that reaches all four image edges: the window is clipped by each of them, and by all at once in an image smaller than it"""
    s = K.scene(W, H, 7, adversarial=False, wide=True, factor=1.0, rect=False)
    s["A"][:, :3] = s["S"][:, :3] + 0.3 * (s["A"][:, :3] - s["S"][:, :3])
    for r in (1, 4):
        cpu, _ = _check(exe, W, H, s, radius=r, min_pixels=1)
        x, y = np.arange(W * H) % W, np.arange(W * H) // W
        inside = (np.minimum(x, r) + np.minimum(W - 1 - x, r) + 1) * (np.minimum(y, r) + np.minimum(H - 1 - y, r) + 1)
        surf = s["idx"] >= 0
        assert surf.all() and np.array_equal(cpu["counted"], inside)
        assert (cpu["lam"] > 0).all()


def test_lambda_zero_cases_keep_every_bit(exe):
    W, H = 33, 17
    s = K.scene(W, H, 11)
    # no new samples anywhere
    t = dict(s, A=s["S"].copy(), M=s["SM"].copy())
    cpu, _ = _check(exe, W, H, t)
    assert (cpu["lam"] == 0).all() and (cpu["counted"] == 0).all() and RC.same(cpu["A"], t["A"]) and RC.same(cpu["M"], t["M"])
    # N < min_pixels everywhere: the largest window of r = 1 has 9 pixels, one pixel in 40 has no new sample
    cpu, _ = _check(exe, W, H, s, radius=1, min_pixels=9)
    few = cpu["counted"] < 9
    assert few.any() and (cpu["lam"][few] == 0).all() and RC.same(cpu["A"][few], s["A"][few])
    cpu, _ = _check(exe, 3, 2, K.scene(3, 2, 1, wide=True, adversarial=False), min_pixels=8)
    assert (cpu["lam"] == 0).all()
    # a miss centre, NaN / +-inf / zero-count records: lambda 0 at the centre, bits kept (the comparison in _check), and such a record is no tap
    cpu, _ = _check(exe, W, H, s)
    bad = ~np.isfinite(s["A"]).all(1) | ~np.isfinite(s["S"]).all(1) | ~(s["S"][:, 3] > 0) | (s["idx"] < 0)
    assert bad.sum() > 20 and (cpu["lam"][bad] == 0).all()


def test_lambda_is_clamped_at_one_and_leaves_the_new_samples(exe):
    W, H = 24, 16
    s = K.scene(W, H, 13, factor=0.05, adversarial=False)
    cpu, _ = _check(exe, W, H, s, sensitivity=10.0)
    one = cpu["lam"] == 1
    assert one.sum() > 20 and (cpu["lam"] <= 1).all()
    new = s["A"].astype(np.float64) - s["S"]
    assert np.allclose(cpu["A"][one], new[one], rtol=1e-6, atol=1e-5) and not cpu["S"][one].any()


@pytest.mark.parametrize("mode", ["on", "off", "mark_only", "now_only"])
def test_moments(exe, mode):
    W, H = 33, 17
    s = K.scene(W, H, 17)
    t = dict(s, M=s["M"] if mode in ("on", "now_only") else None, SM=s["SM"] if mode in ("on", "mark_only") else None)
    cpu, ref = _check(exe, W, H, t)
    base = RC.run_cpu(exe, W, H, s["cur"], s["A"], s["S"], K.FOV)
    assert RC.same(cpu["lam"], base["lam"]) and RC.same(cpu["A"], base["A"]) and RC.same(cpu["S"], base["S"])     # the moments decide nothing
    w = cpu["lam"] > 0
    if mode == "on":
        assert not RC.same(cpu["M"][w], s["M"][w]) and not RC.same(cpu["SM"][w], s["SM"][w])
    for key in ("M", "SM"):
        if mode != "on" and t[key] is not None:
            assert RC.same(cpu[key], t[key]), "moments that are on at one end only are left alone"


def test_new_samples_survive_one_and_two_calls(exe):
    """A' - S' = A - S within rounding: the call may be repeated; with nothing new between two calls the second finds the same evidence against
    a smaller history"""
    W, H = 48, 32
    s = K.scene(W, H, 19, adversarial=False)
    new = s["A"].astype(np.float64) - s["S"]
    one, _ = _check(exe, W, H, s, sensitivity=0.5)
    two, _ = _check(exe, W, H, dict(s, A=one["A"], S=one["S"], M=one["M"], SM=one["SM"]), sensitivity=0.5)
    for out in (one, two):
        got = out["A"].astype(np.float64) - out["S"]
        # each call rounds A' and S' once: half an ulp of the larger of the two operands each
        bound = 2.0 * 2.0 ** -24 * np.maximum(np.abs(s["A"]), np.abs(s["S"])) * 2 + 1e-12
        assert (np.abs(got - new) <= bound).all(), float((np.abs(got - new) / bound).max())
    w = one["lam"] > 0
    left = w & (one["S"][:, 3] > 0)
    assert left.any() and (two["S"][left, 3] < one["S"][left, 3]).all() and (one["S"][w, 3] < s["S"][w, 3]).all()


def test_bad_parameters_are_refused(exe):
    s = K.scene(7, 5, 1)
    for bad in (dict(radius=0), dict(radius=5), dict(gamma=-1.0), dict(gamma=np.inf), dict(gamma=np.nan), dict(sensitivity=0.0), dict(sensitivity=np.inf),
                dict(lum_floor=-0.1), dict(lum_floor=np.nan), dict(min_pixels=0), dict(min_pixels=50), dict(radius=1, min_pixels=10),
                dict(plane_tolerance_px=0.0), dict(plane_tolerance_px=np.nan), dict(normal_cos=1.5), dict(normal_cos=np.nan)):
        RC.run_cpu(exe, 7, 5, s["cur"], s["A"], s["S"], K.FOV, expect_refused=True, **bad)
    assert RC.run_cpu(exe, 7, 5, s["cur"], s["A"], s["S"], K.FOV, radius=4, min_pixels=81, gamma=0.0, lum_floor=0.0, normal_cos=-1.0) is not None


def test_statistical_case_on_the_prototypes_plane(exe):
    """64 x 48 plane, history 32 spp of mean 1, one new sample uniform in [0, 2 mean] on four pixels in five, the right half's mean dropped to
    0.3, gamma 3, sensitivity 1, fixed seed; both halves without the three columns next to the boundary.  Unchanged half: mean lambda <= 0.02;
    changed half: mean lambda >= 0.45 (ceiling 0.7 / 1.01 = 0.69).  Confirmed with the restatement first, then asserted of the counterpart."""
    W, H = 64, 48
    s = K.statistical(20260101)
    x = np.arange(W * H) % W
    left, right = x < W // 2 - 3, x >= W // 2 + 3
    for out in (RC.reference(W, H, s["cur"], s["A"], s["S"], K.FOV, gamma=3.0, sensitivity=1.0),
                RC.run_cpu(exe, W, H, s["cur"], s["A"], s["S"], K.FOV, gamma=3.0, sensitivity=1.0)):
        lo, hi = float(out["lam"][left].mean()), float(out["lam"][right].mean())
        print(f"statistical case: mean lambda unchanged half {lo:.5f} ({100 * (out['lam'][left] > 0).mean():.2f} % of it > 0), changed half {hi:.4f}")
        assert lo <= 0.02, lo
        assert hi >= 0.45, hi
