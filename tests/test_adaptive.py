"""The stopping rule of the adaptive microkernel render (fluctus_amd/csrc/flx_adaptive.h) on the CPU: the counterpart
tests/adaptive_cpu.cpp, which includes the header, against the float64 restatement of tests/adaptive_reference.py; the end state of an adaptive
run on a synthetic sampler; and the adaptive render simulated from the oracle's per-sample microkernel images, where the defaults were swept
and where tests/test_gpu_adaptive.py's expected image comes from.

Tolerances: r within 1e-5 relative + 1e-7 absolute of float64 (float32 rounding of five operations; measured worst 0.2 of it); flags and the
list EQUAL on every pixel whose float64 r is not within that tolerance of the threshold; the pixels left out are capped at 0.5 % per case."""
import os
import shutil
import numpy as np
import pytest
import adaptive_reference as A

MAX_EXCLUDED = 0.005
HEADER = os.path.join(A.ROOT, "fluctus_amd", "csrc", "flx_adaptive.h")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return A.build_cpu(tmp_path_factory.mktemp("adaptive"))


def synthetic_moments(W, H, seed, min_samples=4, max_samples=32, threshold=0.05, lum_floor=0.01, adversarial=True):
    """moments of n samples of a per-pixel distribution: n of 0, 1, min, max and between, zero variance, and (adversarial) NaN / +-inf /
    overflowed sums and S2 < S1^2 / n by rounding.  Pixels whose float64 r falls within the comparison tolerance of the threshold are nudged away
    (S2 scaled), so that the float64 reference alone stays inside the cap.
    What float32 allows: v comes from S2 / n - mu^2, a difference of two numbers of size mu^2 that carry a rounding error of about 2^-23 mu^2
    between them, so its RELATIVE error is 2^-23 / rel^2 (rel = the samples' relative standard deviation) and r's half of that.  The 1e-5 tolerance
    therefore holds from rel = 0.2 upwards (3e-6) -- the spread drawn here, which puts r = rel / sqrt(n) on both sides of every threshold used --
    and on zero variance where the sums are exact (powers of two).  Below that r is rounding noise of at most 3.5e-4 / sqrt(n), two decades under
    any useful threshold."""
    rng = np.random.default_rng(seed)
    N = W * H
    n = rng.choice([0, 1, 2, 3, min_samples - 1, min_samples, min_samples + 1, max_samples - 1, max_samples, max_samples + 5, 7, 16], N).astype(np.float32)
    mu = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), N))
    rel = np.exp(rng.uniform(np.log(0.2), np.log(3.0), N))                  # the sample's relative standard deviation
    zero = rng.random(N) < 0.15                                             # zero variance, exactly: a power of two, n times
    mu[zero] = 2.0 ** rng.integers(-6, 4, zero.sum())
    rel[zero] = 0.0
    s1 = mu * n
    s2 = (mu * mu * (1.0 + rel * rel)) * n
    mom = np.stack([s1, s2, np.zeros(N), n], 1).astype(np.float32)
    k = rng.random(N) < 0.05
    mom[k, 1] = (mom[k, 0] * mom[k, 0] / np.maximum(mom[k, 3], 1)) * np.float32(1 - 2e-6)      # S2 < S1^2 / n, as rounding leaves it: the variance clamps to 0
    if adversarial:
        for col, val in ((0, np.nan), (1, np.nan), (0, np.inf), (1, np.inf), (0, -np.inf), (3, np.nan), (3, np.inf), (1, 3e38), (0, 3e38), (0, -1.0)):
            mom[rng.random(N) < 0.01, col] = val
    for _ in range(4):
        near = A.reference(W, H, mom, threshold=threshold, min_samples=min_samples, max_samples=max_samples, lum_floor=lum_floor, dilate=0)[3]
        if not near.any():
            break
        mom[near, 1] *= np.float32(1.01)
    return mom


SIZES = [(1, 1), (1, 7), (5, 1), (3, 3), (7, 5), (33, 17), (80, 60), (257, 129)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("dilate", [0, 1])
def test_counterpart_vs_float64(exe, W, H, dilate):
    worst_all = 0.0
    for seed, kw in ((1, {}), (2, dict(threshold=0.2, min_samples=2, max_samples=8)), (3, dict(threshold=0.0, lum_floor=0.0)), (4, dict(min_samples=1, max_samples=1))):
        P = dict(A.DEFAULTS, **kw, dilate=dilate)
        mom = synthetic_moments(W, H, seed * 100 + W, P["min_samples"], P["max_samples"], P["threshold"], P["lum_floor"])
        cpu, ref = A.run_cpu(exe, W, H, mom, **P), A.reference(W, H, mom, **P)
        worst, share = A.compare(cpu, ref, MAX_EXCLUDED)
        print(f"{W} x {H} dilate {dilate} {kw}: worst r error {worst:.3f} of the tolerance, {100 * share:.3f} % excluded, {cpu[2].size} active")
        assert worst <= 1.0, worst
        worst_all = max(worst_all, worst)
        bad = ~np.isfinite(mom).all(1)
        assert not (cpu[0][bad] & A.CONVERGED).any(), "a pixel with a NaN or a non-finite sum converged"


def test_flag_semantics_by_hand(exe):
    """hand-made records at 5 x 3: every clause of the definition once"""
    W, H = 5, 3
    flat = [8.0, 8.0, 0.0, 8.0]                                  # zero variance, n = 8: converged
    mom = np.tile(np.array(flat, np.float32), (W * H, 1))
    noisy = [8.0, 80.0, 0.0, 8.0]                                 # mu 1, sample variance 9 -> r = sqrt(9 / 8) / 1.01 > 0.05
    mom[7] = noisy                                                # the centre
    f, r, lst = A.run_cpu(exe, W, H, mom, dilate=0)
    assert list(lst) == [7] and f[7] == A.OWN | A.ACTIVE and f[0] == A.CONVERGED
    assert abs(r[7] - np.sqrt(9.0 / 8.0) / 1.01) < 1e-6 and r[0] == 0.0
    f, r, lst = A.run_cpu(exe, W, H, mom, dilate=1)
    assert list(lst) == [1, 2, 3, 6, 7, 8, 11, 12, 13] and f[1] == A.CONVERGED | A.ACTIVE and f[4] == A.CONVERGED
    mom[6] = [32.0, 32.0, 0.0, 32.0]                              # a done neighbour is never active
    f, r, lst = A.run_cpu(exe, W, H, mom, dilate=1)
    assert 6 not in lst and f[6] & A.DONE
    mom[7] = [40.0, 400.0, 0.0, 32.0]                             # n = max: done although noisy ("<" vs "<=")
    f, r, lst = A.run_cpu(exe, W, H, mom, dilate=1)
    assert lst.size == 0 and f[7] == A.DONE
    mom[7] = [31.0, 310.0, 0.0, 31.0]                             # n = max - 1: still sampled
    assert list(A.run_cpu(exe, W, H, mom, dilate=0)[2]) == [7]
    mom[:] = flat; mom[0] = [3.0, 3.0, 0.0, 3.0]                  # n < min_samples: own whatever the variance
    mom[14] = [1.0, 1.0, 0.0, 1.0]
    f, r, lst = A.run_cpu(exe, W, H, mom, dilate=0, min_samples=4)
    assert list(lst) == [0, 14]
    f, r, lst = A.run_cpu(exe, W, H, mom, dilate=0, min_samples=1)      # n >= 2 is required whatever min_samples says
    assert list(lst) == [14]
    mom[:] = flat; mom[3] = [0.0, 0.0, 0.0, 8.0]                  # a black pixel converges through lum_floor ...
    assert A.run_cpu(exe, W, H, mom, dilate=0)[2].size == 0
    assert list(A.run_cpu(exe, W, H, mom, dilate=0, lum_floor=0.0)[2]) == [3]      # ... and never without it
    for bad in ([np.nan, 8.0, 0.0, 8.0], [8.0, np.nan, 0.0, 8.0], [np.inf, 8.0, 0.0, 8.0], [8.0, np.inf, 0.0, 8.0], [-np.inf, 1.0, 0.0, 8.0]):
        mom[:] = flat; mom[9] = bad
        f, r, lst = A.run_cpu(exe, W, H, mom, dilate=0)
        assert list(lst) == [9] and not f[9] & A.CONVERGED, bad


def test_the_copies_of_the_defaults_agree():
    """FLX_AD_DEFAULT_* (csrc/flx_adaptive.h) is the one definition; the Python mirrors and the C header's comment restate it (the C++ mirror
    uses the macros themselves)"""
    import re
    from fluctus_amd import device
    txt = open(HEADER).read()
    m = {k.lower(): float(v.rstrip("fu")) for k, v in re.findall(r"#define FLX_AD_DEFAULT_(\w+) ([0-9.]+[fu]?)", txt)}
    assert set(m) == set(A.DEFAULTS) == set(device.ADAPTIVE_DEFAULTS)
    for k, v in m.items():
        assert float(A.DEFAULTS[k]) == v and float(device.ADAPTIVE_DEFAULTS[k]) == v, k
    abi = open(os.path.join(A.ROOT, "include", "fluctus_hip.h")).read()
    quoted = "{%g, %d, %d, %g, %d}" % (m["threshold"], m["min_samples"], m["max_samples"], m["lum_floor"], m["dilate"])
    assert quoted in abi, quoted
    assert [f[0] for f in device.AdaptiveParams._fields_] == ["threshold", "min_samples", "max_samples", "lum_floor", "dilate"]


def table_sampler(W, H, S, seed=5):
    """left half: the constant 0.5; right half: a fixed table of noisy values -> (S, N, 3) float32 radiance (grey)"""
    rng = np.random.default_rng(seed)
    v = np.full((S, H, W), 0.5, np.float32)
    sigma = np.exp(rng.uniform(np.log(0.02), np.log(2.0), (H, W - W // 2))).astype(np.float32)
    v[:, :, W // 2:] = np.abs(1.0 + sigma[None] * rng.standard_normal((S, H, W - W // 2))).astype(np.float32)
    return np.repeat(v.reshape(S, W * H, 1), 3, 2)


@pytest.mark.parametrize("dilate", [0, 1])
def test_end_state_on_a_synthetic_sampler(exe, dilate):
    W, H, lo, hi, thr = 24, 10, 4, 32, 0.05
    smp = table_sampler(W, H, hi)
    px, mom, hist = A.simulate(exe, W, H, smp, lo, hi, threshold=thr, dilate=dilate)
    n = px[:, 3].reshape(H, W)
    assert np.array_equal(px[:, 3], mom[:, 3])
    left = n[:, :W // 2 - 1] if dilate else n[:, :W // 2]
    assert (left == lo).all(), "a constant pixel took more than min_samples"
    if dilate:                                                    # the guard column stays active as long as a right-hand neighbour does
        own_right = np.pad(n[:, W // 2], 1, mode="edge")
        longest = np.maximum(np.maximum(own_right[:-2], own_right[1:-1]), own_right[2:])
        assert (n[:, W // 2 - 1] >= lo).all() and (n[:, W // 2 - 1] <= np.maximum(longest, lo)).all() and (n[:, W // 2 - 1] > lo).any()
    r, ok = A.rel_error64(mom, 0.01)
    right = np.zeros((H, W), bool); right[:, W // 2:] = True
    right = right.reshape(-1)
    assert ((px[right, 3] == hi) | (r[right] <= thr * (1 + 1e-5))).all(), "a noisy pixel stopped above the threshold before max_samples"
    assert len(set(px[right, 3])) >= 3
    assert sum(c for c, _ in hist) == int(px[:, 3].sum())
    if not dilate:                                                # without the guard a pixel stops the moment it is below the threshold
        flags = A.run_cpu(exe, W, H, mom, threshold=thr, min_samples=lo, max_samples=hi, dilate=0)[0]
        assert not (flags & A.ACTIVE).any()


# ---- the oracle's per-sample microkernel images: a pure function of (scene, parameters), so the adaptive run is too
W3, H3, LO, HI = 80, 60, 4, 32


@pytest.fixture(scope="module")
def oracle_run():
    import common
    from fluctus_amd import host
    from oracle.binding import OracleContext
    d = common.mixed_material_scene()
    p = common.scene_params(d, W3, H3, maxBounces=4, useAreaLight=1, useEnvMap=1)
    env = host.synthetic_sky(64, 32)

    def make():
        o = OracleContext(W3 * H3, threads=8)
        o.upload_scene(d); o.upload_envmap(env)
        return o
    smp, acc = A.per_sample_stack(make(), p, HI)
    truth = A.per_sample_stack(make(), p, 512, keep=False)[1]
    return dict(samples=smp, acc=acc, truth=truth)


def test_simulated_render_on_the_oracle_stack(exe, oracle_run):
    """the adaptive render simulated from the oracle's per-sample images of mixed_material_scene 80 x 60: every pixel equals the uniform
    accumulation after its own count bit for bit (the simulation adds the same float32 values in the same order), several counts occur,
    and at equal budget the metric the rule controls is better than the uniform render's (measured: see DESIGN.md 4.2.1)"""
    smp, acc, truth = oracle_run["samples"], oracle_run["acc"], oracle_run["truth"]
    N = W3 * H3
    for dilate in (1, 0):
        px, mom, hist = A.simulate(exe, W3, H3, smp, LO, HI, dilate=dilate)
        n = px[:, 3].astype(np.int64)
        assert n.min() >= LO and n.max() <= HI and len(np.unique(n)) >= 3
        assert np.array_equal(px, acc[n - 1, np.arange(N)]), "a pixel differs from the uniform accumulation after its own count"
        S = int(n.sum())
        assert S == sum(c for c, _ in hist)
        spp = -(-S // N)                                           # rounded up: favours the uniform side
        qa, ra = A.quality(px, truth)
        qu, ru = A.quality(acc[spp - 1], truth)
        print(f"dilate {dilate}: {S} samples ({S / N:.2f} per pixel, counts {np.unique(n).size} distinct, {100 * (n == HI).mean():.1f} % at max) "
              f"adaptive metric {qa:.5f} rmse {ra:.5f} | uniform {spp} spp metric {qu:.5f} rmse {ru:.5f}")
        assert qa < qu, (qa, qu)


def test_sweep_prints_the_defaults_table(exe, oracle_run):
    """the sweep behind FLX_AD_DEFAULT_THRESHOLD: printed with -s; asserts only that the budget falls as the threshold rises"""
    smp, acc, truth = oracle_run["samples"], oracle_run["acc"], oracle_run["truth"]
    N, last = W3 * H3, None
    for thr in (0.02, 0.05, 0.1, 0.2):
        px, _, _ = A.simulate(exe, W3, H3, smp, LO, HI, threshold=thr)
        S = int(px[:, 3].sum()); spp = -(-S // N)
        qa, ra = A.quality(px, truth); qu, ru = A.quality(acc[spp - 1], truth)
        print(f"threshold {thr}: {S / N:.2f} spp, metric {qa:.5f} (uniform {spp} spp: {qu:.5f}), rmse {ra:.5f} ({ru:.5f})")
        assert last is None or S <= last
        last = S


def test_an_unsorted_list_is_caught(exe):
    """compare() demands the ascending list of the active pixels: a permuted list fails it (the mutation 'unstable list')"""
    W, H = 33, 17
    mom = synthetic_moments(W, H, 77)
    cpu, ref = A.run_cpu(exe, W, H, mom), A.reference(W, H, mom)
    A.compare(cpu, ref, MAX_EXCLUDED)
    assert cpu[2].size > 2
    with pytest.raises(AssertionError):
        A.compare((cpu[0], cpu[1], cpu[2][::-1].copy()), ref, MAX_EXCLUDED)
