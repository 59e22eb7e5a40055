"""Every traversal kernel the library can launch, on the adversarial scenes and rays of tests/traversal_cases.py, against the oracle on the
same input and against the float64 brute force.

Per scene (every builder) and per parameter set (env light on / area light off: far -> near any-hit order; both off: last-slot-first),
the crafted rays are loaded into a HipContext and an OracleContext as one extension and one shadow queue, and traced by
  default        persistent k_trace4r (closest hit) + k_shadow4
  refill         refill_extend 0 (thread-per-ray k_extend4) + refill_shadow 16 | 32 << 8 (persistent k_shadow4r)
  binary         extend_tree 2 / shadow_tree 2 (the reference's binary traversal order)
Asserted: any hit and the binary closest hit bit-identical to the oracle on every ray; on the decided rays the 4-wide closest hits pass
test_gpu_wide._extend_flips with zero flips, and on the others differ from the oracle only by a tie in t; every decided ray equals the
brute force.  The scenes include one past
2^26 (wideClamp 2^64), rays with exactly-zero direction components in the planes of flat boxes, and a root box past 2^62, which the upload
must refuse without breaking the context."""
import numpy as np
import pytest
import traversal_cases as tc
import common
import test_gpu_wide
from common import COL
from fluctus_amd import host, driver

pytestmark = pytest.mark.gpu
SCENES = dict(tc.scene_cases())
VARIANTS = {"default": {}, "refill": {"refill_extend": 0, "refill_shadow": 16 | (32 << 8)}, "binary": {"extend_tree": 2, "shadow_tree": 2}}


def _rays_and_witness(d):
    rays = tc.all_rays(tc.tri_points(d), tc.Leaves(d))
    orig = np.concatenate([r[0] for r in rays.values()]); dirs = np.concatenate([r[1] for r in rays.values()])
    tmax = np.concatenate([r[2] for r in rays.values()])
    gen = np.concatenate([np.full(r[0].shape[0], i) for i, r in enumerate(rays.values())])
    return orig, dirs, tmax, gen, list(rays)


@pytest.mark.parametrize("builder", tc.BUILDERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_kernels_vs_oracle_and_brute_force(name, builder):
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    d = tc.make_scene(SCENES[name])
    host.build_bvh(d, "sbvh")
    orig, dirs, tmax, gen, names = _rays_and_witness(d)
    host.build_bvh(d, builder)
    v = tc.BruteForce(tc.tri_points(d), orig, dirs, tmax).verdict(d)
    assert not v["uncovered"], f"{name}/{builder}: robust hits outside every leaf box of their triangle: {v['uncovered'][:3]}"
    n = orig.shape[0]
    dec, P = v["ext_decided"], tc.tri_points(d)
    g, o = HipContext(n), OracleContext(n, threads=16)
    try:
        launched = []
        for env in (1, 0):
            p = tc.params(d, env)
            for c in (g, o):
                c.upload_scene(d); c.set_params(p); driver.reset_renderer(c)
            info = g.scene_info()
            assert info["nested"] == 1
            for var, opts in VARIANTS.items():
                for k in ("extend_tree", "shadow_tree"):
                    g.set_option(k, opts.get(k, 4))
                g.set_option("refill_extend", opts.get("refill_extend", 16 | (32 << 8)))
                g.set_option("refill_shadow", opts.get("refill_shadow", -1))
                what = f"{name}/{builder}/env{env}/{var}"
                # closest hit, decided rays: test_gpu_wide._extend_flips (every hit record of an agreeing ray bit-identical), zero flips
                tc.load_rays(o, orig, dirs, tmax, np.nonzero(dec)[0])
                common.sync(g, o)
                _, flips = test_gpu_wide._extend_flips(g, o, what)
                assert flips == 0, f"{what}: {flips} decided rays flip against the oracle"
                hg, _ = tc.hits(g, n)
                ho, _ = tc.hits(o, n)
                # undecided rays (the reference's rounding decides them): hit / miss as the oracle, a different triangle only at the same t
                # within the fp32 resolution of the two intersections (tests/test_traversal_edges.py: the emulation's rule)
                tc.load_rays(o, orig, dirs, tmax, np.nonzero(~dec)[0])
                common.sync(g, o)
                g.wf_extend(); o.wf_extend(); g.finish()
                hu, _ = tc.hits(g, n)
                ou, _ = tc.hits(o, n)
                hg, ho = np.where(dec, hg, hu), np.where(dec, ho, ou)
                assert np.array_equal(hg >= 0, ho >= 0), f"{what}: hit / miss differs from the oracle on {int(((hg >= 0) != (ho >= 0)).sum())} rays"
                flip = hg != ho
                if var == "binary":
                    assert not flip.any(), f"{what}: the binary kernel's closest hit differs from the oracle's on {int(flip.sum())} rays"
                if flip.any():
                    (ta, ea), (tb, eb) = tc.pair_t(P, orig[flip], dirs[flip], hg[flip]), tc.pair_t(P, orig[flip], dirs[flip], ho[flip])
                    wide = ~(np.abs(ta - tb) <= 1e-5 * np.abs(tb) + 1e-6 + ea + eb)
                    assert not wide.any(), f"{what}: a closest-hit flip that is not a tie in t: {ta[wide][:4]} vs {tb[wide][:4]}"
                bad = v["ext_decided"] & (hg != ho)
                assert not bad.any(), f"{what}: {int(bad.sum())} decided rays flip against the oracle (generators {sorted({names[i] for i in gen[bad]})})"
                bad = v["ext_decided"] & (hg != v["closest"])
                assert not bad.any(), f"{what}: {int(bad.sum())} decided closest hits differ from the brute force, first {orig[bad][:1].tolist()} {dirs[bad][:1].tolist()}"
                # any hit: bit-identical on every ray
                tc.load_rays(o, orig, dirs, tmax)
                common.sync(g, o)
                g.wf_shadow(); o.wf_shadow(); g.finish()
                _, bg = tc.hits(g, n)
                _, bo = tc.hits(o, n)
                assert np.array_equal(bg, bo), f"{what}: shadowRayBlocked differs from the oracle on {int((bg != bo).sum())} of {n} rays"
                bad = v["sh_decided"] & (bg != v["blocked"])
                assert not bad.any(), f"{what}: {int(bad.sum())} decided shadow rays differ from the brute force"
                launched.append((env, var))
        assert len(launched) == 2 * len(VARIANTS)
    finally:
        g.close()
        o.close()


def test_upload_refuses_root_past_2_62_and_context_stays_usable():
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    bad = tc.make_scene(tc.beyond_bound_scene())
    host.build_bvh(bad, "sbvh")
    good = tc.make_scene(SCENES["flat_walls-o1e8"])
    host.build_bvh(good, "sbvh")
    orig, dirs, tmax, _, _ = _rays_and_witness(good)
    n = orig.shape[0]
    g, o = HipContext(n), OracleContext(n, threads=16)
    try:
        g.upload_scene(good)
        with pytest.raises(RuntimeError, match=r"beyond \+-2\^62"):
            g.upload_scene(bad)
        for c in (g, o):
            if c is o:
                c.upload_scene(good)
            c.set_params(tc.params(good, 0)); driver.reset_renderer(c)
            tc.load_rays(c, orig, dirs, tmax)
        g.wf_extend(); o.wf_extend(); g.wf_shadow(); o.wf_shadow(); g.finish()
        hg, bg = tc.hits(g, n)
        ho, bo = tc.hits(o, n)
        assert np.array_equal(bg, bo)
        # (the default closest-hit kernel may differ from the oracle by ties only; the context is on its previous scene)
        v = tc.BruteForce(tc.tri_points(good), orig, dirs, tmax).verdict(good)
        assert not (v["ext_decided"] & (hg != v["closest"])).any()
        assert g.state_export().view(np.int32)[COL.HIT_I][:n].max() < good.tris.size
    finally:
        g.close()
        o.close()
