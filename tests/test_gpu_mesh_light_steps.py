"""The MESH instances of mk_next_vertex and mk_sample_bsdf path by path: crafted states in, one kernel, the state out --
Ei against the float64 restatement of tests/mesh_light_step_cases.py within the tolerance derived per case, bit-identical where the
restatement says nothing is added, and every other column bit-identical to the option-off kernel (which is oracle-exact) run on the same
state, its seed advanced by the three draws the sampled light takes.  Then one absolute number: a lamp over a floor against Lambert's
closed form, in the three sampling modes."""
import numpy as np
import pytest
import mesh_light_cases as MC
import mesh_light_reference as MR
import mesh_light_step_cases as SC
from common import COL, PAD_COLS
from fluctus_amd import driver, host

pytestmark = pytest.mark.gpu
F = np.float32
EI = (COL.EI, COL.EI + 1, COL.EI + 2)
COLS = [c for c in range(64) if c not in PAD_COLS]
OTHER = [c for c in COLS if c not in EI]
_CACHE = {}


def make_ctx(d, n, mesh, update=None, env=None):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    g.set_option("mesh_lights", int(mesh))
    g.upload_scene(d)
    if update is not None:
        g.update_triangles(update)
    if env is not None:
        g.upload_envmap(env)
    return g


def run(g, p, st, step, lst=None):
    """one kernel on an imported state: (state out as uint32 (64, N), stats)"""
    g.set_params(p)
    g.mk_reset()
    g.state_import(st)
    if lst is not None:
        g.mk_active_write(lst)
    g.mk_stats(reset=True)
    getattr(g, step)()
    g.finish()
    out, stats = g.state_export().view(np.uint32).copy(), g.mk_stats()
    if lst is not None:
        g.mk_adaptive_clear()
    return out, stats


def template(g, p):
    g.set_params(p)
    g.mk_reset()
    return g.state_export().copy()


def ei_of(u, n):
    return u[list(EI), :n].view(F).T.astype(np.float64)


def same(a, b, cols, what, sel=slice(None)):
    for c in cols:
        bad = a[c][sel] != b[c][sel]
        assert not bad.any(), f"{what}: column {c} differs on {int(bad.sum())} paths, first {int(np.argmax(bad))}"


def check_ei(v, u_on, prior_bits, n, what, labels):
    """(i) decided cases within their tolerance of prior + dEi; (ii) where the restatement adds nothing, the prior's bits"""
    got = ei_of(u_on, n)
    r = np.where(v.decided, v.ratio(got), 0.0)
    worst = int(np.argmax(r))
    print(f"{what}: largest error / tolerance {r.max():.3f} (case {worst}, {labels[worst]}); {int(v.decided.sum())} of {n} decided, "
          f"{int((v.decided & ~v.silent).sum())} contribute")
    assert (r <= 1.0).all(), f"{what}: {int((r > 1.0).sum())} decided cases off float64, worst {r.max():.3g} at {worst} ({labels[worst]}): " \
                             f"{got[worst].tolist()} vs {v.out[worst].tolist()}"
    bad = v.silent & (u_on[list(EI), :n] != prior_bits).any(0)
    assert not bad.any(), f"{what}: Ei changed on {int(bad.sum())} paths that add nothing, first {int(np.argmax(bad))} ({labels[int(np.argmax(bad))]})"
    return float(r.max())


def world():
    """the scene on two contexts per group (option on / off), the triangle that gains its emission already updated, and the device's table"""
    if "w" not in _CACHE:
        S = SC.step_scene()
        a = SC.ImplicitCases(S)
        ga = [make_ctx(S.d0, a.n + SC.EXTRA, mesh, update=S.d1.tris) for mesh in (1, 0)]
        tab = ga[0].mesh_lights_read()
        for x, y in zip(tab[:3], S.table[:3]):
            assert x.tobytes() == y.tobytes(), "the device's table is the host's (the CPU self-checks ran on those bytes)"
        assert not np.isin(S.gains, tab[0])
        b = SC.SampledCases(S, tab)
        env = host.synthetic_sky(64, 32)
        gb = [make_ctx(S.d0, b.n + SC.EXTRA, mesh, update=S.d1.tris, env=env) for mesh in (1, 0)]
        _CACHE["w"] = S, tab, a, ga, b, gb
    return _CACHE["w"]


# ---- A. mk_next_vertex
@pytest.mark.parametrize("expl,impl", SC.MODES)
def test_implicit_hit(expl, impl):
    S, tab, c, (on, off), _, _ = world()
    n = c.n
    p = S.params(n, (expl, impl))
    assert int(p["width"]) * int(p["height"]) >= n + SC.EXTRA and (n + SC.EXTRA) % 64
    st = c.state(template(on, p))
    v = SC.implicit_verdict(S, c, tab, (expl, impl))
    a, sa = run(on, p, st, "mk_next_vertex")
    b, sb = run(off, p, st, "mk_next_vertex")
    same(a, b, OTHER, "option on against off")                          # (iii) phase and pathLen included
    assert np.array_equal(sa, sb) and int(sa[0]) == (c.len_before == 0).sum() and int(sa[1]) == (c.len_before > 0).sum()
    same(b, st.view(np.uint32), EI, "option off leaves Ei alone")
    hit = b[COL.HIT_I, :n].view(np.int32)
    assert np.array_equal(hit[c.robust], c.hit[c.robust]), "the float64 nearest hit is the traversal's on the robust rays"
    assert np.array_equal(b[COL.PATH_LEN, :n], c.len_before + 1) and (b[COL.PHASE, :n][hit >= 0] == SC.PH_SAMPLE_BSDF).all()
    check_ei(v, a, st.view(np.uint32)[list(EI), :n], n, f"implicit hit, sampleExpl {expl} sampleImpl {impl}", c.label)
    same(a, st.view(np.uint32), COLS, "padding paths", sel=slice(n, None))


def test_implicit_hit_behind_the_parametric_quad():
    """useAreaLight: where the quad is met before the lamp it wins (flags 1, the path ends on the quad's E) and the lamp adds nothing"""
    S, tab, c, (on, off), _, _ = world()
    n = c.n
    p = S.params(n, (1, 1), useAreaLight=1)
    st = c.state(template(on, p))
    v = SC.implicit_verdict(S, c, tab, (1, 1), quad=True)
    a, sa = run(on, p, st, "mk_next_vertex")
    b, sb = run(off, p, st, "mk_next_vertex")
    same(a, b, OTHER, "option on against off")
    assert np.array_equal(sa, sb)
    wins = c.quad_wins & c.robust
    assert wins.sum() >= 10 and (a[COL.AREA_LIGHT_HIT, :n][wins] == 1).all() and (a[COL.PHASE, :n][wins] == SC.PH_SPLAT).all()
    assert (a[COL.AREA_LIGHT_HIT, :n][c.quad_clear & ~c.quad_wins] == 0).all()
    same(a, b, EI, "the quad wins: Ei as with the option off", sel=np.nonzero(wins)[0])
    assert (ei_of(a, n)[wins] > c.Ei[wins]).all(), "the quad's own emission arrives"
    lamp_behind = wins & (S.ke[np.maximum(c.hit, 0)] > 0).any(1) & (c.hit >= 0)
    assert lamp_behind.sum() >= 10, "rays that would have met a lamp's front"
    v.decided &= ~c.quad_wins
    v.silent &= ~c.quad_wins
    check_ei(v, a, st.view(np.uint32)[list(EI), :n], n, "implicit hit with the parametric quad on", c.label)
    assert (~c.quad_wins).sum() > 0.9 * n


# ---- B. mk_sample_bsdf
def sampled_seeds(c, expl):
    """the option-off partner's seed: the mesh lights' three draws taken on the CPU (none on a singular receiver or without sampleExpl)"""
    return np.where(c.singular | (not expl), c.seed.astype(np.uint32), SC.advance(c.seed, 3))


@pytest.mark.parametrize("expl,impl", SC.MODES)
def test_sampled_light(expl, impl):
    S, tab, _, _, c, (on, off) = world()
    n = c.n
    p = S.params(n, (expl, impl))
    assert int(p["width"]) * int(p["height"]) >= n + SC.EXTRA and (n + SC.EXTRA) % 64
    t = template(on, p)
    st = c.state(t.copy())
    g = SC.SampledGeometry(S, c, tab)
    v = SC.sampled_verdict(S, c, tab, g, (expl, impl))
    a, sa = run(on, p, st, "mk_sample_bsdf")
    b, sb = run(off, p, c.state(t.copy(), seed=sampled_seeds(c, expl)), "mk_sample_bsdf")
    same(a, b, OTHER, "draw order: option on against off with the seed advanced three draws")       # (ii) T, seed, orig, lastPdfW, dir, lastSpecular, phase
    same(b, st.view(np.uint32), EI, "option off, no other light: Ei stays")
    check_ei(v, a, st.view(np.uint32)[list(EI), :n], n, f"sampled light, sampleExpl {expl} sampleImpl {impl}", c.label)
    # (iii) a singular receiver: nothing drawn, nothing traced -- the whole state as with the option off from the SAME seed
    sing = np.nonzero(c.singular)[0]
    assert sing.size >= 40
    same(a, b, COLS, "singular receivers", sel=sing)
    assert np.array_equal(st.view(np.uint32)[COL.SEED, sing], c.seed[sing].astype(np.uint32))
    # (iv) one shadow ray per active non-singular path, and none with the option off
    rays = int((~c.singular).sum()) if expl else 0
    assert int(sa[2]) == rays and int(sb[2]) == 0, (sa, sb, rays)
    assert np.array_equal(sa[[0, 1, 3]], sb[[0, 1, 3]])
    same(a, st.view(np.uint32), COLS, "padding paths", sel=slice(n, None))


def test_no_pickable_light_draws_nothing():
    """emissive materials on zero-area triangles only: a list, no weight -- the state and the counters of the option-off kernel, same seed"""
    _, _, _, _, c, _ = world()
    d = MC.degenerate_lamps_scene()
    host.build_bvh(d, "sbvh")
    S = SC.step_scene()
    n = 300
    p = S.params(n, (1, 1))
    p["worldRadius"], p["n_tris"] = d.world_radius, d.tris.size
    on, off = make_ctx(d, n + SC.EXTRA, 1), make_ctx(d, n + SC.EXTRA, 0)
    tab = on.mesh_lights_read()
    assert tab[3] == 0.0 and not (tab[2] > 0).any() and MR.lights(d).size == 4, "emissive triangles, none of them pickable"
    st = c.state(np.concatenate([template(on, p)] * ((c.n + SC.EXTRA) // (n + SC.EXTRA) + 1), 1))[:, :n + SC.EXTRA].copy()
    u = st.view(np.uint32)
    u[COL.MAT_ID, :n] = np.arange(n) % 4                                   # the scene's materials (all diffuse), its triangles
    u[COL.HIT_I, :n] = np.arange(n) % d.tris.size
    u[COL.PHASE, n:] = SC.PH_SPLAT
    a, sa = run(on, p, st, "mk_sample_bsdf")
    b, sb = run(off, p, st, "mk_sample_bsdf")
    same(a, b, COLS, "no pickable light")
    assert np.array_equal(sa, sb) and int(sa[2]) == 0
    assert (a[COL.SEED, :n] != u[COL.SEED, :n]).all(), "the paths ran"
    on.close(); off.close()


# ---- C. the three kinds of light together
@pytest.mark.parametrize("expl,impl", [(1, 1), (1, 0)])
def test_sampled_light_after_the_environment_and_the_quad(expl, impl):
    """useEnvMap and useAreaLight on: the mesh draws are numbers 4 to 6 of the stream (environment 1, quad 2, mesh 3).
    dEi: what the mesh lights add from those draws, read as Ei of the option-on kernel run alone (no other light, the seed advanced three
    draws, prior Ei 0: 0 + x is x) and held to float64 within the case's tolerance -- derived on dEi itself, no prior to lean on.
    Ei_on against fl32(Ei_off + dEi) within 2 ulp of the sum, Ei_off from the option-off run of the same seed.
    The other columns against the option-off kernel without the other two lights, its seed advanced by the six draws: what the sampler
    sees does not depend on who took them."""
    import copy
    S, tab, _, _, c, (on, off) = world()
    n = c.n
    sub = np.isin(c.group, ("pick edges", "arrangements", "horizon", "back face", "singular", "random"))
    p = S.params(n, (expl, impl), useEnvMap=1, useAreaLight=1, envMapStrength=1.5)
    t = template(on, p)
    st = c.state(t.copy())
    c0 = copy.copy(c)
    c0.Ei = np.zeros_like(c.Ei)
    g = SC.SampledGeometry(S, c, tab, first=3)
    v = SC.sampled_verdict(S, c0, tab, g, (expl, impl))
    a, sa = run(on, p, st, "mk_sample_bsdf")
    b, sb = run(off, p, st, "mk_sample_bsdf")
    adv = lambda k: np.where(c.singular, c.seed.astype(np.uint32), SC.advance(c.seed, k))
    bare, _ = run(off, S.params(n, (expl, impl)), c.state(t.copy(), seed=adv(6)), "mk_sample_bsdf")
    lone, _ = run(on, S.params(n, (expl, impl)), c0.state(t.copy(), seed=adv(3)), "mk_sample_bsdf")
    same(a, bare, OTHER, "draw order: the mesh lights draw after the environment and the quad", sel=np.nonzero(sub)[0])
    nonsing = int((~c.singular).sum())
    assert int(sa[2]) == 3 * nonsing and int(sb[2]) == 2 * nonsing
    # dEi against float64
    m = sub & v.decided
    print(f"three lights: {int((sub & ~v.decided).sum())} of {int(sub.sum())} undecided with no prior")
    assert (sub & ~v.decided).sum() <= SC.UNDECIDED_CAP * sub.sum()
    v.decided = m
    v.silent = v.silent & m
    check_ei(v, lone, np.zeros((3, n), np.uint32), n, f"three lights, sampleExpl {expl} sampleImpl {impl}: dEi alone", c.label)
    # the sum
    ei_on, ei_off, delta = ei_of(a, n), ei_of(b, n), ei_of(lone, n)
    assert (ei_off[m] > c.Ei[m]).any(1).mean() > 0.5, "the other two lights add to most paths"
    total = (ei_off + delta).astype(F)
    dist = np.where(m[:, None], MR.ulp_diff(ei_on.astype(F), total), 0).max(1)
    w = int(np.argmax(dist))
    print(f"three lights, sampleExpl {expl} sampleImpl {impl}: Ei_on is at most {dist.max()} ulp from fl32(Ei_off + dEi) (case {w}, {c.label[w]}); "
          f"{int(m.sum())} decided, the mesh lights add on {int((m & ~v.silent).sum())}")
    assert (m & ~v.silent).sum() > 300
    assert (dist <= 2).all(), f"{int((dist > 2).sum())} decided cases beyond 2 ulp of the sum, worst {dist.max()} at {w} ({c.label[w]})"
    same(a, b, EI, "nothing added: Ei as with the option off", sel=np.nonzero(m & v.silent)[0])


# ---- D. the list-driven instances
@pytest.mark.parametrize("size", [1, 63, 65, 0])
def test_sampled_light_through_a_list(size):
    S, tab, _, _, c, _ = world()
    n = c.n
    if "d" not in _CACHE:
        g = make_ctx(S.d0, n + SC.EXTRA, 1, update=S.d1.tris)
        p = S.params(n, (1, 1), width=n + SC.EXTRA, height=1)                   # a list needs one path per pixel
        st = c.state(template(g, p))
        _CACHE["d"] = g, p, st, run(g, p, st, "mk_sample_bsdf")
    g, p, st, (full, sfull) = _CACHE["d"]
    lst = np.sort(np.random.RandomState(size).permutation(n)[:size or n]).astype(np.uint32)
    a, sa = run(g, p, st, "mk_sample_bsdf", lst=lst)
    listed = np.zeros(n + SC.EXTRA, bool); listed[lst] = True
    same(a, full, COLS, "listed paths against the full grid", sel=listed)
    same(a, st.view(np.uint32), COLS, "unlisted paths untouched", sel=~listed)
    assert int(sa[2]) == int((~c.singular[lst]).sum())
    if not size:
        assert np.array_equal(sa, sfull)


# ---- 3. one absolute number
LF_SPP = 256
LF_TILE_SE = {(1, 1): 0.02, (1, 0): 0.02, (0, 1): 0.08}


@pytest.mark.parametrize("expl,impl", SC.MODES)
def test_lamp_over_floor_against_the_closed_form(expl, impl):
    """|mean - truth| <= 5 SE on every 8 x 8 tile and on the whole image, with the SEs themselves bounded so that noise cannot hide a bias"""
    from fluctus_amd.device import HipContext
    d = SC.lamp_floor_scene()
    p = SC.lamp_floor_params(d, (expl, impl))
    W, H = SC.LF_W, SC.LF_H
    if "truth" not in _CACHE:
        _CACHE["truth"] = SC.lamp_floor_truth(p, 4)
    truth = _CACHE["truth"]
    g = HipContext(W * H)
    g.set_option("moments", 1); g.set_option("mesh_lights", 1)
    g.upload_scene(d)
    driver.render_single(g, p, LF_SPP)
    px, mom = g.read_pixels(0), g.read_pixels(7)
    g.close()
    assert (px[:, 3] == LF_SPP).all() and np.isfinite(px).all()
    assert np.allclose(px[:, 0], px[:, 1], rtol=1e-5) and np.allclose(px[:, 0], px[:, 2], rtol=1e-5), "a grey lamp over a grey floor"
    mean, var = MR.tile_stats(px, mom, W, H)
    tt = SC.tile_means(truth)
    se = np.sqrt(var)
    z = np.abs(mean - tt) / se
    m = np.asarray(mom, np.float64).reshape(H, W, 4)
    pm = m[..., 0] / m[..., 3]
    pv = np.maximum(m[..., 1] / m[..., 3] - pm * pm, 0.0) / m[..., 3]
    all_mean, all_se = pm.mean(), np.sqrt(pv.sum()) / (W * H)
    z_all = abs(all_mean - truth.mean()) / all_se
    print(f"lamp over floor, sampleExpl {expl} sampleImpl {impl}: largest |mean - truth| / SE over {z.size} tiles {z.max():.2f}, whole image {z_all:.2f}; "
          f"relative SE of a tile {(se / tt).min():.4f} .. {(se / tt).max():.4f}, of the image {all_se / truth.mean():.5f}; "
          f"image mean {all_mean:.5f} against {truth.mean():.5f}")
    assert all_se / truth.mean() <= 0.003 and (se / tt).max() <= LF_TILE_SE[(expl, impl)]
    assert (SC.LF_SUBPIXEL_REL * tt <= 0.1 * se).all(), "the truth's sub-pixel grid has converged to a tenth of every tile's SE"
    assert (z <= 5.0).all() and z_all <= 5.0
