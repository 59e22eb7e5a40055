"""Emissive triangles as lights of the WAVEFRONT integrator (option "mesh_lights_wavefront"): off is off, the boundary runs the
unfused chain while the lamps light it, the MESH instance of the plain logic pass path by path against float64 (implicit hits and sampled
lights), one absolute number (a lamp over a floor against Lambert's closed form), the wavefront loop against the microkernel integrator with
all three kinds of light on, and lamps that move between two renders."""
import numpy as np
import pytest
import bsdf_cases as bc
import common
import logic_step_cases as LC
import mesh_light_cases as MC
import mesh_light_reference as MR
import mesh_light_step_cases as SC
import wf_mesh_light_cases as WC
from common import COL, Q, PAD_COLS
from fluctus_amd import driver, host

pytestmark = pytest.mark.gpu
F = np.float32
EI = (COL.EI, COL.EI + 1, COL.EI + 2)
COLS = [c for c in range(64) if c not in PAD_COLS and c != COL.PHASE]
MATERIAL_QUEUES = (Q.DIFFUSE, Q.GLOSSY, Q.GGX_REFL, Q.GGX_REFR, Q.DELTA)
_CACHE = {}


def ctx(n, **options):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    for k, v in options.items():
        g.set_option(k, v)
    return g


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def counters(c):
    cnt = c.get_counters()
    if hasattr(c, "finish"):
        c.finish()
    return np.array(cnt, copy=True)


def queue_sets(snap):
    cnt, qs = snap[2], snap[3]
    return {qi: np.asarray(qs[qi][:int(cnt[qi])], np.int64) for qi in range(Q.NUM)}


# ---- 1. off is off
@pytest.mark.parametrize("mesh,wavefront,emissive", [(0, 1, True), (1, 1, False), (1, 0, True)])
def test_off_is_off(mesh, wavefront, emissive):
    """reset -> (logic, raygen, materials, extend, shadow) x 4 in lockstep with the oracle, which knows nothing of Ke: the same bits in state,
    queues, counters and pixels, and the fused pass is the one that ran"""
    from oracle.binding import OracleContext
    d = WC.emissive_mixed_scene(emissive)
    w, h = 64, 48
    n = w * h + 100
    p = common.scene_params(d, w, h, maxBounces=4, useAreaLight=1, useEnvMap=1, envMapStrength=1.5, wfSeparateQueues=1)
    g, o = ctx(n, extend_tree=2, mesh_lights_wavefront=wavefront, mesh_lights=mesh), OracleContext(n, threads=8)
    env = host.synthetic_sky(64, 32)
    for c in (g, o):
        c.upload_scene(d); c.upload_envmap(env); c.set_params(p)
        driver.reset_renderer(c)
    assert g.get_option("mesh_lights") == mesh and g.get_option("mesh_lights_wavefront") == wavefront, "both options survive the upload"
    if mesh:
        assert (g.mesh_lights_read()[0].size > 0) == emissive
    g.profile_enable(1); g.profile_reset()
    for it in range(4):
        for c in (g, o):
            c.wf_logic(False); c.wf_raygen(); c.wf_materials()
        cg, cc = counters(g), counters(o)
        assert np.array_equal(cg, cc), f"iteration {it}: counters {cg} vs {cc}"
        for qi in range(Q.NUM):
            x, y = g.queue_read(qi)[:int(cg[qi])], o.queue_read(qi)[:int(cc[qi])]
            if qi == Q.EXTENSION:                                       # (the fused pass lists the continuing paths by path id: the same set)
                x, y = np.sort(x), np.sort(y)
            assert np.array_equal(x, y), f"iteration {it}: queue {qi} differs"
        for c in (g, o):
            c.wf_extend(); c.wf_shadow()
        g.finish()
        fails = common.state_diff(g.state_export(), o.state_export(), 0.0, 0.0)
        assert not fails, f"iteration {it}: " + "; ".join(fails[:4])
        for c in (g, o):
            c.clear_queues()
            if hasattr(c, "finish"):
                c.finish()
            c.pixel_index_update(w * h, int(cc[0]))
    prof = g.profile_get(); g.profile_enable(0)
    assert prof["logic_fused"][1] == 4 and prof["logic"][1] == 0, prof
    assert np.array_equal(bits(g.read_pixels(0)), bits(o.read_pixels(0))), "the framebuffer differs"
    g.close()


# ---- 2. the boundary
def test_boundary_runs_the_unfused_chain():
    d = WC.emissive_mixed_scene(True)
    w, h = 64, 48
    n = w * h + 100
    p = common.scene_params(d, w, h, maxBounces=4, useAreaLight=1, useEnvMap=1, envMapStrength=1.5, wfSeparateQueues=1)
    g = ctx(n, mesh_lights=1, mesh_lights_wavefront=1)
    g.upload_scene(d); g.upload_envmap(host.synthetic_sky(64, 32)); g.set_params(p)
    assert g.get_option("fuse") == 1 and g.get_option("extend_tree") == 4 and g.get_option("refill_extend") > 0, "the defaults: fused, the persistent 4-wide kernel"

    def chain_after_a_raw_extend():
        driver.reset_renderer(g)
        g.wf_logic(False); g.wf_raygen(); g.wf_materials()
        g.wf_extend()
        assert g.get_option("phase") & 8, "the extension kernel left RAW hit records"
        g.wf_shadow(); g.clear_queues()
        g.profile_enable(1); g.profile_reset()
        g.wf_logic(False); g.wf_raygen(); g.wf_materials()
        g.finish()
        prof = g.profile_get(); g.profile_enable(0)
        assert not g.get_option("phase") & 8, "the RAW records are committed"
        assert g.get_option("fuse") == 1, "\"fuse\" reads back what the caller set"
        return prof["logic"][1], prof["logic_fused"][1]
    assert chain_after_a_raw_extend() == (1, 0), "lamps light the wavefront integrator: the plain pass, its MESH instance"
    g.set_option("mesh_lights_wavefront", 0)
    assert chain_after_a_raw_extend() == (0, 1), "switched off: the fused pass is back"
    g.set_option("mesh_lights_wavefront", 1)
    assert chain_after_a_raw_extend() == (1, 0)
    g.set_option("mesh_lights", 0)
    assert chain_after_a_raw_extend() == (0, 1), "inert without \"mesh_lights\""
    g.close()


# ---- 3. / 4. path by path
def check_ei(v, got, prior_bits, got_bits, what, labels):
    r = np.where(v.decided, v.ratio(got), 0.0)
    worst = int(np.argmax(r))
    print(f"{what}: largest error / tolerance {r.max():.3f} (case {worst}, {labels[worst]}); {int(v.decided.sum())} of {v.decided.size} decided, "
          f"{int((v.decided & ~v.silent).sum())} contribute")
    assert (r <= 1.0).all(), f"{what}: {int((r > 1.0).sum())} decided cases off float64, worst {r.max():.3g} at {worst} ({labels[worst]}): " \
                             f"{got[worst].tolist()} vs {v.out[worst].tolist()}"
    bad = v.silent & (got_bits != prior_bits).any(0)
    assert not bad.any(), f"{what}: Ei changed on {int(bad.sum())} paths that add nothing, first {int(np.argmax(bad))} ({labels[int(np.argmax(bad))]})"
    return float(r.max())


def step_world():
    """the step scene on two contexts per group (both options on / both off), the triangle that gains its emission already updated"""
    if "w" not in _CACHE:
        S, a = WC.implicit_cases()
        env = host.synthetic_sky(64, 32)

        def make(n, on):
            g = ctx(n, extend_tree=2, mesh_lights=int(on), mesh_lights_wavefront=int(on))
            g.upload_scene(S.d0); g.update_triangles(S.d1.tris); g.upload_envmap(env)
            return g
        ga = [make(a.n + WC.EXTRA, on) for on in (True, False)]
        tab = ga[0].mesh_lights_read()
        for x, y in zip(tab[:3], S.table[:3]):
            assert x.tobytes() == y.tobytes(), "the device's table is the host's"
        b = SC.SampledCases(S, tab)
        gb = [make(b.n + WC.EXTRA, on) for on in (True, False)]
        _CACHE["w"] = S, tab, a, ga, b, gb
    return _CACHE["w"]


@pytest.mark.parametrize("cfg", list(WC.LIGHTS))
@pytest.mark.parametrize("expl,impl", SC.MODES)
def test_implicit_hits(expl, impl, cfg):
    S, tab, c, (on, off), _, _ = step_world()
    w, n = WC.WfImplicit(c), c.n
    assert w.n_tasks % 64
    p = S.params(n, (expl, impl), **WC.LIGHTS[cfg])
    assert int(p["width"]) * int(p["height"]) >= w.n_tasks
    v, base = WC.implicit_verdict(S, c, tab, (expl, impl), cfg)
    share = float((~v.decided[base]).mean())
    print(f"implicit hits, {cfg}: {share:.4f} of the robust cases undecided")
    assert share <= SC.UNDECIDED_CAP
    snaps = []
    for g in (on, off):
        g.set_params(p)
        driver.reset_renderer(g)
        st = LC.load_rays(g, w)
        g.wf_extend()
        g.clear_queues()
        g.profile_enable(1); g.profile_reset()
        g.wf_logic(False)
        snaps.append(LC.snapshot(g))
        prof = g.profile_get(); g.profile_enable(0)
        assert prof["logic"][1] == 1 and prof["logic_fused"][1] == 0, prof
    a, b = snaps
    ua, ub, u0 = a[0].view(np.uint32), b[0].view(np.uint32), st.view(np.uint32)
    quad = bool(WC.LIGHTS[cfg]["useAreaLight"]) and bool(impl)
    seen = c.robust & ~(c.quad_wins if quad else False)
    assert np.array_equal(ua[COL.HIT_I, :n].view(np.int32)[seen], c.hit[seen]), "the float64 nearest hit is the traversal's on the robust rays"
    what = f"implicit hits, {cfg}, sampleExpl {expl} sampleImpl {impl}"
    check_ei(v, a[0][list(EI), :n].T.astype(np.float64), u0[list(EI), :n], ua[list(EI), :n], what, c.label)
    assert (v.decided & ~v.silent).sum() > 100, "lamps are collected"
    # the path continues: the queues that say where a path goes next, and pathLen, as with the option off
    qa, qb = queue_sets(a), queue_sets(b)
    for qi in (Q.RAYGEN,) + MATERIAL_QUEUES:
        assert np.array_equal(qa[qi], qb[qi]), f"{what}: queue {qi} differs from the option-off pass"
    assert np.array_equal(ua[COL.PATH_LEN], ub[COL.PATH_LEN]) and np.array_equal(ua[COL.PATH_LEN, :n], c.len_before + 1)
    lamps_hit = v.decided & ~v.silent & (c.T != 0).any(1)
    assert not np.isin(np.nonzero(lamps_hit)[0], qa[Q.RAYGEN]).any(), "a path that collects a lamp is not terminated by it"
    # option off: Ei is the oracle-exact plain pass's, which adds nothing for a triangle
    if not WC.LIGHTS[cfg]["useEnvMap"] and not quad:
        assert np.array_equal(ub[list(EI), :n], u0[list(EI), :n])


def test_last_vertex_rule():
    """4.2.3, the last vertex: a path ended by the bounce limit ALONE still collects the lamp it has just hit -- the same bits as under a limit it
    does not reach (which test_implicit_hits holds to float64) -- and is ended all the same; a path the roulette kills collects nothing, one it
    spares collects with T / contProb; a path with lastPdfW = 0 collects nothing under either limit."""
    import copy
    S, tab, c0, (on, _), _, _ = step_world()
    n = c0.n
    c = copy.copy(c0)
    c.lastPdfW = c0.lastPdfW.copy()
    dead = np.arange(n) % 7 == 3
    c.lastPdfW[dead] = 0.0
    w = WC.WfImplicit(c)
    prior = SC.f32(c.Ei).astype(F)

    def run(**kw):
        p = S.params(n, (1, 1), **kw)
        on.set_params(p)
        driver.reset_renderer(on)
        LC.load_rays(on, w)
        on.wf_extend()
        on.clear_queues()
        on.wf_logic(False)
        s = LC.snapshot(on)
        ended = np.zeros(w.n_tasks, bool); ended[queue_sets(s)[Q.RAYGEN]] = True
        return s[0][list(EI), :n].T.copy(), ended[:n]
    far, far_ended = run(maxBounces=8)
    cut, cut_ended = run(maxBounces=1)
    live = (c.T != 0).any(1) & ~dead
    at_limit = c.len_before + 1 >= 2                                        # len >= maxBounces + 1 under maxBounces = 1
    added = (far != prior).any(1)
    assert (added & live & at_limit).sum() > 200, "lamps are collected by paths at the limit"
    assert np.array_equal(cut.view(np.uint32), far.view(np.uint32)), "the bounce limit alone changes nothing of what a path collects"
    assert cut_ended[at_limit].all() and not far_ended[live & added].any(), "... and ends the path all the same"
    assert dead.sum() > 100 and np.array_equal(far.view(np.uint32)[dead], prior.view(np.uint32)[dead]) and far_ended[dead].all(), "lastPdfW = 0: ended, nothing collected"
    # the roulette: contProb = clamp(luminance(T), 0.01, 0.5) in fp32, one draw of the path's seed; killed where the draw is larger
    rl, rl_ended = run(maxBounces=1, useRoulette=1)
    T32 = c.T.astype(F)
    lum = (F(LC.LUM[0]) * T32[:, 0] + F(LC.LUM[1]) * T32[:, 1]).astype(F) + F(LC.LUM[2]) * T32[:, 2]
    cont = np.clip(lum, F(0.01), F(0.5)).astype(np.float64)
    draw, _ = bc.rand01((np.arange(n) * 2654435761 % 2 ** 32).astype(np.uint64))
    clear = np.abs(draw - cont) > 1e-5
    played = at_limit & live & clear
    killed, spared = played & (draw > cont), played & (draw < cont)
    assert killed.sum() > 100 and spared.sum() > 100
    assert np.array_equal(rl.view(np.uint32)[killed], prior.view(np.uint32)[killed]) and rl_ended[killed].all(), "killed by the roulette: nothing collected"
    assert not rl_ended[spared & added].any()
    d_far, d_rl = far.astype(np.float64) - prior, rl.astype(np.float64) - prior
    ok = np.abs(d_rl * cont[:, None] - d_far) <= 1e-5 * np.abs(far) + 1e-7
    assert ok[spared].all(), "spared by the roulette: the same lamp with T / contProb"
    assert np.array_equal(rl.view(np.uint32)[~at_limit], far.view(np.uint32)[~at_limit]), "below the limit the roulette is not played"


@pytest.mark.parametrize("cfg", ["env", "both"])
def test_implicit_environment_weight(cfg):
    """rays that leave the scene, MIS: the MESH instance weighs the implicit environment hit with lastPdfW / (lastPdfW + pdf k), k = useEnvMap / den
    from the parameters (4.2.3) -- the complement of the NEE weight -- and not with the reference's (lastPdfW pick) / (lastPdfW pick + pdf).
    No float64 environment lookup is needed: lastPdfW / (lastPdfW + pdf k) IS the reference's weight for lastPdfW / k and pick = 1, so the
    option-off plain pass (oracle-exact) on that state is the yardstick -- bit for bit where k = 1/2 (both scalings are exact), within 16 ulp of
    Ei where k = 1/3 (lastPdfW / k rounds, and so do the two sums)."""
    import types
    S, tab, c, (on, off), _, _ = step_world()
    n = c.n
    rng = np.random.RandomState(61)
    d = rng.normal(size=(n, 3)); d[:, 1] = np.abs(d[:, 1]) + 0.2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = types.SimpleNamespace(n=n, orig=SC.f32(np.tile([0.0, 30.0, 0.0], (n, 1)) + rng.uniform(-1, 1, (n, 3))), dir=SC.f32(d), T=c.T, Ei=c.Ei,
                              lastPdfW=c.lastPdfW, lastSpecular=c.lastSpecular, len_before=c.len_before)
    w = WC.WfImplicit(m)
    k = F(F(1.0) / F(WC.den_of(cfg)))
    p = S.params(n, (1, 1), **WC.LIGHTS[cfg])

    def run(g, edit):
        g.set_params(p)
        driver.reset_renderer(g)
        st = w.state(g.state_export().copy())
        edit(st)
        g.state_import(st); g.clear_queues()
        g.queue_write(Q.EXTENSION, w.index.astype(np.uint32))
        cnt = counters(g); cnt[:] = 0; cnt[Q.EXTENSION] = n
        g.set_counters(cnt)
        g.wf_extend(); g.clear_queues()
        g.wf_logic(False)
        g.finish()
        return g.state_export().copy()

    def scaled(st):
        st[COL.LAST_PICK_PROB, :n] = 1.0
        st[COL.LAST_PDF_W, :n] = (st[COL.LAST_PDF_W, :n] / k).astype(F)

    def as_stored(st):
        st[COL.LAST_PICK_PROB, :n] = k                                         # what the previous vertex' sample would have stored
    a, b, r = run(on, lambda st: None), run(off, scaled), run(off, as_stored)
    assert (a.view(np.int32)[COL.HIT_I, :n] == -1).all(), "every ray leaves the scene"
    ea, eb, er = (x[list(EI), :n].T.astype(np.float64) for x in (a, b, r))
    mis = (c.len_before + 1 > 1) & (c.lastSpecular == 0) & (c.T != 0).any(1)
    assert mis.sum() > 300 and (ea > c.Ei).any(1)[(c.T != 0).any(1)].mean() > 0.9, "the environment adds to the live paths"
    if cfg == "env":
        assert np.array_equal(a.view(np.uint32)[list(EI), :n], b.view(np.uint32)[list(EI), :n]), "k = 1/2: the yardstick's bits"
    err = np.abs(ea - eb) / (2.0 ** -24 * np.abs(eb).max(1, keepdims=True))
    print(f"implicit environment weight, {cfg}: Ei at most {err.max():.2f} ulp from the plain pass at lastPdfW / k, pick 1; "
          f"the reference's weight differs on {int(((ea != er).any(1) & mis).sum())} of {int(mis.sum())} MIS paths")
    assert (err <= 16.0).all()
    assert ((ea != er).any(1) & mis).mean() > 0.25 * mis.mean(), "the two weights differ where the environment's pdf matters"
    assert np.array_equal(ea[~mis], er[~mis]), "no MIS weight: nothing to correct"


@pytest.mark.parametrize("cfg,mode", [("none", (1, 1)), ("both", (1, 1)), ("both", (1, 0))])
def test_sampled_lights(cfg, mode):
    """crafted hit records -> wf_logic: the draws, the stored sample, the shadow queue; -> wf_shadow: the brute force's any-hit over
    [0, 0.995 |L|]; -> materials, extend, and the option-off plain logic pass: the consumed light sample against float64 (den = 1 and 3);
    then the MESH instance's own consume step, in the two steps of 4.2.2 group C: dEi read from that instance with prior 0 against float64,
    and Ei of the pass in which the other kinds add too against fl32(Ei without the sample + dEi)"""
    S, tab, _, _, c, (on, off) = step_world()
    ws, n = WC.WfSampled(c, cfg), c.n
    den = WC.den_of(cfg)
    p = S.params(n, mode, **WC.LIGHTS[cfg])
    assert int(p["width"]) * int(p["height"]) >= ws.n_tasks and ws.n_tasks % 64
    g = SC.SampledGeometry(S, c, tab)                                       # c.seed is the stream behind the kind draw: pick, r1, r2 follow
    r = WC.sample_restatement(S, c, g, tab, den)
    on.set_params(p)
    driver.reset_renderer(on)
    st = ws.state(on.state_export().copy())
    on.state_import(st); on.clear_queues()
    on.wf_logic(False)
    a = LC.snapshot(on)
    ua, u0 = a[0].view(np.uint32), st.view(np.uint32)
    qa = queue_sets(a)
    nonsing = ~c.singular & (c.T != 0).any(1)
    mesh, envk, quadk = nonsing & (ws.kind == 2), nonsing & (ws.kind == 0), nonsing & (ws.kind == 1)
    assert mesh.sum() >= (300 if den == 3 else 1000), "enough paths pick the lamps"
    what = f"sampled lights, {cfg}, sampleExpl {mode[0]} sampleImpl {mode[1]}"
    # the draws: 1 + 3 for the lamps, 1 + 1 for the environment map, 1 + 2 for the quad, none on a singular receiver
    seed0 = ws.seed.astype(np.uint32)
    assert np.array_equal(ua[COL.SEED, :n][mesh], SC.advance(seed0, 4)[mesh]), f"{what}: a mesh pick takes the kind draw and three more"
    assert np.array_equal(ua[COL.SEED, :n][envk], SC.advance(seed0, 2)[envk]) and np.array_equal(ua[COL.SEED, :n][quadk], SC.advance(seed0, 3)[quadk])
    assert np.array_equal(ua[COL.SEED, :n][c.singular], seed0[c.singular]), f"{what}: a singular receiver draws nothing"
    if den == 3:
        assert envk.sum() > 100 and quadk.sum() > 100
        in_shadow = np.zeros(ws.n_tasks, bool); in_shadow[qa[Q.SHADOW]] = True
        for k, sel in ((1.0 / 3.0, envk), (1.0 / 3.0, quadk)):
            s = sel & in_shadow[:n]
            assert s.sum() > 0 and (a[0][COL.LAST_PICK_PROB, :n][s] == F(F(1.0) / F(3.0))).all(), f"{what}: the kind probability stored is 1 / den"
    # the shadow queue and shadowRayBlocked, exact where cosLight is decided
    margin = 1e-5
    lit, dark = mesh & (r["cosLight"] > margin), mesh & (SC._dot(*(_ng_and_L(S, g))) > margin)
    in_shadow = np.zeros(ws.n_tasks, bool); in_shadow[qa[Q.SHADOW]] = True
    assert in_shadow[:n][lit].all() and not in_shadow[:n][dark].any(), f"{what}: shadow-queue membership"
    assert (ua[COL.SHADOW_BLOCKED, :n][dark] == 1).all(), f"{what}: a lamp seen from behind blocks"
    assert lit.sum() > 200 and dark.sum() > 20
    # the stored sample against float64
    bounds = WC.sample_bounds(r)
    worst = {}
    for name, (col, k) in WC.SAMPLE_COLS.items():
        got = a[0][col:col + k, :n].T.astype(np.float64)
        ref = np.asarray(r[name], np.float64).reshape(n, k)
        bnd = np.broadcast_to(bounds[name], (n, k))
        err = np.abs(got - ref)[lit]
        ok = err <= bnd[lit]
        with np.errstate(all="ignore"):
            worst[name] = float(np.max(np.where(err > 0, err / np.maximum(bnd[lit], 1e-300), 0.0))) if err.size else 0.0
        assert ok.all(), f"{what}: {name} off float64 on {int((~ok).sum())} paths, worst {worst[name]:.3g} of the bound"
    print(f"{what}: largest error / bound per column {worst}")
    # every column the sample does not own: the input's bits, but the normal logic turns toward the ray (the option-off pass does the same)
    off.set_params(p)
    driver.reset_renderer(off)
    off.state_import(st); off.clear_queues()
    off.wf_logic(False)
    b = LC.snapshot(off)
    ub = b[0].view(np.uint32)
    own = {COL.SEED, COL.SHADOW_BLOCKED}
    for col, k in WC.SAMPLE_COLS.values():
        own |= set(range(col, col + k))
    for col in COLS:
        if col not in own:
            assert np.array_equal(ua[col, :n], ub[col, :n]), f"{what}: column {common.colname(col)} differs from the option-off pass"
    qb = queue_sets(b)
    for qi in (Q.RAYGEN,) + MATERIAL_QUEUES:
        assert np.array_equal(qa[qi], qb[qi]), f"{what}: queue {qi} differs from the option-off pass"
    if cfg == "none":
        assert np.array_equal(ub[COL.SEED, :n][nonsing], SC.advance(seed0, 1)[nonsing]), "option off, no light: the kind draw alone"
    # the shadow rays: traced with useAreaLight = 0, so no mesh shadow ray meets the parametric quad (the shadow kernels test it first, and the
    # brute force knows triangles only); from here on the other two kinds are off, so that nothing but the stored sample adds to Ei
    p_none = S.params(n, mode, **WC.LIGHTS["none"])
    on.set_params(p_none)
    on.wf_shadow()
    on.finish()
    blocked = on.state_export().view(np.uint32)[COL.SHADOW_BLOCKED, :n]
    sure = lit & g.robust
    assert sure.sum() > 200 and np.array_equal(blocked[sure] != 0, g.occluded[sure]), f"{what}: shadowRayBlocked against the brute force's any-hit"
    veiled = sure & np.isin(g.k, ws.c.k_of["veiled"])
    assert veiled.sum() >= 8 and not blocked[veiled].any(), "the veil 3 mm before a lamp lies past 0.995 |L|: it does not occlude"
    assert g.occluded[sure].sum() > 20, "some lamps are hidden"
    # the consumed sample: materials, extend, then the option-off plain pass (oracle-exact; it adds nothing for the lamp the new ray may hit)
    # (the extension rays are traced under the configuration's own parameters again: with the quad on they may meet it)
    on.set_params(p)
    on.wf_materials(); on.wf_extend(); on.clear_queues()
    mid = on.state_export().copy()
    off.set_params(p_none)
    off.state_import(mid); off.clear_queues()
    off.wf_logic(False)
    off.finish()
    out = off.state_export()
    # the consume step weighs with the STORED kind probability: pdf_a_to_w(...) (1 / den) on both sides of the MIS weight and under the
    # contribution, which is mesh_light_step_cases' restatement with every pick scaled by 1 / den
    kind = float(F(1.0) / F(den))
    v = SC.sampled_verdict(S, c, (tab[0], tab[1], np.asarray(tab[2], np.float64) * kind, tab[3]), g, mode)
    keep = mesh | c.singular | ~(c.T != 0).any(1)
    v.decided &= keep
    v.silent &= keep
    check_ei(v, out[list(EI), :n].T.astype(np.float64), u0[list(EI), :n], out.view(np.uint32)[list(EI), :n], f"{what}: the consumed sample", c.label)
    assert (v.decided & ~v.silent).sum() > (300 if den == 1 else 150)
    # ---- the MESH instance consumes (4.2.2 group C).  One wf_logic of the ON context adds, in this order, the implicit hit of the new vertex
    # (a lamp with its MIS weight, the environment with the corrected one, the quad) and the consumed sample.
    def logic2(edit, params):
        s2 = mid.copy()
        edit(s2)
        on.set_params(params)
        on.state_import(s2); on.clear_queues()
        on.wf_logic(False)
        on.finish()
        return on.state_export().copy()

    def alone(s2):                                                          # prior 0, and a vertex that adds nothing: a miss with the environment off
        s2[list(EI), :n] = 0.0
        s2.view(np.int32)[COL.HIT_I, :n] = -1
        s2.view(np.uint32)[COL.AREA_LIGHT_HIT, :n] = 0

    def without_the_sample(s2):
        s2.view(np.uint32)[COL.SHADOW_BLOCKED, np.nonzero(mesh)[0]] = 1
    full, bare, lone = logic2(lambda s2: None, p), logic2(without_the_sample, p), logic2(alone, p_none)
    # step 1: dEi = Ei of the lone run (0 + x is x) against float64, no prior to lean on
    import copy
    c0 = copy.copy(c)
    c0.Ei = np.zeros_like(c.Ei)
    v0 = SC.sampled_verdict(S, c0, (tab[0], tab[1], np.asarray(tab[2], np.float64) * kind, tab[3]), g, mode)
    m = mesh & v0.decided
    print(f"{what}: group C, {int((mesh & ~v0.decided).sum())} of {int(mesh.sum())} mesh picks undecided with no prior")
    assert (mesh & ~v0.decided).sum() <= SC.UNDECIDED_CAP * mesh.sum()
    v0.decided = m
    v0.silent = v0.silent & m
    check_ei(v0, lone[list(EI), :n].T.astype(np.float64), np.zeros((3, n), np.uint32), lone.view(np.uint32)[list(EI), :n], f"{what}: group C, dEi alone", c.label)
    # step 2: the sum
    e_full, e_bare, e_lone = (x[list(EI), :n].T.astype(F) for x in (full, bare, lone))
    total = (e_bare + e_lone).astype(F)
    dist = np.where(m[:, None], MR.ulp_diff(e_full, total), 0).max(1)
    wi = int(np.argmax(dist))
    others = (e_bare != c.Ei.astype(F)).any(1)
    print(f"{what}: group C, Ei is at most {dist.max()} ulp from fl32(Ei without the sample + dEi) (case {wi}, {c.label[wi]}); {int(m.sum())} decided, "
          f"the sample adds on {int((m & ~v0.silent).sum())}, the new vertex adds on {int((m & others).sum())}")
    assert (e_full[m] >= 0).all() and (total[m] >= 0).all()
    assert (dist <= 2).all(), f"{int((dist > 2).sum())} decided cases beyond 2 ulp of the sum, worst {dist.max()} at {wi} ({c.label[wi]})"
    assert (m & ~v0.silent).sum() > (300 if den == 1 else 150)
    if cfg == "both" and mode[1]:
        assert (m & others).sum() > 0.3 * m.sum(), "the other kinds add to Ei in the same pass"
    same_bits = (full.view(np.uint32)[list(EI), :n] == bare.view(np.uint32)[list(EI), :n]).all(0)
    assert same_bits[m & v0.silent].all(), "nothing consumed: Ei as without the sample"


def _ng_and_L(S, g):
    P3 = S.P[g.tri]
    cr = np.cross(P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0])
    return cr / np.linalg.norm(cr, axis=1, keepdims=True), g.L


@pytest.mark.parametrize("cfg", ["env", "quad", "both"])
def test_kind_draw_at_its_thresholds(cfg):
    """the one kind draw at both thresholds and the draws on either side: which kind is sampled, read from the number of draws taken"""
    S, tab, _, _, c, (on, _) = step_world()
    n = c.n
    edges = WC.kind_edges(cfg)
    i0 = int(np.nonzero(~c.singular & (c.T != 0).any(1) & (c.group == "random"))[0][0])
    ws = WC.WfSampled(c, cfg)
    seeds = ws.seed.copy()
    idx = np.arange(edges.size)
    seeds[idx] = [bc.seed_for_draw(1, v) for v in edges]
    ws.seed = seeds
    p = S.params(n, (1, 1), **WC.LIGHTS[cfg])
    on.set_params(p)
    driver.reset_renderer(on)
    st = ws.state(on.state_export().copy())
    for col in range(64):                                                    # the same receiver under every edge draw
        st[col, idx] = st[col, i0]
    st.view(np.uint32)[COL.SEED, idx] = seeds[idx].astype(np.uint32)
    st.view(np.uint32)[COL.PIXEL_INDEX, :] = np.arange(st.shape[1])
    on.state_import(st); on.clear_queues()
    on.wf_logic(False)
    on.finish()
    u = on.state_export().view(np.uint32)
    kind = WC.kind_of(cfg, edges)
    draws = np.array([2, 3, 4])[kind]                                        # environment 1 + 1, quad 1 + 2, lamps 1 + 3
    got = u[COL.SEED, idx]
    want = np.array([SC.advance(np.array([s], np.uint64), int(k))[0] for s, k in zip(seeds[idx], draws)], np.uint32)
    assert np.array_equal(got, want), f"{cfg}: kind draws {edges.tolist()} select {kind.tolist()}; seeds advanced differently at {np.nonzero(got != want)[0].tolist()}"
    assert set(kind.tolist()) == set(WC.kind_of(cfg, np.linspace(0, 1, 64, dtype=F)).tolist()), "every kind of the configuration is reached"


# ---- 5. / 6. / 7. renders by the wavefront loop
def render_wavefront(g, p, spp, cap=4000):
    """the benchmark loop until every pixel has at least spp samples: (pixels, moments)"""
    g.set_params(p)
    driver.reset_renderer(g)
    npix = int(p["width"]) * int(p["height"])
    for it in range(cap):
        driver.benchmark_iteration(g, npix)
        if it % 32 == 31 and g.read_pixels(0)[:, 3].min() >= spp:
            break
    px, mom = g.read_pixels(0), g.read_pixels(7)
    assert px[:, 3].min() >= spp and np.isfinite(px).all(), f"{px[:, 3].min()} samples after {cap} iterations"
    return px, mom


LF_SPP = 256
LF_TILE_SE = {(1, 1): 0.02, (1, 0): 0.02, (0, 1): 0.08}


@pytest.mark.parametrize("expl,impl", SC.MODES)
def test_lamp_over_floor_against_the_closed_form(expl, impl):
    d = SC.lamp_floor_scene()
    p = SC.lamp_floor_params(d, (expl, impl))
    W, H = SC.LF_W, SC.LF_H
    if "truth" not in _CACHE:
        _CACHE["truth"] = SC.lamp_floor_truth(p, 4)
    truth = _CACHE["truth"]
    g = ctx(2 * W * H, moments=1, mesh_lights=1, mesh_lights_wavefront=1)
    g.upload_scene(d)
    px, mom = render_wavefront(g, p, LF_SPP)
    g.close()
    mean, var = MR.tile_stats(px, mom, W, H)
    tt = SC.tile_means(truth)
    se = np.sqrt(var)
    z = np.abs(mean - tt) / se
    m = np.asarray(mom, np.float64).reshape(H, W, 4)
    pm = m[..., 0] / m[..., 3]
    pv = np.maximum(m[..., 1] / m[..., 3] - pm * pm, 0.0) / m[..., 3]
    all_mean, all_se = pm.mean(), np.sqrt(pv.sum()) / (W * H)
    z_all = abs(all_mean - truth.mean()) / all_se
    print(f"lamp over floor by the wavefront loop, sampleExpl {expl} sampleImpl {impl}: largest |mean - truth| / SE over {z.size} tiles {z.max():.2f}, "
          f"whole image {z_all:.2f}; relative SE of a tile {(se / tt).min():.4f} .. {(se / tt).max():.4f}, of the image {all_se / truth.mean():.5f}; "
          f"image mean {all_mean:.5f} against {truth.mean():.5f}; samples per pixel {px[:, 3].min():.0f} .. {px[:, 3].max():.0f}")
    assert all_se / truth.mean() <= 0.003 and (se / tt).max() <= LF_TILE_SE[(expl, impl)]
    assert (z <= 5.0).all() and z_all <= 5.0


W6, H6, SPP6 = 48, 32, 256
QUAD6 = dict(pos=(0.0, 2.5, 0.0), N=(0.0, -1.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))      # above every lamp: no ray from a surface to a lamp crosses it


def params6(d, mode):
    p = MC.render_params(d, W6, H6, mode, useEnvMap=1, useAreaLight=1, envMapStrength=0.5, maxBounces=8)
    for k in ("pos", "N", "right", "up"):
        p["areaLight"][k]["x"], p["areaLight"][k]["y"], p["areaLight"][k]["z"] = QUAD6[k]
    return p


@pytest.mark.parametrize("expl,impl", [(1, 1), (1, 0)])
def test_against_the_microkernel_with_three_kinds_of_light(expl, impl):
    """the microkernel integrator (closed-form- and float64-tested) is the reference: environment map, quad and lamps together, den = 3.
    maxBounces = 8: the two integrators count their last vertex differently (4.2.3), and eight bounces in an open scene leave nothing there.

    Measured on the MI355X: MIS 3.99 SE, NEE only 2.04 SE.  (3.99 is one tile of this stream: the same comparison on other sample streams --
    3 and 5 paths per pixel in the wavefront loop, and 512 samples on both sides -- reads 2.56, 2.18 and 2.75; per-tile figures in DESIGN.md 4.2.3.)
    The MIS case is the one that found the reference's implicit environment weight,
    (lastPdfW pick) / (lastPdfW pick + directPdfW), not to be the complement of its NEE weight unless pick = 1: with that weight this case read
    24.45 SE, and the parent's code WITHOUT any lamp (both options off, environment map and quad on) 19.28 SE on the same scene (image mean
    0.4006 wavefront against 0.4578 microkernel; NEE only 2.03; quad alone 1.88 / 1.84, environment map alone 2.88 / 1.33).  The MESH instance
    weighs the implicit environment hit against pdf x kind probability instead (test_implicit_environment_weight); the
    instances without lamps keep the reference's weight, which the oracle pins."""
    d, _ = MC.three_lamps_scene(back_lamp=True)
    p = params6(d, (expl, impl))
    env = host.synthetic_sky(64, 32)
    a = ctx(W6 * H6, moments=1, mesh_lights=1)
    a.upload_scene(d); a.upload_envmap(env)
    driver.render_single(a, p, SPP6)
    ref = a.read_pixels(0), a.read_pixels(7)
    a.close()
    b = ctx(2 * W6 * H6, moments=1, mesh_lights=1, mesh_lights_wavefront=1)
    b.upload_scene(d); b.upload_envmap(env)
    q = p.copy(); q["useRoulette"] = 0
    got = render_wavefront(b, q, SPP6)
    b.close()
    z, ma, mb = MR.tile_z(ref, got, W6, H6)
    print(f"wavefront vs microkernel, sampleExpl {expl} sampleImpl {impl}: largest |A - B| / SE {z.max():.2f} over {z.size} tiles; "
          f"tile means {ma.min():.4f} .. {ma.max():.4f}")
    assert ma.max() > 0.05 and (ma > 0).sum() >= z.size // 2, "the scene must be lit"
    assert (z <= 5.0).all(), f"tiles {np.argwhere(z > 5.0).tolist()} differ by {z[z > 5.0]} standard errors"


def test_lamps_move():
    """flx_objects_pose of a lamp between two wavefront renders: the table is rebuilt, and the lit tile moves with the lamp"""
    mats = MC.RENDER_MATS + [MC.emissive((30.0, 30.0, 30.0))]
    tris = list(MC.FLOOR) + MC.quad((-1.0, 0.5, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.2, 0.2, 2, (0.0, -1.0, 0.0))
    d = MC.scene(tris, mats)
    obj = np.array([MC.NO_OBJECT] * len(MC.FLOOR) + [0, 0], np.uint32)
    W, H = 48, 32
    p = MC.render_params(d, W, H, (1, 1))
    g = ctx(2 * W * H, moments=1, mesh_lights=1, mesh_lights_wavefront=1)
    g.upload_scene(d)
    g.objects_define(d.tris, obj, 1)

    def brightest_column():
        px, mom = render_wavefront(g, p, 32)
        mean, _ = MR.tile_stats(px, mom, W, H)
        assert mean.max() > 0
        return int(np.unravel_index(np.argmax(mean), mean.shape)[1]), mean
    col0, m0 = brightest_column()
    X = np.array([[1.0, 0.0, 0.0, 2.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]], F)      # the lamp from x = -1 to x = +1
    g.objects_pose([0], X)
    members = np.nonzero(obj == 0)[0]
    d.tris[members] = host.pose_triangles(d.tris[members], X)
    dev, ref = g.mesh_lights_read(), host.mesh_light_table(d)
    for name, x, y in zip(("tris", "cdf", "pick"), dev, ref):
        assert x.tobytes() == y.tobytes(), f"after flx_objects_pose: {name} differs"
    col1, m1 = brightest_column()
    ncol = W // 8
    print(f"lamps move: brightest tile column {col0} -> {col1} of {ncol}")
    assert col0 < ncol // 2 <= col1, (col0, col1)
    g.close()
