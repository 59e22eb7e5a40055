"""The restatement of tests/logic_step_cases.py checked on the CPU before the GPU tests lean on it: the scene holds what the cases need, the
classifier decides every named case and all but 3 % of each group in every configuration and sampling mode, the seeds give the draws they were
chosen for, the cases reach what they were built for, and the oracle's wf_logic -- the reference's arithmetic in fp32 -- run on the same
imported states satisfies every assertion tests/test_gpu_logic_steps.py makes on the device."""
import numpy as np
import pytest
import bsdf_cases as bc
import logic_step_cases as LC
from common import COL, Q
from fluctus_amd import driver

F = np.float32
CFGS = list(LC.CONFIGS)


@pytest.fixture(scope="module")
def S():
    return LC.scene()


def oracle_step(S, cfg, mode):
    """the oracle's wf_logic on the imported cases: (state in, state out, framebuffer, counters, queues)"""
    from oracle.binding import OracleContext
    c = LC.cases(cfg)
    n = c.n + LC.EXTRA
    o = OracleContext(n, threads=8)
    try:
        o.upload_scene(S.d)
        o.upload_envmap(S.env(cfg))
        o.set_params(S.params(n, cfg, mode))
        driver.reset_renderer(o)
        st = c.state(o.state_export().copy())
        o.state_import(st)
        o.clear_queues()
        o.wf_logic(False)
        cnt = np.array(o.get_counters(), copy=True)
        return st, o.state_export().copy(), np.array(o.read_pixels(0), copy=True), cnt, {q: o.queue_read(q).copy() for q in range(Q.NUM)}
    finally:
        o.close()


def test_scene_holds_what_the_cases_need(S):
    assert 300 <= S.d.tris.size <= 600
    assert set(int(t) for t in S.type) == set(bc.TYPES)
    for m in S.MAPPED:
        w, h = (int(x) for x in list(S.tex.desc[S.mapN[m]])[1:])
        assert (w & (w - 1)) and (h & (h - 1)), "the normal map is not a power of two wide or high"
    u = S.UV[S.FLAT]
    assert ((u[1] - u[0])[0] * (u[2] - u[0])[1] - (u[1] - u[0])[1] * (u[2] - u[0])[0]) == 0.0
    assert (S.Nv != S.Nv[:, :1]).any(), "per-vertex normals that differ within a triangle"
    for e, dom, black in zip(S.envs, S.dominant, S.black):
        rgb = np.asarray(e.rgb).reshape(e.h, e.w, 3)
        pdf = np.asarray(e.pdf)
        assert pdf[dom] == pdf.max() and pdf[dom] > 20 * np.median(pdf)
        assert all(e.prob[i] == 0 and pdf[i] == 0 and e.alias[i] != i for i in black)
        for row in (0, e.h - 1):
            assert np.unique(rgb[row, :, 0]).size > e.w // 2, "a pole row that is not uniform"
            assert (rgb[row] == 0).all(1).any() and (rgb[row] > 0).all(1).any()
    assert (S.envs[0].w, S.envs[0].h, S.envs[1].w, S.envs[1].h) == (16, 8, 12, 5)


@pytest.mark.parametrize("cfg", CFGS)
def test_cases_are_decided(S, cfg):
    c = LC.cases(cfg)
    assert 1500 <= c.n <= 6000 and (c.n + LC.EXTRA) % 64
    for mode in LC.MODES:
        v = LC.verdict(cfg, mode)
        share = LC.undecided_share(v, c.group)
        print(f"{cfg}, sampleExpl {mode[0]} sampleImpl {mode[1]}: undecided " + ", ".join(f"{g} {s:.4f}" for g, s in share.items()))
        assert all(s <= LC.UNDECIDED_CAP for s in share.values()), share
        assert v.decided[c.named].all(), f"named cases undecided: {np.unique(c.label[c.named & ~v.decided]).tolist()}"
    # the named quirk is undecided where it bites (MIS on), by the classifier's verdict
    v = LC.verdict(cfg, (1, 1))
    q = (c.label == "-y pole") & v.info["mis_env"]
    if LC.CONFIGS[cfg]["useEnvMap"]:
        assert q.any() and not v.decided[q].any()


@pytest.mark.parametrize("cfg", CFGS)
def test_seeds_give_their_draws(S, cfg):
    c = LC.cases(cfg)
    i = LC.verdict(cfg, (1, 1)).info
    C = LC.CONFIGS[cfg]
    for side, cmp_ in (("at", np.equal), ("above", np.greater), ("below", np.less)):
        for lb, cp in (("0.01", LC.CONT_LO), ("0.5", LC.CONT_HI)):
            m = c.label == f"roulette draw {side} contProb {lb}"
            assert m.sum() == 3 and cmp_(i["r_roul"][m], cp).all() and (np.abs(i["r_roul"][m] - cp) <= np.spacing(F(cp))).all()
            if C["useRoulette"]:
                assert (i["contProb"][m] == cp).all() and (i["stop"][m] == (side == "above")).all(), "the clamped contProb is exact: the draw decides"
    if C["useEnvMap"]:
        env = S.env(cfg)
        assert len(c.picks) >= 8
        for lb, val in c.picks.items():
            m = c.label == lb
            assert m.any() and i["pickEnv"][m].all() and (i["r1"][m].astype(F) == val).all(), lb
        last = env.w * env.h - 1
        for lb in ("pick draw = 1 - ulp (index clamp)", "pick draw = 1 (index clamp)"):
            if lb in c.picks:
                assert (i["slot"][c.label == lb] == last).all()
        if "pick draw = 1 (index clamp)" in c.picks:
            assert float(F(1.0) * F(env.w) * F(env.h)) == last + 1, "floor(r w h) is one past the table: the clamp works"
        if "pick draw = 0" in c.picks:
            assert (i["slot"][c.label == "pick draw = 0"] == 0).all()
        below = [lb for lb in c.picks if lb.endswith("below prob")]
        assert below or cfg == "both"
        for lb in below:
            at = lb.replace("below prob", "at prob")
            k = int(lb.split()[1].rstrip(":"))
            assert (i["slot"][c.label == lb] == k).all() and i["own"][c.label == lb].all()
            if at in c.picks:
                assert (i["slot"][c.label == at] == k).all() and not i["own"][c.label == at].any()
                assert float(c.picks[at]) - float(c.picks[lb]) <= max(2.0 ** -32, float(np.spacing(c.picks[lb]))), "neighbouring draws"
        dom = S.dominant[C["env"]]
        assert (i["texel"][np.char.endswith(c.label, "alias is the dominant texel")] == dom).all()
        assert (i["texel"][c.label == "the dominant texel's own slot"] == dom).all()
        m = np.char.endswith(c.label, "black, aliased")
        assert m.any() and not i["own"][m].any() and not np.isin(i["texel"][m], S.black[C["env"]]).any()
    if cfg == "env":
        m = c.label == "choice draw = 1: no light at all"
        assert m.any() and (i["r0"][m] == 1.0).all() and not (i["pickEnv"] | i["pickQuad"])[m].any() and i["nee"][m].all()
    if C["useAreaLight"]:
        assert len(c.quad_draws) >= (6 if cfg == "quad" else 3)
        for lb, (k, val) in c.quad_draws.items():
            m = c.label == lb
            assert i["pickQuad"][m].all() and (i["r1" if k == 2 else "r2"][m].astype(F) == val).all(), lb
    if cfg == "both":
        for lb, env_side in (("choice draw = 0.5", False), ("choice draw = 0.5 - ulp", True), ("choice draw = 0.5 + ulp", False)):
            m = c.label == lb
            assert m.sum() == 4 and (i["pickEnv"][m] == env_side).all() and (i["pickQuad"][m] != env_side).all(), lb


@pytest.mark.parametrize("cfg", CFGS)
def test_cases_reach_what_they_were_built_for(S, cfg):
    c = LC.cases(cfg)
    C = LC.CONFIGS[cfg]
    v, v10, v01 = (LC.verdict(cfg, m) for m in LC.MODES)
    i, d = v.info, v.decided
    inside = lambda w, m: ((w > 0.02) & (w < 0.98) & m & d).sum()
    if C["useEnvMap"]:
        assert inside(i["w_env"], i["mis_env"]) > 100, "the implicit environment sample's MIS weight strictly between 0 and 1"
        assert (i["pickEnv"] & i["own"] & d).sum() > 50 and (i["pickEnv"] & ~i["own"] & d).sum() > 50, "both alias branches"
        assert (i["pickEnv"] & d & (i["cosTh"] == 0)).sum() > 20 and (i["pickEnv"] & d & (i["cosTh"] > 0)).sum() > 50, "normals toward and away from L"
        assert (i["pickEnv"] & i["back"] & d).sum() >= 20, "light samples on back faces"
    if C["useAreaLight"]:
        assert inside(i["w_q"], i["mis_q"]) >= 10, "the implicit quad hit's MIS weight strictly between 0 and 1"
        assert (i["pickQuad"] & ~i["lit"] & d).sum() >= 20, "receivers behind the quad: shadowRayBlocked set, no queue entry"
        assert (i["pickQuad"] & i["lit"] & d).sum() > 200
        m = c.label == "nearly in the quad's plane"
        assert (m & d & i["lit"]).sum() >= 10, "some of them close enough to the plane to be undecided, some decided"
    assert inside(i["w_c"], i["cons"]) > 100, "the consumed sample's MIS weight strictly between 0 and 1"
    assert (v10.info["w_c"] == 1).all() and not v10.info["mis_env"].any() and not v01.info["mis_env"].any() and not v01.info["mis_q"].any()
    assert not v01.info["nee"].any() and v.info["nee"].sum() > 500
    if C["useRoulette"]:
        assert (i["roul"] & i["stop"] & d).sum() >= 10 and (i["roul"] & ~i["stop"] & d).sum() >= 10, "roulette ends and keeps paths"
        for lb in ("lum < 0.01", "lum inside", "lum > 0.5"):
            assert (c.label == f"roulette, {lb}").sum() == 12
        assert (i["contProb"][c.label == "roulette, lum < 0.01"] == LC.CONT_LO).all() and (i["contProb"][c.label == "roulette, lum > 0.5"] == 0.5).all()
        m = c.label == "roulette, lum inside"
        assert ((i["contProb"][m] > LC.CONT_LO) & (i["contProb"][m] < 0.5)).all()
        assert (v.changed["T"] == i["roul"]).all() and (v.out["T"][i["roul"]] > c.T[i["roul"]]).all(), "T after the roulette division"
    else:
        assert not v.changed["T"].any() and v.exact["terminate"][c.pathLen >= LC.MAX_BOUNCES + 1].all()
    assert not v.exact["terminate"][(c.label == f"pathLen {LC.MAX_BOUNCES}")].any()
    m = np.char.startswith(c.label, "pathLen 0")
    assert m.sum() == 12 and v.exact["terminate"][m].all() and not v.exact["splat"][m].any(), "pathLen 0 terminators do not splat"
    assert (i["turn"] & d).sum() > 100 and not i["turn"][c.label == "uv determinant 0"].any() and (c.label == "uv determinant 0").sum() == 36
    mapped = c.group == "normal map"
    assert (i["turn"] & i["back"] & d & mapped).sum() >= 10 and (i["turn"] & ~i["back"] & d & mapped).sum() >= 10, "the turned normal decides the face"
    assert (i["turn"] & i["nee"] & d & (i["pickEnv"] | i["lit"])).sum() >= 50, "the turned normal feeds lastCosTh"
    assert (v.exact["list"][:, None] == np.array([Q.DIFFUSE, Q.GLOSSY, Q.GGX_REFL, Q.GGX_REFR, Q.DELTA])[None, :]).sum(0).min() >= 40, "every material queue"
    silent = d & ~v.changed["Ei"]
    assert silent.sum() > 100 and (d & v.changed["Ei"]).sum() > 300


@pytest.mark.parametrize("expl,impl", LC.MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_oracle_satisfies_the_gpu_assertions(S, cfg, expl, impl):
    """the reference's own arithmetic stays inside the tolerances and the cap"""
    c, v = LC.cases(cfg), LC.verdict(cfg, (expl, impl))
    st, out, px, cnt, qs = oracle_step(S, cfg, (expl, impl))
    what = f"oracle, {cfg}, sampleExpl {expl} sampleImpl {impl}"
    worst, label = LC.check(v, c, st, out, px, cnt, qs, what)
    print(f"{what}: largest error / tolerance {worst:.3f} ({label}); {int(v.decided.sum())} of {c.n} decided")
    assert np.isfinite(out[COL.EI:COL.EI + 3, :c.n]).all()


def test_named_quirk_on_the_oracle(S):
    """a miss toward exactly (0, -1, 0) with MIS on: Ei comes back NEGATIVE and finite (see the module docstring of logic_step_cases)"""
    c, v = LC.cases("both"), LC.verdict("both", (1, 1))
    st, out, px, cnt, qs = oracle_step(S, "both", (1, 1))
    q = np.nonzero((c.label == "-y pole") & v.info["mis_env"])[0]
    ei = out[COL.EI:COL.EI + 3, q].T
    print(f"the -y pole with a MIS weight: Ei {ei.tolist()}, the float64 restatement {v.out['Ei'][q].tolist()}")
    assert q.size == 3 and np.isfinite(ei).all() and (ei < 0).all(), "envMapPdf is negative on the last row when v rounds to 1"
    plain = np.nonzero((c.label == "-y pole") & ~v.info["mis_env"])[0]
    assert (out[COL.EI:COL.EI + 3, plain] > 0).all() and v.decided[plain].all(), "without the weight the pole is an ordinary lookup"


# ---- the RAW chain's cases: rays, the float64 commit, then the same logic step
RAY_SETS = [(False, None), (False, 256), (True, None)]


@pytest.mark.parametrize("all_diffuse,pad_to", RAY_SETS)
def test_ray_cases_and_the_oracle_chain(all_diffuse, pad_to):
    """what tests/test_gpu_logic_steps.py::test_raw_chain asserts on the device, on the oracle: extension rays, then logic, genRays and the
    material kernels back to back -- continuing paths through the exported state, terminating ones through their pixel, regenerated ones by
    count and pixel word"""
    from oracle.binding import OracleContext
    S, c = LC.scene(all_diffuse), LC.ray_cases(all_diffuse, pad_to)
    n = c.n_tasks
    assert (n % 256 == 0) == (pad_to == 256) and 1000 <= c.n <= 3000
    assert c.robust.mean() > 0.97
    for group, wins in (("quad", True), ("ground before the quad", False), ("sphere behind the quad", True)):
        m = (c.group == group) & c.robust
        assert m.sum() >= 40 and (c.quad_wins[m] == wins).mean() > 0.9, group
    assert (c.hit[c.group == "sphere behind the quad"] >= 0).mean() > 0.5, "a triangle behind the quad"
    assert (c.hit[c.group == "sky"] < 0).all()
    if all_diffuse:
        assert (S.type == bc.BXDF.DIFFUSE).all()
    o = OracleContext(n, threads=8)
    try:
        o.upload_scene(S.d)
        o.upload_envmap(S.env("both"))
        for mode in LC.MODES:
            v = LC.ray_verdict(all_diffuse, pad_to, mode)
            share = LC.undecided_share(v, c.group)
            what = f"oracle, rays (all diffuse {all_diffuse}, padded to {pad_to}), sampleExpl {mode[0]} sampleImpl {mode[1]}"
            print(f"{what}: undecided " + ", ".join(f"{g} {s:.4f}" for g, s in share.items()))
            assert all(s <= LC.UNDECIDED_CAP for s in share.values()), share
            p = S.params(n, "both", mode, quad=c.quad)
            o.set_params(p)
            driver.reset_renderer(o)
            st = LC.load_rays(o, c)
            o.wf_extend()
            hit = o.state_export().view(np.int32)[COL.HIT_I, c.index]
            on = c.robust & ~(c.quad_wins & bool(mode[1]))
            assert np.array_equal(hit[on], c.hit[on]), "the float64 nearest hit is the traversal's on the robust rays"
            o.clear_queues()
            o.wf_logic(False)
            lone = LC.snapshot(o)
            worst, label = LC.check(v, c, st, *lone, what + ", logic alone", index=c.index)          # (T and the seed too)
            o.wf_raygen(); o.wf_materials()
            out = LC.snapshot(o)
            worst2, label2 = LC.check(v, c, st, *out, what, chained=True, index=c.index)
            cnt = LC.check_regenerated(v, c, out[0], out[2], out[3], n, int(p["width"]) * int(p["height"]), what)
            print(f"{what}: largest error / tolerance {max(worst, worst2):.3f} ({label if worst >= worst2 else label2}); {int(v.decided.sum())} of {c.n} decided, "
                  f"{cnt} paths regenerated")
            i = v.info
            if mode == (1, 1):
                assert (i["quad"] & v.decided).sum() >= 100 and ((i["w_q"] < 0.98) & i["mis_q"] & v.decided).sum() >= 10
                assert (i["miss"] & v.decided).sum() >= 100 and (i["turn"] & v.decided).sum() >= 30 and (i["back"] & v.decided).sum() >= 100
    finally:
        o.close()


def test_atan2_at_the_signed_zeros():
    """include/flx_math.h atan2f_ against OpenCL 1.2 s7.5.1 (= C99 F.9.1.4) where directionToUV meets it on exact axis directions: found by
    the miss group (a ray along +-y, one toward (-0, 0, 1)) -- device and oracle shared the departure, so parity could not see it"""
    from oracle.binding import math_array
    y = np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 1.0, -1.0], F)
    x = np.array([-0.0, -0.0, 0.0, 0.0, -1.0, -1.0, 1.0, 1.0, 0.0, 0.0, -0.0, -0.0], F)
    got = math_array(3, y, x).view(F)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    assert np.allclose(got, want, rtol=3e-7, atol=0), (got, want)
    nz = want != 0                                   # (the sign of a zero result does not reach u = 1 + atan2 / pi)
    assert np.array_equal(np.signbit(got[nz]), np.signbit(want[nz])), (got, want)
