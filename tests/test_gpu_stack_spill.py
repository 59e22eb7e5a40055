"""The traversal stacks' spill paths on the device, on rays that provably reach them (tests/stack_cases.py; the proof is the host-side
witness, asserted on the CPU in tests/test_stack_spill.py and again here for the very rays each test traces).

Covered: Stack::push / pop beyond LDS_LEVELS in k_extend, k_shadow, k_gbuffer<2>, k_mk_next_vertex, k_mk_sample_bsdf and their _list
instances; WStack::reserve / wstack_page_out / wstack_page_in and the page-in inside pop in k_extend4, k_shadow4 (both visit orders),
k_shadow4s (rays that suspend and page after they resume in another lane; rays too deep for a continuation record), both instances of
k_trace4r (a refilled lane resets stk.base) and k_gbuffer<4>; flx_upload_scene's sizing of the two spill buffers, re-sizing in one context,
the second buffer under an overlapped shadow kernel, every launcher's stride, and both refits.

What counts as correct: the oracle bit for bit and the float64 brute force (traversal_cases.BruteForce) on every ray -- every crafted ray is
decided; another device run only where a case says so.  Closest hit: test_gpu_wide._extend_flips reports zero flips (every hit record
bit-identical to the oracle's) and the triangle is the brute force's; any hit: shadowRayBlocked is the oracle's and the brute force's.
Each test prints the witness's peak depth, page-outs and page-ins per family next to its pass; a witness threshold that is not met fails."""
import numpy as np
import pytest
import common
import stack_cases as sc
import traversal_cases as tc
import reproject_reference as R
import test_gpu_wide
import test_stack_spill
from test_gpu_traversal_edges import VARIANTS
from common import COL
from fluctus_amd import host, driver, wire

pytestmark = pytest.mark.gpu
REFILLS = (16 | (32 << 8), 8 | (16 << 8), 48)
N_BIG = 64 * 300 + 37           # more 64-ray blocks than the persistent kernels have waves: their lanes are refilled from further blocks
N_SMALL = 64 * 3 + 37           # < 256
_cases = {}


class Case:
    """A scene, its mixed queue of n rays, the witness (thresholds asserted) and the brute force's answers, computed once."""

    def __init__(self, d, what, n, min_cycles=1, thresholds=True):
        self.d, self.what, self.n = d, what, n
        self.P = tc.tri_points(d)
        self.orig, self.dirs, self.tmax, self.fam = sc.mixed_queue(self.P, n)
        self.table = ""
        if thresholds:
            self.w = sc.witness(d, self.orig, self.dirs, self.tmax)
            self.table = sc.format_rows(f"{what}, {n} rays", sc.check_thresholds(self.w, self.fam, what, min_cycles))
        v = tc.BruteForce(self.P, self.orig, self.dirs, self.tmax).verdict(d)
        assert not v["uncovered"] and v["ext_decided"].all() and v["sh_decided"].all(), f"{what}: undecided rays (cap 0)"
        self.closest, self.blocked = v["closest"], v["blocked"]
        exp = sc.expected_hits(self.P, self.fam)
        assert np.array_equal(self.closest, exp[0]) and np.array_equal(self.blocked, exp[1])


def _case(name, n):
    if (name, n) not in _cases:
        _cases[(name, n)] = Case(sc.SCENES[name](), name, n, min_cycles=3 if name == "decks" else 1)
    return _cases[(name, n)]


def _ctxs(n):
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    return HipContext(n), OracleContext(n, threads=16)


def _setup(ctxs, d, env):
    p = tc.params(d, env)
    for c in ctxs:
        c.upload_scene(d); c.set_params(p); driver.reset_renderer(c)


def _variant(g, var, refill=None):
    opts = dict(VARIANTS[var])
    if refill is not None:
        opts["refill_extend" if var == "default" else "refill_shadow"] = refill
    for k in ("extend_tree", "shadow_tree"):
        g.set_option(k, opts.get(k, 4))
    g.set_option("refill_extend", opts.get("refill_extend", 16 | (32 << 8)))
    g.set_option("refill_shadow", opts.get("refill_shadow", -1))


def _closest(g, o, c, what):
    """the extension queue through the device and the oracle: zero flips, every hit record bit-identical, the brute force's triangle"""
    tc.load_rays(o, c.orig, c.dirs, c.tmax)
    common.sync(g, o)
    rays, flips = test_gpu_wide._extend_flips(g, o, what)
    assert rays == c.n and flips == 0, f"{what}: {flips} of {rays} closest hits differ from the oracle's"
    hg, _ = tc.hits(g, c.n)
    assert np.array_equal(hg, c.closest), f"{what}: {int((hg != c.closest).sum())} closest hits differ from the brute force's"


def _any(g, o, c, what):
    tc.load_rays(o, c.orig, c.dirs, c.tmax)
    common.sync(g, o)
    g.wf_shadow(); o.wf_shadow(); g.finish()
    _, bg = tc.hits(g, c.n)
    _, bo = tc.hits(o, c.n)
    assert np.array_equal(bg, bo), f"{what}: shadowRayBlocked differs from the oracle's on {int((bg != bo).sum())} of {c.n} rays"
    assert np.array_equal(bg, c.blocked), f"{what}: shadowRayBlocked differs from the brute force's on {int((bg != c.blocked).sum())} rays"
    return bg


def _all_variants(g, o, c, env):
    runs = 0
    for var in VARIANTS:
        for refill in (REFILLS if var != "binary" else (None,)):
            _variant(g, var, refill)
            what = f"{c.what}/{c.n}/env{env}/{var}/{refill}"
            _closest(g, o, c, what)
            _any(g, o, c, what)
            runs += 1
    return runs


# ---- 1. every traversal variant
@pytest.mark.parametrize("name", list(sc.SCENES))
def test_all_traversal_variants_on_spilling_rays(name):
    import torch
    c = _case(name, N_BIG)
    assert (N_BIG + 63) // 64 > torch.cuda.get_device_properties(0).multi_processor_count, "the persistent kernels would not refill from a further block"
    g, o = _ctxs(c.n)
    try:
        for env in (1, 0):                  # far -> near | last-slot-first any-hit order
            _setup((g, o), c.d, env)
            info = g.scene_info()
            assert info["nested"] == 1 and info["binary_depth"] > sc.LDS_LEVELS and info["wide_stack_bound"] > sc.WIDE_NO_PAGE
            assert _all_variants(g, o, c, env) == 2 * len(REFILLS) + 1
    finally:
        g.close(); o.close()
    print(c.table)


def test_all_traversal_variants_on_a_queue_below_256_rays():
    g, o = _ctxs(N_SMALL)
    try:
        for name in sc.SCENES:
            c = _case(name, N_SMALL)
            for env in (1, 0):
                _setup((g, o), c.d, env)
                _all_variants(g, o, c, env)
            print(c.table)
    finally:
        g.close(); o.close()


# ---- 2. k_shadow4s
@pytest.mark.parametrize("name", ["deck100", "decks"])
def test_split_any_hit_kernel_suspends_resumes_and_pages(name):
    """shadow_split k1 | k2 << 8: a ray whose budget runs out in front of an inner node with an unpaged stack below FLX_SPLIT_KEEP entries
    suspends into a continuation record and is resumed by another lane with its own spill column (budgets 1 and 3: every deep ray, 3 and
    9 entries; it pages after it resumes); one that is deeper or partly paged out keeps going (budget 8 on the single deck: 24 entries,
    base 16; on the decks of decks the hole rays have emptied the top deck by then and suspend after paging out and back in).  Equal to the
    unsplit kernel (the case's second reference: same query, cut across launches), the oracle and the brute force."""
    c = _case(name, N_BIG)
    g, o = _ctxs(c.n)
    try:
        for env, mode in ((1, "any_far_near"), (0, "any_last_slot")):
            _setup((g, o), c.d, env)
            _variant(g, "default")
            g.set_option("refill_shadow", 0)
            unsplit = _any(g, o, c, f"{name}/env{env}/unsplit")
            deep = np.isin(c.fam, [sc.FAMILIES.index(f) for f in sc.DEEP_IN[mode]])
            for split, budget, suspends in ((1, 1, True), (8 | (8 << 8), 8, False), (3 | (200 << 8), 3, True)):
                w = sc.wide_witness(c.d, c.orig, c.dirs, c.tmax, mode, budget)
                can = (w["susp_sp"] >= 0) & (w["susp_base"] == 0) & (w["susp_sp"] < 14)
                paged = (w["susp_sp"] >= 0) & (w["susp_base"] > 0)
                assert (w["page_outs"][deep] >= 1).all()
                if suspends:
                    assert can[deep].all(), f"{name}/env{env}/split {split}: a deep ray does not suspend"
                elif name == "deck100":
                    assert paged[deep].all(), f"{name}/env{env}/split {split}: a deep ray reaches the budget with an unpaged stack"
                else:       # decks: 8 visits end inside the top deck -- a hole ray has paged out and back in by then and suspends with what is pending below
                    assert can[deep & np.isin(c.fam, [1, 3])].all(), f"{name}/env{env}/split {split}: a hole ray does not suspend"
                g.set_option("shadow_split", split)
                got = _any(g, o, c, f"{name}/env{env}/split {split}")
                g.set_option("shadow_split", 0)
                assert np.array_equal(got, unsplit)
                print(f"{name} env{env} shadow_split {split:#x}: {int(can.sum())} rays suspend ({int((can & deep).sum())} of them page after resuming), "
                      f"{int(paged.sum())} reach the budget partly paged out and keep going")
    finally:
        g.close(); o.close()
    print(c.table)


# ---- 3. both spill buffers at once
@pytest.mark.parametrize("overlap", [2, 0])
def test_extension_and_shadow_kernels_back_to_back(overlap):
    """flx_wf_extend directly followed by flx_wf_shadow: with overlap 2 the shadow kernel runs on the second stream beside the extension
    kernel and pages through the second spill buffer; both queues hold deep rays.  Same answers as one by one."""
    c = _case("decks", N_BIG)
    g, o = _ctxs(c.n)
    try:
        for env in (1, 0):
            _setup((g, o), c.d, env)
            for var in ("default", "refill", "binary"):
                _variant(g, var)
                g.set_option("overlap", overlap)
                what = f"decks/env{env}/{var}/overlap {overlap}"
                tc.load_rays(o, c.orig, c.dirs, c.tmax)
                common.sync(g, o)
                g.wf_extend(); g.wf_shadow(); g.finish()
                o.wf_extend(); o.wf_shadow()
                sg, so = g.state_export().view(np.uint32), o.state_export().view(np.uint32)
                for col in test_gpu_wide.HIT_COLS + [COL.SHADOW_BLOCKED]:
                    assert np.array_equal(sg[col], so[col]), f"{what}: column {common.colname(col)} differs from the oracle's on {int((sg[col] != so[col]).sum())} paths"
                hg, bg = tc.hits(g, c.n)
                assert np.array_equal(hg, c.closest) and np.array_equal(bg, c.blocked), f"{what}: differs from the brute force"
            g.set_option("overlap", -1)
    finally:
        g.close(); o.close()
    print(c.table)


# ---- 4. / 5. a pinhole camera above the deck, looking down
W_CAM, H_CAM = 48, 40


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_cpu(tmp_path_factory.mktemp("stack_spill_gpu"))


def _camera_case(exe, lights=False):
    """deck41 under a narrow pinhole camera off the deck's centre: the pixel-centre rays fan through the solid and the hole halves.  lights:
    a small area light BELOW the deck facing up, under the solid half -- next-event rays from the top card run down through the whole deck --
    and the environment light."""
    d = sc.SCENES["deck41"]()
    P = tc.tri_points(d)
    top = P[:, :, 2].max()
    p = tc.params(d, int(lights))
    p["width"], p["height"] = W_CAM, H_CAM
    eye = np.array([1.0137, 0.9721, top + 8.0])
    wire.look_at(p, eye, eye - np.array([0.0, 0.0, 1.0]), fov=12.0)
    if lights:
        p["useAreaLight"], p["maxBounces"], p["envMapStrength"] = 1, 4, 1.5
        al = p["areaLight"]
        for k, v in (("pos", (0.6, 0.6, -2.0)), ("N", (0.0, 0.0, 1.0)), ("right", (1.0, 0.0, 0.0)), ("up", (0.0, 1.0, 0.0))):
            al[k]["x"], al[k]["y"], al[k]["z"] = v
        al["size"] = (0.05, 0.05)
    n = W_CAM * H_CAM
    dirs = R.centre_rays(exe, W_CAM, H_CAM, p["camera"])
    orig = np.repeat(np.array([[p["camera"]["pos"][k] for k in "xyz"]], np.float32), n, 0)
    return d, P, p, orig, dirs


def _deep_counts(d, orig, dirs, tmax, what, kernels=("binary_closest", "closest")):
    """witness of rays that are not crafted one by one: how many spill, how many come back"""
    out = {}
    for k in kernels:
        w = sc.binary_witness(d, orig, dirs, tmax, k == "binary_any") if k.startswith("binary") else sc.wide_witness(d, orig, dirs, tmax, k)
        outs = w["climbs"] if k.startswith("binary") else w["page_outs"]
        back = (outs >= 1) & (w["tri"] < 0) if k.startswith("binary") else w["page_ins"] >= 1
        out[k] = (int(w["peak"].max()), int((outs >= 1).sum()), int(back.sum()), int((outs == 0).sum()))
        print(f"{what} {k}: {orig.shape[0]} rays, deepest stack {out[k][0]}, {out[k][1]} spill, {out[k][2]} of them empty the stack again, {out[k][3]} stay in LDS")
    return out


def test_gbuffer_on_spilling_pixel_rays(exe):
    """k_gbuffer<2> and <4>: hit index and t bit for bit those of flx_wf_extend under extend_tree 2 and the brute force's triangle, from a
    context with one path per pixel and from one with fewer paths than pixels (the kernel strides, a lane's spill column serves several rays)"""
    d, P, p, orig, dirs = _camera_case(exe)
    n = W_CAM * H_CAM
    tmax = np.full(n, 3.0e38, np.float32)
    counts = _deep_counts(d, orig, dirs, tmax, "gbuffer deck41")
    for k, (peak, spill, back, lds) in counts.items():
        assert spill >= n // 4 and back >= n // 16 and lds >= 1, f"{k}: the pixel rays do not exercise the spill path: {counts[k]}"
    v = tc.BruteForce(P, orig, dirs, tmax).verdict(d)
    dec = v["ext_decided"]
    assert dec.sum() >= 0.95 * n
    from fluctus_amd.device import HipContext
    a, b = HipContext(n), HipContext(64 * 10 + 37)
    try:
        for g in (a, b):
            g.upload_scene(d); g.set_params(p)
        a.set_option("extend_tree", 2)
        tc.load_rays(a, orig, dirs, tmax)
        a.wf_extend(); a.finish()
        st = a.state_export()
        hi_, ht = st.view(np.int32)[COL.HIT_I][:n].copy(), st[COL.HIT_T][:n].copy()
        hit = hi_ >= 0
        assert not (dec & (hi_ != v["closest"])).any() and hit.sum() > n // 8 and (~hit).sum() > n // 8
        for g, who in ((a, "one path per pixel"), (b, "fewer paths than pixels")):
            for tree in (2, 4):
                g.set_option("extend_tree", tree)
                g.gbuffer(); g.finish()
                gb, _ = g.gbuffer_read(0)
                gi, gt = gb[:, 3].copy().view(np.int32), gb[:, 7]
                what = f"gbuffer tree {tree}, {who}"
                same = dec if tree == 4 else np.ones(n, bool)         # (an undecided ray may tie between the two visit orders)
                assert np.array_equal(gi[same], hi_[same]), f"{what}: {int((gi != hi_)[same].sum())} hit indices differ from the extension kernel's"
                assert np.array_equal(gt[same & hit].view(np.uint32), ht[same & hit].view(np.uint32)), f"{what}: t differs from the extension kernel's"
                assert (gi[dec] == v["closest"][dec]).all(), f"{what}: differs from the brute force"
                assert (gt[~hit & same] == -1).all()
    finally:
        a.close(); b.close()


def test_microkernel_integrator_on_spilling_rays(exe):
    """mk_reset, mk_raygen, two rounds of mk_next_vertex / mk_sample_bsdf, mk_splat in lockstep with the oracle, state and pixels bit-exact
    (the pattern of test_microkernel_lockstep_bit_exact), then again with a ragged list of active pixels (every third): the listed pixels equal
    the oracle's, the others keep their bytes.  The primary rays spill in k_mk_next_vertex; k_mk_sample_bsdf's shadow rays start on the top
    card and run down through the deck to the light below it."""
    from oracle.binding import OracleContext
    from fluctus_amd.device import HipContext
    d, P, p, orig, dirs = _camera_case(exe, lights=True)
    npix = W_CAM * H_CAM
    n = npix + 37
    env = host.synthetic_sky(64, 32)
    steps = [("raygen", lambda c: c.mk_raygen())] + [(k, f) for _ in range(2) for k, f in (("next_vertex", lambda c: c.mk_next_vertex()),
                                                                                        ("sample_bsdf", lambda c: c.mk_sample_bsdf()))] + [("splat", lambda c: c.mk_splat())]
    for listed in (None, np.arange(0, npix, 3, dtype=np.uint32)):
        g, o = HipContext(n), OracleContext(n, threads=8)
        try:
            for c in (g, o):
                c.upload_scene(d); c.upload_envmap(env); c.set_params(p); c.mk_reset()
            mask = np.ones(n, bool)
            if listed is not None:
                g.mk_active_write(listed)
                mask[:] = False; mask[listed] = True
            tag = "all pixels" if listed is None else "every third pixel"
            px0 = g.read_pixels(0).view(np.uint32).copy()
            witnessed = set()
            for name, fn in steps:
                s0 = o.state_export()
                if name == "next_vertex" and name not in witnessed:
                    # the witness, on the primary rays the kernel is about to trace
                    witnessed.add(name)
                    act = np.nonzero(mask[:npix])[0]
                    ro, rd = np.ascontiguousarray(s0[COL.ORIG:COL.ORIG + 3, act].T), np.ascontiguousarray(s0[COL.DIR:COL.DIR + 3, act].T)
                    cnt = _deep_counts(d, ro, rd, np.full(act.size, 3.0e38, np.float32), f"mk next_vertex ({tag})", ("binary_closest",))["binary_closest"]
                    assert cnt[1] >= act.size // 4 and cnt[2] >= act.size // 16, f"the primary rays do not spill: {cnt}"
                if name == "sample_bsdf" and name not in witnessed:
                    # next-event rays toward the light below the deck from the hit points on the top card: the quad's corners and centre (the
                    # footprint of every box is convex, so what holds for the corners holds for every sample of the quad)
                    witnessed.add(name)
                    hitp = np.nonzero(mask[:npix] & (s0.view(np.int32)[COL.HIT_I][:npix] == d.tris.size - 1) & (s0.view(np.uint32)[COL.AREA_LIGHT_HIT][:npix] == 0))[0]
                    assert hitp.size >= npix // 16, "too few primary hits on the top card"
                    ho = np.ascontiguousarray((s0[COL.P:COL.P + 3, hitp] - np.float32(1e-3) * s0[COL.DIR:COL.DIR + 3, hitp]).T)
                    for cx, cy in ((0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
                        L = np.array([0.6 + 0.05 * cx, 0.6 + 0.05 * cy, -2.0]) - ho.astype(np.float64)
                        ln = np.linalg.norm(L, axis=1)
                        w = sc.binary_witness(d, ho, np.ascontiguousarray(L / ln[:, None], np.float32), ln.astype(np.float32), True)
                        assert (w["peak"] > sc.LDS_LEVELS).all() and (w["tri"] >= 0).all(), "a shadow ray from the top card to the light does not spill"
                    print(f"mk sample_bsdf ({tag}): {hitp.size} next-event rays from the top card to the light, deepest stack {int(w['peak'].max())}")
                g.state_import(s0)
                fn(g); fn(o)
                sa, sb = g.state_export(), o.state_export()
                fails = common.state_diff(sa, sb, 0.0, 0.0, mask=mask)
                assert not fails, f"{tag}, {name}: " + "; ".join(fails[:4])
                assert np.array_equal(sa.view(np.uint32)[COL.PHASE][mask], sb.view(np.uint32)[COL.PHASE][mask])
                if listed is not None:
                    assert np.array_equal(sa.view(np.uint32)[:, ~mask], s0.view(np.uint32)[:, ~mask]), f"{tag}, {name}: an unlisted pixel's state changed"
            pg, po = g.read_pixels(0).view(np.uint32), o.read_pixels(0).view(np.uint32)
            assert np.array_equal(pg[mask[:npix]], po[mask[:npix]]), f"{tag}: pixels differ from the oracle's"
            assert np.array_equal(pg[~mask[:npix]], px0[~mask[:npix]]), f"{tag}: an unlisted pixel was written"
            assert po[:, 3].view(np.float32).sum() > 0
        finally:
            g.close(); o.close()


# ---- 6. re-sizing in one context
def test_spill_buffers_follow_the_scene_in_one_context():
    """shallow scene, deck41, deck100, deck41 uploaded into ONE context: the buffers grow and are kept, scene_info()["spill_levels"] follows
    the scene, the default variant equals the oracle and the brute force after every upload and, at the end, a fresh context."""
    from fluctus_amd.device import HipContext
    n = 64 * 20 + 37
    shallow = Case(sc.shallow_scene(), "two cards", n, thresholds=False)
    seq = [shallow, _case("deck41", n), _case("deck100", n), _case("deck41", n)]
    g, o = _ctxs(n)
    try:
        for c in seq:
            info_host = host.wide_tree_check(c.d)
            depth = c.d.tris.size - 1
            want = max(1, depth + 1 - sc.LDS_LEVELS)
            if info_host["max_stack"] > sc.WIDE_NO_PAGE:
                want = max(want, info_host["max_stack"] + 8)
            for env in (1, 0):
                _setup((g, o), c.d, env)
                info = g.scene_info()
                assert info["spill_levels"] == want and info["binary_depth"] == depth and info["wide_stack_bound"] == info_host["max_stack"], (c.what, info, want)
                _variant(g, "default")
                _closest(g, o, c, f"resize/{c.what}/env{env}")
                _any(g, o, c, f"resize/{c.what}/env{env}")
        c = seq[-1]
        sg = g.state_export()
        f = HipContext(n)
        try:
            _setup((f,), c.d, 0)
            _variant(f, "default")
            tc.load_rays(f, c.orig, c.dirs, c.tmax)
            f.wf_extend(); f.wf_shadow(); f.finish()
            sf = f.state_export()
            for col in [k for k in test_gpu_wide.HIT_COLS if k != COL.PATH_LEN] + [COL.SHADOW_BLOCKED]:
                assert np.array_equal(sf.view(np.uint32)[col][:n], sg.view(np.uint32)[col][:n]), f"a fresh context differs in column {common.colname(col)}"
        finally:
            f.close()
    finally:
        g.close(); o.close()
    print(seq[1].table); print(seq[2].table)


# ---- 7. refit
@pytest.mark.parametrize("name", ["deck41", "decks"])
def test_refitted_trees_still_spill_and_trace_right(name):
    """flx_update_triangles (the deck moved, its z spacing doubled), then flx_update_triangles_subset (every third card shifted by 0.25 in
    x): the re-aimed families meet the witness thresholds on the nodes host.refit_bvh / host.refit_bvh_subset give, and the device on its own
    refitted trees equals the oracle on those nodes and the brute force"""
    d0, steps = test_stack_spill.refit_steps(name)
    n = 64 * 20 + 37
    g, o = _ctxs(n)
    try:
        g.upload_scene(d0)
        for label, d, idx in steps:
            c = Case(d, f"{name} {label}", n, min_cycles=3 if name == "decks" else 1)
            if idx is None:
                g.update_triangles(d.tris)
            else:
                g.update_triangles_subset(d.tris[idx], idx)
            for env in (1, 0):
                p = tc.params(d, env)
                g.set_params(p); driver.reset_renderer(g)
                o.upload_scene(d); o.set_params(p); driver.reset_renderer(o)
                for var in ("default", "refill", "binary"):
                    _variant(g, var)
                    _closest(g, o, c, f"{c.what}/env{env}/{var}")
                    _any(g, o, c, f"{c.what}/env{env}/{var}")
            print(c.table)
    finally:
        g.close(); o.close()
