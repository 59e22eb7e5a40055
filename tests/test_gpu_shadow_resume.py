"""GPU: the split any-hit launch with its suspended rays finished in persistent waves (trace4r.hip: k_trace4r_resume).

Pass 1, k_shadow4s<ORDER, true>, traces every shadow ray under a budget of K node visits and parks the rays that are not done in 64-byte continuation
records; the resume kernel's waves refill their lanes from those records and finish them.  A ray's own sequence of node and leaf visits is k_shadow4's,
only cut at the suspension and continued in another lane of another kernel, so everything the launch leaves behind must be IDENTICAL to the unsplit
kernel's.  Three contexts get one and the same path state, queues and counters (common.sync from a fourth that produced them) and run flx_wf_shadow:

    a   shadow_split 0                         k_shadow4
    b   shadow_split K, shadow_resume 1        k_shadow4s + k_trace4r_resume
    c   shadow_split K, shadow_resume 0        k_shadow4s + k_shadow4s (one lane per record slot)

and are compared with == on shadowRayBlocked, on the whole exported state and on the queue counters.  How many rays suspended is read from the read-only
option "shadow_split_suspended" and asserted wherever a case is about rays that do (or do not) suspend.

Scenes: the reference's egyptcat.obj (tests/golden/egyptcat_scene.npz) under the night environment map, environment light only -- the far -> near visit
order, the parameters the split is the library's own choice for -- at 2^16 and 2^14 paths, and the deck of cards of tests/stack_cases.py (deck100: stacks
of 100 entries) with the crafted rays of tests/test_gpu_stack_spill.py, both visit orders."""
import numpy as np
import pytest
import common
import stack_cases as sc
import test_gpu_stack_spill as spill
from common import COL, Q
from fluctus_amd import driver

pytestmark = pytest.mark.gpu

W, H = 128, 128
NPIX = W * H
CHOSEN_K = 8                        # the library's choice under environment-only parameters (api.hip: FLX_SPLIT_DEFAULT)
LISTS = 256                         # sub-lists of continuation records (flx_trace4.h: FLX_SPLIT_LISTS)
_inputs = {}


def _egyptcat(area=0, name="egyptcat"):
    """the scene, environment-only parameters (area: with the area light too) and the night map.  name "kitchen": the small procedural kitchen of
    tests/test_gpu_lazy_commit.py (3 000 triangles, open to the sky: its shadow rays are a mix of blocked and free ones; the cat's are nearly all blocked)"""
    import bench
    from fluctus_amd import host, wire
    if name not in _inputs:
        if name == "egyptcat":
            d, p, _ = bench.build_workload(width=W, height=H, name="egyptcat")
        else:
            d = host.generate_scene("kitchen", 3000, 7)
            host.build_bvh(d, "binned")
            p = wire.default_params(W, H, d.world_radius, d.tris.size)
            wire.look_at(p, (0.0, 1.2, 2.6), (0.0, 0.2, 0.0), fov=60.0)
            p["maxBounces"], p["wfSeparateQueues"] = 8, 1
        _inputs[name] = (d, p, bench.night_env())
    d, p, env = _inputs[name]
    p = p.copy()
    p["useEnvMap"], p["useAreaLight"] = 1, int(area)
    return d, p, env


def _ctx(n, d, p, env, **options):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    g.upload_scene(d)
    if env is not None:
        g.upload_envmap(env)
    g.set_params(p)
    for k, v in options.items():
        g.set_option(k, v)
    driver.reset_renderer(g)
    return g


def _trio(n, d, p, env, k, limit=0):
    return [_ctx(n, d, p, env, shadow_split=0), _ctx(n, d, p, env, shadow_split=k, shadow_resume=1, shadow_split_limit=limit),
            _ctx(n, d, p, env, shadow_split=k, shadow_resume=0, shadow_split_limit=limit)]


def _producer(n, iterations=4, name="egyptcat"):
    """a context in the steady state of the wavefront loop, stopped in front of flx_wf_shadow: its shadow queue and path state are the inputs"""
    d, p, env = _egyptcat(name=name)
    src = _ctx(n, d, p, env, shadow_split=0)
    for _ in range(iterations):
        driver.benchmark_iteration(src, NPIX)
    src.wf_logic(False); src.wf_raygen(); src.wf_materials(); src.wf_extend()
    return src


def _shadow(src, ctxs, keep=None, what=""):
    """flx_wf_shadow in every context from src's state, the shadow queue cut to its first `keep` entries; compares; returns (queue length, suspended in b, in c)"""
    out = []
    for g in ctxs:
        common.sync(g, src)
        cnt = g.get_counters(); g.finish()          # (valid after finish())
        cnt = np.array(cnt, copy=True)
        if keep is not None:
            cnt[Q.SHADOW] = min(int(keep), int(cnt[Q.SHADOW]))
            g.set_counters(cnt)
        g.wf_shadow(); g.finish()
        after = g.get_counters(); g.finish()
        out.append((g.state_export().view(np.uint32), np.array(after, copy=True), int(cnt[Q.SHADOW])))
    (sa, ca, qlen) = out[0]
    for (s, c, _), name in zip(out[1:], ("resume 1", "resume 0")):
        diff = sa[COL.SHADOW_BLOCKED] != s[COL.SHADOW_BLOCKED]
        assert not diff.any(), f"{what} {name}: shadowRayBlocked differs on {int(diff.sum())} of {qlen} rays"
        rows = np.flatnonzero((sa != s).any(axis=1))
        assert rows.size == 0, f"{what} {name}: exported state differs in columns {[common.colname(int(r)) for r in rows]}"
        assert (ca == c).all(), f"{what} {name}: counters {ca} vs {c}"
    susp = [g.get_option("shadow_split_suspended") for g in ctxs]
    assert susp[0] == 0 and susp[1] == susp[2], f"{what}: suspended {susp}"
    return qlen, susp[1], sa[COL.SHADOW_BLOCKED]


def _close(ctxs):
    for g in ctxs:
        g.close()


# ---- 1. budgets, queue lengths, list lengths
@pytest.mark.parametrize("name,n,k", [("egyptcat", 1 << 16, 1), ("egyptcat", 1 << 16, 2), ("egyptcat", 1 << 16, 8), ("egyptcat", 1 << 14, 8), ("egyptcat", 1 << 14, 1),
                                      ("kitchen", 1 << 16, 1), ("kitchen", 1 << 16, 8), ("kitchen", 4096 + 37, 1), ("kitchen", 192, 1)])
def test_resumed_rays_are_bit_identical(name, n, k):
    """K = 1 (at least half of the rays suspend), 2 and 8 (some do); the whole shadow queue, an empty one, one shorter than a wave, and one that is no
    multiple of 64.  At 2^14 paths pass 1 has 256 waves, one per sub-list, so every list holds fewer records than one wave's 64 (K = 8: a handful each);
    with the queue cut to 5 blocks + 37 only six lists hold any and 250 are empty; with 37 rays one list does.  The kitchen's rays end both ways.  Below
    2^14 paths (4 133 and 192: 65 and 3 pass-1 waves) the resume kernel's grid of one wave per sub-list is larger than the number of 64-lane columns the
    spill areas have; the waves beyond find their lists empty."""
    d, p, env = _egyptcat(name=name)
    src = _producer(n, name=name)
    ctxs = _trio(n, d, p, env, k)
    try:
        assert [g.get_option("shadow_split") for g in ctxs] == [0, k, k]
        qlen, susp, blocked = _shadow(src, ctxs, None, f"{name} n {n} K {k} whole queue")
        nb = int((blocked[src.queue_read(Q.SHADOW)[:qlen]] != 0).sum())
        print(f"{name} n {n} K {k}: {qlen} shadow rays, {susp} suspended ({susp / max(1, qlen):.3f}), {nb} of them blocked")
        assert qlen > n // 4, "the steady state has too few shadow rays to say anything"
        if name == "kitchen" and n >= 4096:
            assert qlen // 100 < nb < qlen - qlen // 100,"the kitchen's shadow rays should be a mix of blocked and free ones"
        if k == 1:
            assert 2 * susp >= qlen, f"K 1: {susp} of {qlen} rays suspended, fewer than half"
        else:
            assert susp > 0, f"K {k}: no ray suspended"
        if n == 1 << 14:
            assert susp <= 64 * LISTS       # (one pass-1 wave per list)
        for keep in (0, 37, 64 * 5 + 37):
            ql, s, _ = _shadow(src, ctxs, keep, f"n {n} K {k} queue cut to {keep}")
            print(f"  queue cut to {ql}: {s} suspended")
            assert ql == min(keep, qlen) and s <= ql
            if keep == 0:
                assert s == 0
            elif k == 1:
                assert 2 * s >= ql
    finally:
        _close(ctxs + [src])


# ---- 2. full sub-lists
def test_full_sub_lists_finish_in_pass_one():
    """shadow_split_limit 5: a sub-list takes five records; the rays beyond finish inside their pass-1 wave (overflow), the five are resumed.  At 2^16
    paths with K = 1 at least half of the rays want a record (test_resumed_rays_are_bit_identical asserts it), many times the 5 x 256 there are."""
    n = 1 << 16
    d, p, env = _egyptcat()
    src = _producer(n)
    ctxs = _trio(n, d, p, env, 1, limit=5)
    try:
        qlen, susp, _ = _shadow(src, ctxs, None, "limit 5")
        print(f"limit 5: {qlen} shadow rays, {susp} records")
        assert qlen // 2 > 4 * 5 * LISTS, "too few rays for the lists to overflow"
        assert 0 < susp <= 5 * LISTS, f"{susp} records in {LISTS} lists of 5"
        ql, s, _ = _shadow(src, ctxs, 64 * 3 + 37, "limit 5, short queue")
        assert 0 < s <= 5 * 4
    finally:
        _close(ctxs + [src])


# ---- 3. deep stacks
@pytest.mark.parametrize("env", [1, 0])
def test_deep_stacks_suspend_resume_and_page(env):
    """deck100 (tests/stack_cases.py), the crafted rays of tests/test_gpu_stack_spill.py: with a budget of 1 every deep ray suspends with three stack
    entries and pages out to the resuming lane's own spill column; with a budget of 8 a deep ray stands on 24 entries, 16 of them paged out, has no record
    and keeps going in pass 1.  The witness (sc.wide_witness) says which rays suspend; the device must report exactly that many.  env 1: far -> near order,
    env 0: last-slot-first."""
    c = spill._case("deck100", spill.N_BIG)
    mode = "any_far_near" if env else "any_last_slot"
    d, p = c.d, spill.tc.params(c.d, env)
    deep = np.isin(c.fam, [sc.FAMILIES.index(f) for f in sc.DEEP_IN[mode]])
    src = _ctx(c.n, d, p, None, shadow_split=0)
    spill.tc.load_rays(src, c.orig, c.dirs, c.tmax)
    for k in (1, 8):
        w = sc.wide_witness(c.d, c.orig, c.dirs, c.tmax, mode, k)
        can = (w["susp_sp"] >= 0) & (w["susp_base"] == 0) & (w["susp_sp"] < 14)
        paged = (w["susp_sp"] >= 0) & (w["susp_base"] > 0)
        assert (w["page_outs"][deep] >= 1).all()
        if k == 1:
            assert can[deep].all(), "a deep ray does not suspend under a budget of 1"
        else:
            assert paged[deep].all() and not can[deep].any(), "a deep ray reaches the budget of 8 with an unpaged stack"
        ctxs = _trio(c.n, d, p, None, k)
        try:
            qlen, susp, blocked = _shadow(src, ctxs, None, f"deck100 env {env} K {k}")
            print(f"deck100 env {env} K {k}: {qlen} rays, witness {int(can.sum())} suspend ({int((can & deep).sum())} deep), {int(paged.sum())} too deep; device {susp}")
            # ray i is queue entry i, its pass-1 wave i // 64 appends to list (i // 64) % 256, and a list has ((n / 2 / 256) + 64) & ~63 slots
            # (api.hip: splitCapA -- 64 here, and 45 lists serve two waves): the rays that find their list full finish in pass 1
            cap = ((c.n // 2 // LISTS) + 64) & ~63
            per_list = np.bincount((np.flatnonzero(can) // 64) % LISTS, minlength=LISTS)
            want = int(np.minimum(per_list, cap).sum())
            print(f"  {int((per_list > cap).sum())} lists overflow their {cap} slots: {want} records")
            assert qlen == c.n and susp == want
            assert np.array_equal(blocked[:c.n] != 0, c.blocked), "shadowRayBlocked differs from the brute force's"
        finally:
            _close(ctxs)
    src.close()


# ---- 4. iterations in a row, and a value with a second budget
def test_three_iterations_in_a_row_and_the_three_launch_chain():
    """Free-running steps of the wavefront loop (the any-hit launch on the second stream, beside the closest-hit kernel): three in a row, so that both
    counter sets are used and the one pass 1 zeroes is the one the next launch appends to -- the count of suspended rays is compared after every step, a
    stale counter would show there and in the results.  The fourth context has a second budget, 8 | 12 << 8: it takes the three-launch chain."""
    n = 1 << 16
    d, p, env = _egyptcat()
    src = _producer(n, iterations=3)
    ctxs = _trio(n, d, p, env, 2) + [_ctx(n, d, p, env, shadow_split=8 | (12 << 8))]
    try:
        assert ctxs[3].get_option("shadow_split") == 8 | (12 << 8)
        for g in ctxs:
            common.sync(g, src)
            g.clear_queues()
        for it in range(3):
            cnts = [driver.benchmark_iteration(g, NPIX) for g in ctxs]
            states = [g.state_export().view(np.uint32) for g in ctxs]
            for g, cn, s in zip(ctxs[1:], cnts[1:], states[1:]):
                assert (cn == cnts[0]).all(), f"step {it}: counters {cnts[0]} vs {cn}"
                rows = np.flatnonzero((states[0] != s).any(axis=1))
                assert rows.size == 0, f"step {it}, shadow_split {g.get_option('shadow_split')} resume {g.get_option('shadow_resume')}: state differs in {[common.colname(int(r)) for r in rows]}"
            susp = [g.get_option("shadow_split_suspended") for g in ctxs]
            print(f"step {it}: {int(cnts[0][Q.SHADOW])} shadow rays, suspended {susp}")
            assert susp[0] == 0 and susp[1] == susp[2] and 0 < susp[1] <= int(cnts[0][Q.SHADOW]) and 0 < susp[3] <= susp[1]
        assert common.fb_close(ctxs[0].read_pixels(0), ctxs[1].read_pixels(0))
    finally:
        _close(ctxs + [src])


# ---- 5. the default
def test_the_library_chooses_the_split_from_the_light():
    """-1, the initial value: K where every shadow ray runs toward the environment light, 0 with an area light; an explicit value holds under both, 0
    included; -1 restores the choice.  The option reports the EFFECTIVE value; under the choice the launch really splits (rays suspend)."""
    n = 1 << 14
    d, p_env, env = _egyptcat(0)
    _, p_area, _ = _egyptcat(1)
    g = _ctx(n, d, p_env, env)
    try:
        assert g.get_option("shadow_split") == CHOSEN_K and g.get_option("shadow_resume") == 1
        for _ in range(3):
            driver.benchmark_iteration(g, NPIX)
        assert g.get_option("shadow_split_suspended") > 0 and g.get_option("shadow_split_fallback") == 0
        # the option reports what flx_wf_shadow launches: nothing splits under the persistent any-hit kernel, the binary tree or the counting kernels
        for name, on, off in (("refill_shadow", 16 | (32 << 8), -1), ("shadow_tree", 2, 4)):
            g.set_option(name, on)
            assert g.get_option("shadow_split") == 0, name
            g.set_option(name, off)
            assert g.get_option("shadow_split") == CHOSEN_K, name
        g.trace_stats_enable(True)
        assert g.get_option("shadow_split") == 0
        g.trace_stats_enable(False)
        assert g.get_option("shadow_split") == CHOSEN_K
        g.set_params(p_area)
        assert g.get_option("shadow_split") == 0
        driver.benchmark_iteration(g, NPIX)
        g.set_option("shadow_split", 0)
        assert g.get_option("shadow_split") == 0
        g.set_params(p_env)
        assert g.get_option("shadow_split") == 0
        g.set_option("shadow_split", 3)
        assert g.get_option("shadow_split") == 3
        g.set_params(p_area)
        assert g.get_option("shadow_split") == 3
        g.set_option("shadow_split", -1)
        assert g.get_option("shadow_split") == 0
        g.set_params(p_env)
        assert g.get_option("shadow_split") == CHOSEN_K
    finally:
        g.close()
