"""The witness that the traversal stacks' spill paths run (tests/stack_cases.py), without a GPU.

The kernels cannot report how deep their stacks went, so the claim "these rays spill" is made on the host, from the same nodes and rays the
device tests (tests/test_gpu_stack_spill.py) trace: traverse<>'s push / pop rule restated in numpy, the 4-wide traversal emulated by
tests/wide_analysis.cpp with WStack's ring rule replayed on each ray's own push / pop sequence.  Asserted here, as conditions:
  * every deep family peaks above LDS_LEVELS / pages out at least once under every traversal it is deep for, hole rays page back in, the
    decks-of-decks hole rays go through at least 3 page-out / page-in cycles, every shallow family stays at or below the thresholds;
  * every crafted ray is DECIDED by the float64 brute force (traversal_cases.BruteForce; cap on undecided rays: 0) and the oracle's closest
    hit and any hit equal the brute force's on all of them, as do the two emulations';
  * the same after a full and a subset refit, on the refitted nodes;
  * and the honest figures of the two older "deep chain" tests, which bound the tree and never reach the spill paths: binary peak 1, 4-wide 3.
LDS_LEVELS and WIDE_LDS_LEVELS come out of the two headers, so a change of either fails here instead of quietly ending the coverage."""
import numpy as np
import pytest
import common
import stack_cases as sc
import traversal_cases as tc
from common import COL, Q
from fluctus_amd import host, wire, driver
from oracle.binding import OracleContext

N_MIXED = 64 * 20 + 37


def _oracle(d, orig, dirs, tmax):
    n = orig.shape[0]
    o = OracleContext(n, threads=8)
    o.upload_scene(d); o.set_params(tc.params(d, 0)); driver.reset_renderer(o)
    tc.load_rays(o, orig, dirs, tmax)
    o.wf_extend(); o.wf_shadow()
    r = tc.hits(o, n)
    o.close()
    return r


def _check_scene(d, what, n=N_MIXED, min_cycles=1):
    P = tc.tri_points(d)
    orig, dirs, tmax, fam = sc.mixed_queue(P, n)
    assert all((fam == f).sum() >= 8 for f in range(len(sc.FAMILIES)))
    w = sc.witness(d, orig, dirs, tmax)
    rows = sc.check_thresholds(w, fam, what, min_cycles)
    print(sc.format_rows(what, rows))
    # the geometry's answer, the brute force's, the oracle's and the two emulations': one and the same on every ray
    closest, blocked = sc.expected_hits(P, fam)
    v = tc.BruteForce(P, orig, dirs, tmax).verdict(d)
    assert not v["uncovered"]
    assert v["ext_decided"].all() and v["sh_decided"].all(), f"{what}: {int((~v['ext_decided']).sum())} / {int((~v['sh_decided']).sum())} rays undecided (cap 0)"
    assert np.array_equal(v["closest"], closest) and np.array_equal(v["blocked"], blocked), f"{what}: the brute force disagrees with the construction"
    hi, bl = _oracle(d, orig, dirs, tmax)
    assert np.array_equal(hi, v["closest"]), f"{what}: the oracle's closest hit differs from the brute force's on {int((hi != v['closest']).sum())} rays"
    assert np.array_equal(bl, v["blocked"]), f"{what}: the oracle's any hit differs from the brute force's on {int((bl != v['blocked']).sum())} rays"
    for k in ("binary_closest", "closest"):
        assert np.array_equal(w[k]["tri"], closest), f"{what}: {k} emulation"
    for k in ("binary_any", "any_last_slot", "any_far_near"):
        assert np.array_equal(w[k]["tri"] >= 0, blocked), f"{what}: {k} emulation"
    return w, fam


def test_constants_come_from_the_headers():
    """the thresholds follow the headers, and the scenes out-climb the levels as they stand with at least one more page of 8 to spare"""
    assert sc.LDS_LEVELS >= 1 and sc.WIDE_LDS_LEVELS >= 8 and sc.WIDE_LDS_LEVELS & (sc.WIDE_LDS_LEVELS - 1) == 0
    assert sc.WIDE_NO_PAGE == sc.WIDE_LDS_LEVELS - 4
    for sizes in ([41], [100], sc.DECKS):
        assert min(sizes) - 1 > max(sc.LDS_LEVELS, sc.WIDE_NO_PAGE), sizes
    assert 41 - 1 >= max(sc.LDS_LEVELS, sc.WIDE_NO_PAGE) + 8


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_crafted_rays_reach_the_spill_paths(name):
    d = sc.SCENES[name]()
    info = host.wide_tree_check(d)
    assert info["nested"]
    nt = d.tris.size
    w, fam = _check_scene(d, name, min_cycles=3 if name == "decks" else 1)
    hole, solid = fam == sc.FAMILIES.index("deep_hole"), fam == sc.FAMILIES.index("deep_solid")
    if name != "decks":
        # one chain: a ray from above pushes at every level, in both trees
        for k in ("binary_closest", "binary_any", "closest", "any_last_slot"):
            assert (w[k]["peak"][hole | solid] == nt - 1).all(), k
        assert info["max_stack"] == nt
    else:
        assert d.nodes.size == 219 and info["max_stack"] == 34
        assert (w["closest"]["peak"][hole] == 32).all() and (w["closest"]["peak"][solid] == 22).all()
        assert (w["binary_closest"]["climbs"][hole] == len(sc.DECKS)).all()          # once per deck


def test_small_queue_and_budgets_of_the_split_kernel():
    """A queue below 256 rays still holds every family, and where k_shadow4s's node-visit budgets run out the deep rays stand as the GPU test
    needs them: budget 1 and 3 in front of an inner node with a short unpaged stack (they suspend, and page after they resume, in another
    lane), budget 8 with part of the stack already paged out (no record can hold them: they keep going)."""
    d = sc.SCENES["deck41"]()
    P = tc.tri_points(d)
    orig, dirs, tmax, fam = sc.mixed_queue(P, 64 * 3 + 37)
    rows = sc.check_thresholds(sc.witness(d, orig, dirs, tmax), fam, "deck41/229")
    print(sc.format_rows("deck41, 229 rays", rows))
    keep = 14                                                              # FLX_SPLIT_KEEP (csrc/flx_trace4.h)
    for mode, deep in (("any_last_slot", sc.DEEP_IN["any_last_slot"]), ("any_far_near", sc.DEEP_IN["any_far_near"])):
        m = np.isin(fam, [sc.FAMILIES.index(f) for f in deep])
        for budget, suspends in ((1, True), (3, True), (8, False)):
            w = sc.wide_witness(d, orig, dirs, tmax, mode, budget)
            assert (w["susp_sp"][m] >= 0).all(), f"{mode} budget {budget}: a deep ray finished inside its budget"
            can = (w["susp_base"][m] == 0) & (w["susp_sp"][m] < keep)
            assert (can == suspends).all(), f"{mode} budget {budget}: sp {w['susp_sp'][m][:4]} base {w['susp_base'][m][:4]}"
            assert (w["page_outs"][m] >= 1).all()
            print(f"deck41 {mode} budget {budget}: deep rays stand at sp {int(w['susp_sp'][m].min())}..{int(w['susp_sp'][m].max())}, "
                  f"base {int(w['susp_base'][m].min())}..{int(w['susp_base'][m].max())} -> {'suspend' if suspends else 'too deep for a record'}")


def refit_steps(name="deck41"):
    """The refit case, shared with the GPU test: [(label, SceneData with refitted nodes, subset indices or None)] -- the deck moved with its z
    spacing doubled (host.refit_bvh), then every third card shifted by 0.25 in x (host.refit_bvh_subset)."""
    d0 = sc.SCENES[name]()
    steps = []
    P1 = sc.deck_points(d0.sizes, dz=0.25, gap=2.0, offset=(0.75, -0.5, 1.25))
    d1 = tc.make_scene(P1); d1.nodes, d1.indices = d0.nodes.copy(), d0.indices.copy()
    host.refit_bvh(d1)
    steps.append(("moved, dz doubled", d1, None))
    P2 = sc.deck_points(d0.sizes, dz=0.25, gap=2.0, offset=(0.75, -0.5, 1.25), shift_every=3, shift_x=0.25)
    d2 = tc.make_scene(P2); d2.nodes, d2.indices = d1.nodes.copy(), d1.indices.copy()
    idx = np.arange(0, P2.shape[0], 3, dtype=np.uint32)
    host.refit_bvh_subset(d2, idx)
    steps.append(("every third card shifted", d2, idx))
    return d0, steps


@pytest.mark.parametrize("name", ["deck41", "decks"])
def test_refitted_decks_still_spill(name):
    d0, steps = refit_steps(name)
    for label, d, idx in steps:
        assert not np.array_equal(d.nodes["bmin"], d0.nodes["bmin"])
        _check_scene(d, f"{name} {label}", min_cycles=3 if name == "decks" else 1)


def legacy_chain_scene(nt):
    """The scene of the two older chain tests (tests/test_gpu_parity.py::test_single_leaf_scene_and_deep_stack_spill, 41 triangles, and
    tests/test_gpu_wide.py::test_wide_tree_edge_cases_single_leaf_and_deep_chain, 61): a right-leaning chain over the first triangles of
    common.small_mesh_scene -- a flat ground grid."""
    d = common.small_mesh_scene(n=6)
    d.tris = d.tris[:nt].copy()
    d.materials = np.array([common.default_material()], wire.MATERIAL)
    d.texdesc = np.zeros(0, wire.TEXDESC); d.texdata = np.zeros(0, np.uint8)
    d.nodes = sc.chain_nodes(tc.tri_points(d), sc.chain_tree([nt]))
    d.indices = np.arange(nt, dtype=np.uint32)
    sc.set_radius(d)
    return d


@pytest.mark.parametrize("nt", [41, 61])
def test_the_older_chain_tests_never_leave_the_lds_levels(nt):
    """The honest figures of the two tests that used to claim the spill paths: their trees are 40 and 60 levels deep (wide stack bound > 16,
    which is all they assert about depth), and over the six iterations they run no ray's binary stack holds more than 1 entry, no 4-wide
    closest-hit stack more than 3, no any-hit stack any: a camera ray over a flat grid pierces a handful of leaf boxes."""
    d = legacy_chain_scene(nt)
    assert host.wide_tree_check(d)["max_stack"] > 16
    p = common.scene_params(d, 32, 32, maxBounces=3)
    o = OracleContext(1024, threads=8)
    o.upload_scene(d); o.set_params(p); driver.reset_renderer(o)
    ext, sh = [], []
    for it in range(6):
        o.wf_logic(False); o.wf_raygen(); o.wf_materials()
        cnt = np.array(o.get_counters(), copy=True)
        st = o.state_export()
        qe, qs = o.queue_read(Q.EXTENSION)[:int(cnt[Q.EXTENSION])], o.queue_read(Q.SHADOW)[:int(cnt[Q.SHADOW])]
        ext.append((st[COL.ORIG:COL.ORIG + 3, qe].T, st[COL.DIR:COL.DIR + 3, qe].T, np.full(qe.size, tc.FLT_MAX, np.float32)))
        sh.append((st[COL.SHADOW_ORIG:COL.SHADOW_ORIG + 3, qs].T, st[COL.SHADOW_DIR:COL.SHADOW_DIR + 3, qs].T, st[COL.SHADOW_LEN, qs]))
        o.wf_extend(); o.wf_shadow()
        o.clear_queues(); o.pixel_index_update(32 * 32, int(cnt[Q.RAYGEN]))
    o.close()
    eo, ed, et = (np.ascontiguousarray(np.concatenate(a), np.float32) for a in zip(*ext))
    so, sd, st_ = (np.ascontiguousarray(np.concatenate(a), np.float32) for a in zip(*sh))
    assert eo.shape[0] > 4096 and so.shape[0] > 0
    peaks = {"binary_closest": int(sc.binary_witness(d, eo, ed, et, False)["peak"].max()),
             "binary_any": int(sc.binary_witness(d, so, sd, st_, True)["peak"].max()),
             "closest": int(sc.wide_witness(d, eo, ed, et, "closest")["peak"].max()),
             "any_last_slot": int(sc.wide_witness(d, so, sd, st_, "any_last_slot")["peak"].max()),
             "any_far_near": int(sc.wide_witness(d, so, sd, st_, "any_far_near")["peak"].max())}
    print(f"{nt}-triangle chain: {eo.shape[0]} extension rays, {so.shape[0]} shadow rays, deepest stacks {peaks}")
    assert peaks["binary_closest"] == 1 and peaks["binary_any"] <= 1
    assert peaks["closest"] == 3 and peaks["any_last_slot"] == 0 and peaks["any_far_near"] == 0
