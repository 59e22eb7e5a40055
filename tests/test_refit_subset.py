"""BVH::refitSubset (host.refit_bvh_subset) on the CPU: the restatement the device's subset refit (tests/test_gpu_refit_subset.py) is compared with.

Trees are built on positions P; the standard subset S (tests/refit_subset_cases.py) is moved by an eighth of the extent.  Asserted against a plain
numpy restatement: the node array bit for bit, every node without a listed triangle below it on its upload bytes, clean clipped leaves still
strictly inside their triangles' full bounds (the property the subset refit exists for), equality with host.refit_bvh where nothing is clipped,
the algebra (all indices = full refit; two disjoint halves = one call; a repeated call changes nothing), no robust hit of the float64 witness
outside a leaf box of its triangle, and the refusals."""
import numpy as np
import pytest
import traversal_cases as tc
import refit_cases as rc
import refit_subset_cases as sc
from fluctus_amd import host


@pytest.mark.parametrize("name,builder", sc.CASES)
def test_subset_refit_equals_the_restatement_and_keeps_clean_nodes(name, builder):
    d = sc.built(name, builder)
    idx, P2 = sc.S(name)
    r = sc.subset_refitted(d, idx, P2)
    want, dirty = sc.refit_subset(sc.moved_scene(d, P2), idx)
    assert r.nodes.tobytes() == want.tobytes()
    assert r.nodes[~dirty].tobytes() == d.nodes[~dirty].tobytes(), "a node without a listed triangle below it changed"
    for f in ("nPrims", "iStartOrRight", "parent"):
        assert np.array_equal(r.nodes[f], d.nodes[f]), f
    assert dirty[0] and 0 < dirty.sum() < dirty.size
    mn, mx = rc.node_box(r.nodes, 0)
    assert np.isclose(r.world_radius, 0.5 * np.linalg.norm(mx.astype(np.float64) - mn), rtol=1e-6)
    assert host.wide_tree_check(r)["nested"]
    leaves = d.nodes["nPrims"] > 0
    print(f"{name}/{builder}: {int((dirty & leaves).sum())} dirty leaves, {int(dirty.sum())} of {dirty.size} nodes rewritten; surface-area sum "
          f"{sc.surface_area_sum(d.nodes):.1f} uploaded, {sc.surface_area_sum(r.nodes):.1f} subset, "
          f"{sc.surface_area_sum(rc.refitted(d, P2).nodes):.1f} full refit")


def test_clean_clipped_leaves_stay_clipped():
    name = "spatial_splits-o0"
    d = sc.built(name, "sbvh")
    assert d.bvh_metrics["spatial_splits"] > 0
    idx, P2 = sc.S(name)
    r = sc.subset_refitted(d, idx, P2)
    dirty = sc.dirty_sets(d, idx)
    before, after = set(sc.clipped_leaves(d)), set(sc.clipped_leaves(r))
    clean_clipped = {i for i in before if not dirty[i]}
    assert clean_clipped, "no clean leaf is clipped: the case does not reach the property"
    assert clean_clipped <= after, "a clean clipped leaf was unclipped"
    assert not any(dirty[i] for i in after), "a dirty leaf is not the union of its triangles' full bounds"
    full = rc.refitted(d, P2)
    assert not sc.clipped_leaves(full)
    assert sc.surface_area_sum(r.nodes) < sc.surface_area_sum(full.nodes)
    print(f"{len(before)} clipped leaves uploaded, {len(clean_clipped)} clean ones kept, {int((dirty & (d.nodes['nPrims'] > 0)).sum())} dirty leaves")


@pytest.mark.parametrize("name,builder", sc.UNCLIPPED)
def test_unclipped_scenes_equal_the_full_refit(name, builder):
    d = sc.built(name, builder)
    assert not sc.clipped_leaves(d)
    idx, P2 = sc.S(name)
    assert sc.subset_refitted(d, idx, P2).nodes.tobytes() == rc.refitted(d, P2).nodes.tobytes()


@pytest.mark.parametrize("name,builder", sc.CASES)
def test_subset_algebra(name, builder):
    d = sc.built(name, builder)
    idx, P2 = sc.S(name)
    once = sc.subset_refitted(d, idx, P2)
    # every index listed: the full refit
    every = np.arange(d.tris.size, dtype=np.uint32)
    assert sc.subset_refitted(d, every, P2).nodes.tobytes() == rc.refitted(d, P2).nodes.tobytes()
    # two calls on disjoint halves: one call
    a, b = idx[::2], idx[1::2]
    half = sc.subset_refitted(d, a, sc.translated(rc.SCENES[name], a, sc.standard_shift(rc.SCENES[name])))
    both = host.refit_bvh_subset(rc.moved(half, P2), b)
    assert both.nodes.tobytes() == once.nodes.tobytes()
    assert both.world_radius == once.world_radius
    # a second identical call changes nothing
    again = host.refit_bvh_subset(rc.moved(once, P2), idx)
    assert again.nodes.tobytes() == once.nodes.tobytes()
    # nothing listed: nothing changes
    assert host.refit_bvh_subset(rc.moved(d, P2), np.zeros(0, np.uint32)).nodes.tobytes() == d.nodes.tobytes()


@pytest.mark.parametrize("name,builder", sc.CASES)
def test_witness_finds_no_hit_outside_its_leaf_boxes(name, builder):
    d = sc.built(name, builder)
    idx, P2 = sc.S(name)
    r = sc.subset_refitted(d, idx, P2)
    rays = tc.all_rays(tc.tri_points(r), tc.Leaves(r))
    orig, dirs, tmax = (np.concatenate([x[k] for x in rays.values()]) for k in range(3))
    v = tc.BruteForce(tc.tri_points(r), orig, dirs, tmax).verdict(r)
    assert not v["uncovered"], f"robust hits outside every leaf box of their triangle: {v['uncovered'][:3]}"
    assert v["ext_decided"].sum() > 0


def test_subset_refit_single_leaf_scene():
    P, d = rc.two_triangle_scene()
    idx = np.array([1], np.uint32)
    P2 = sc.translated(P, idx, (512.0, 0.0, 0.0))
    r = sc.subset_refitted(d, idx, P2)
    assert r.nodes.tobytes() == rc.refitted(d, P2).nodes.tobytes()


def test_refusals_leave_the_nodes_untouched():
    name = "flat_walls-o0"
    d = rc.built(rc.SCENES[name], "sah")
    idx, P2 = sc.S(name)

    def refused(m, i, msg):
        keep = m.nodes.tobytes()
        with pytest.raises(RuntimeError, match=msg):
            host.refit_bvh_subset(m, np.asarray(i, np.uint32))
        assert m.nodes.tobytes() == keep, f"'{msg}': the node array changed"

    refused(rc.moved(d, P2), [0, 8, d.tris.size], "triangle index out of range")
    refused(rc.moved(d, P2), [8, 0], "not strictly ascending")
    refused(rc.moved(d, P2), [0, 8, 8], "not strictly ascending")
    m = rc.moved(d, P2)
    leaf = int(np.nonzero(m.nodes["nPrims"] > 0)[0][-1])
    m.nodes["iStartOrRight"][leaf] = m.indices.size                      # a leaf run past the index list
    refused(m, idx, "leaf range outside the index list")
    m = rc.moved(d, P2)
    inner = int(np.nonzero(m.nodes["nPrims"] == 0)[0][-1])
    m.nodes["iStartOrRight"][inner] = inner                              # a right child that is not behind its parent
    refused(m, idx, "child index out of range")
    refused(rc.moved(d, P2[:-3]), idx[idx < d.tris.size - 3], "triangle index out of range")     # a triangle array shorter than the tree's
