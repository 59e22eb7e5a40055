"""BVH::refit (host.refit_bvh) and the refit's quantiser on the CPU: the restatement the device refit (tests/test_gpu_refit.py) is compared with.

Trees are built on positions P and refitted to P' (tests/refit_cases.py: identity, smooth, scramble).  Asserted: topology, parents, leaf ranges
and the index list untouched; every leaf box the union of its triangles' fp32 bounds and every inner box the union of its two children, bit for
bit; the 4-wide tree built over the result passes host.wide_tree_check; refit is idempotent and has no history (P -> P' -> P equals P -> P).
The fp64 quantiser the kernels run (csrc/flx_refit.h, compiled for the host) must contain every child box in exact rational arithmetic and never
pick a larger scale than build_wide's long-double quantiser."""
import numpy as np
import pytest
import refit_cases as rc
from fluctus_amd import host


@pytest.mark.parametrize("kind", rc.DEFORMS)
@pytest.mark.parametrize("builder", rc.BUILDERS)
@pytest.mark.parametrize("name", rc.CASES)
def test_refit_boxes_are_unions_and_topology_is_untouched(name, builder, kind):
    P = rc.SCENES[name]
    d = rc.built(P, builder)
    r = rc.refitted(d, rc.deform(P, kind))
    for f in ("nPrims", "iStartOrRight", "parent"):
        assert np.array_equal(r.nodes[f], d.nodes[f]), f
    assert r.indices is d.indices or np.array_equal(r.indices, d.indices)
    rc.check_refit_boxes(r)
    info = host.wide_tree_check(r)
    assert info["nested"]
    mn, mx = rc.node_box(r.nodes, 0)
    assert np.isclose(r.world_radius, 0.5 * np.linalg.norm(mx.astype(np.float64) - mn), rtol=1e-6)     # as the builder derives it: half the root box's diagonal
    nodes, leaves = host.wide_tables_check(r)
    assert nodes == info["wide_nodes"] and leaves == info["leaves"]


@pytest.mark.parametrize("builder", rc.BUILDERS)
def test_refit_is_idempotent_and_has_no_history(builder):
    P = rc.SCENES["spatial_splits-o0"]
    d = rc.built(P, builder)
    P2 = rc.deform(P, "smooth")
    once = rc.refitted(d, P2)
    twice = host.refit_bvh(rc.moved(once, P2))
    assert once.nodes.tobytes() == twice.nodes.tobytes()
    back = host.refit_bvh(rc.moved(once, P))
    assert back.nodes.tobytes() == rc.refitted(d, P).nodes.tobytes()
    assert back.world_radius == rc.refitted(d, P).world_radius


def test_refit_unclips_spatially_split_leaves():
    """identity on an SBVH with spatial splits: every box contains the builder's, and some leaf grows (the clipped ones)"""
    P = rc.SCENES["spatial_splits-o0"]
    d = rc.built(P, "sbvh")
    assert d.bvh_metrics["spatial_splits"] > 0
    r = rc.refitted(d, P)
    grew = 0
    for k in "xyz":
        assert (r.nodes["bmin"][k] <= d.nodes["bmin"][k]).all() and (r.nodes["bmax"][k] >= d.nodes["bmax"][k]).all()
        grew += int(((r.nodes["bmin"][k] < d.nodes["bmin"][k]) | (r.nodes["bmax"][k] > d.nodes["bmax"][k])).sum())
    assert grew > 0


def test_refit_single_leaf_scene():
    P, d = rc.two_triangle_scene()
    r = rc.refitted(d, P + 3.0)
    rc.check_refit_boxes(r)
    assert host.wide_tables_check(r) == (1, 1)


def test_refit_refuses_a_triangle_array_of_another_length():
    P = rc.SCENES["flat_walls-o0"]
    d = rc.built(P, "sah")
    m = rc.moved(d, P[:-3])
    with pytest.raises(RuntimeError, match="triangle index out of range"):
        host.refit_bvh(m)


def _child_box_sets():
    """(ns, 3) child boxes: random ones over 40 binades, exact powers of two and their neighbours (where the first guess of the exponent of the
    two arithmetics differs), zero extents, tiny boxes far from the origin, the +-2^62 bound"""
    rng = np.random.RandomState(17)
    out = []
    for _ in range(400):
        ns = rng.randint(2, 5)
        c = rng.normal(size=3) * 10.0 ** rng.uniform(-6, 6)
        e = 10.0 ** rng.uniform(-8, 4, size=(ns, 3))
        lo = c + rng.normal(size=(ns, 3)) * e
        out.append((lo, lo + np.abs(rng.normal(size=(ns, 3))) * e * rng.choice([0.0, 1.0], (ns, 3), p=[0.15, 0.85])))
    for k in (-100, -20, 0, 7, 30, 61):
        w = 255.0 * 2.0 ** k
        for d in (0.0, 1.0, -1.0):                      # extent exactly 255 * 2^k, and one ulp either side
            hi = np.float32(w)
            hi = np.nextafter(hi, np.float32(np.inf)) if d > 0 else np.nextafter(hi, np.float32(0)) if d < 0 else hi
            lo = np.zeros((2, 3)); up = np.full((2, 3), float(hi)); up[1] *= 0.5
            out.append((lo, up))
    out.append((np.array([[-2.0 ** -100] * 3, [2.0 ** 60] * 3]), np.array([[2.0 ** -101] * 3, [2.0 ** 60] * 3])))      # c - lo needs > 64 bits
    out.append((np.array([[-2.0 ** 62] * 3, [1.0] * 3]), np.array([[0.0] * 3, [2.0 ** 62] * 3])))
    out.append((np.array([[1e5] * 3, [1e5 + 0.0078125] * 3]), np.array([[1e5] * 3, [1e5 + 0.015625] * 3])))
    out.append((np.zeros((3, 3)), np.zeros((3, 3))))
    return [(np.float32(a), np.float32(b)) for a, b in out]


def test_device_quantiser_contains_the_boxes_exactly_and_is_no_looser_than_the_host():
    differ = 0
    for cmin, cmax in _child_box_sets():
        ns = cmin.shape[0]
        o, s, qlo, qhi = host.wide_quantise(cmin, cmax, device_arithmetic=True)
        ho, hs, hqlo, hqhi = host.wide_quantise(cmin, cmax)
        assert np.array_equal(rc.bits(o), rc.bits(rc.fold_min(cmin)))
        assert rc.planes_contain(o, s, qlo, qhi, cmin, cmax), (cmin, cmax, s, qlo, qhi)
        e = np.log2(s.astype(np.float64))
        assert (e == np.round(e)).all() and (e >= -108).all()
        assert (s <= hs).all(), f"fp64 scale {s} above the long-double one {hs}"
        for a in range(3):                               # unused slots inverted
            for k in range(ns, 4):
                assert (int(qlo[a]) >> (8 * k)) & 255 == 255 and (int(qhi[a]) >> (8 * k)) & 255 == 0
            # the smallest scale that fits: at half of it (above the floor) some plane needs more than 8 bits
            if e[a] > -108:
                need = max(float(cmax[k, a]) - float(o[a]) for k in range(ns)) / (float(s[a]) / 2.0)
                assert need > 255.0, (cmin, cmax, s)
        differ += int(not (np.array_equal(s, hs) and np.array_equal(qlo, hqlo) and np.array_equal(qhi, hqhi)))
    print(f"grids that differ between the fp64 and the long-double quantiser: {differ}")
