"""The restatement of tests/mesh_light_step_cases.py checked on the CPU before the GPU tests lean on it: the scene holds
what the cases need, the classifier decides every named edge case and all but 3 % of each group, the seeds give the draws they were chosen
for, and the closed form of the lamp over the floor agrees with quadrature and has converged over the sub-pixel grid."""
import numpy as np
import pytest
import bsdf_cases as bc
import mesh_light_cases as MC
import mesh_light_reference as MR
import mesh_light_step_cases as SC

F = np.float32


@pytest.fixture(scope="module")
def S():
    return SC.step_scene()


@pytest.fixture(scope="module")
def implicit(S):
    c = SC.ImplicitCases(S)
    return c, {mode: SC.implicit_verdict(S, c, S.table, mode) for mode in SC.MODES}


@pytest.fixture(scope="module")
def sampled(S):
    c = SC.SampledCases(S, S.table)
    g = SC.SampledGeometry(S, c, S.table)
    return c, g, {mode: SC.sampled_verdict(S, c, S.table, g, mode) for mode in SC.MODES[:2]}


def test_scene_holds_what_the_cases_need(S):
    tris, cdf, pick, total = S.table
    assert 300 <= S.d0.tris.size <= 600
    assert tris.size > MC.SCAN_BLOCK + 3 and np.array_equal(tris, S.lamps)
    k = {name: [int(np.searchsorted(tris, t)) for t in S.names[name]] for name in ("tiny", "dominant", "last")}
    assert pick[k["tiny"][0]] == 0 and k["dominant"][0] == k["tiny"][0] + 1, "a pick that rounds to 0 next to the dominant light"
    assert pick[k["dominant"]].sum() > 0.5
    assert k["last"][0] == tris.size - 1 and cdf[-1] == 1.0 and pick[-1] == 0, "the last light is not pickable: the clamp is not the last index"
    assert S.gains not in tris and (S.ke[S.gains] > 0).any() and not (MR.ke_of(S.d0)[S.gains] > 0).any()
    types = set(int(S.type[S.mat[S.names[f"receiver{j}"][0]]]) for j in range(6))
    assert types == set(bc.TYPES)
    # the veil is past 0.995 |L| from every receiver point below it, and before the lamp
    y_lamp, y_veil = S.P[S.names["veiled"][0], 0, 1], S.P[S.names["veil"][0], 0, 1]
    assert 0.995 < y_veil / y_lamp < 1.0 and 0.995 < (y_veil - 1e-3) / (y_lamp - 1e-3)


def test_implicit_cases_are_decided(S, implicit):
    c, verdicts = implicit
    assert 1000 <= c.n <= 3000
    for mode, v in verdicts.items():
        share = SC.undecided_share(v, c.group)
        print(f"implicit, mode {mode}: undecided {share}; contributing {int(v.nom['contrib'].sum())}, MIS-weighted {int(v.nom['mis'].sum())} of {c.n}")
        assert all(s <= SC.UNDECIDED_CAP for s in share.values()), share
        assert v.decided[c.named].all(), f"named cases undecided: {np.unique(c.label[c.named & ~v.decided]).tolist()}"
    v = verdicts[(1, 1)]
    w = v.nom["w"]
    # the cases reach what they were built for
    for label in ("light 0", "light 255", "light 256", "dominant"):
        m = np.char.startswith(c.label, label) & v.nom["mis"]
        assert m.any() and (w[m] < 1.0).any(), label
    for label in ("pick = 0", "last light", "gains emission"):
        m = np.char.startswith(c.label, label)
        assert v.nom["contrib"][m].all() and (w[m] == 1.0).all(), f"{label}: seen with weight 1"
    for label in ("back of a lamp", "plate before a lamp", "no light"):
        assert not v.nom["contrib"][np.char.startswith(c.label, label)].any(), label
    m = np.char.startswith(c.label, "lamp before a lamp")
    assert np.isin(c.hit[m], S.names["front"]).all()
    hidden = c.group == "hidden"
    assert (c.hit[hidden] != c.target[hidden]).mean() > 0.4, "the hidden lamps are mostly hidden"
    assert ((c.cos <= 1e-3) & v.decided & v.nom["mis"]).sum() >= 4, "grazing incidence reaches the MIS weight"
    assert (w[v.nom["mis"] & v.decided] < 0.5).sum() > 50 and (w[v.nom["mis"] & v.decided] > 0.5).sum() > 50
    assert c.quad_wins.sum() >= 10 and c.quad_clear.mean() > 0.97
    # implicit only: nothing is weighted; NEE only: nothing beyond the first vertex is counted
    assert not verdicts[(0, 1)].nom["mis"].any()
    assert not verdicts[(1, 0)].nom["contrib"][c.len_before > 0].any() and verdicts[(1, 0)].nom["contrib"][c.len_before == 0].any()


def test_sampled_cases_are_decided(S, sampled):
    c, g, verdicts = sampled
    tris, cdf, pick, _ = S.table
    assert 1000 <= c.n <= 3000
    for mode, v in verdicts.items():
        share = SC.undecided_share(v, c.group)
        print(f"sampled, mode {mode}: undecided {share}; lit {int(v.nom['lit'].sum())} of {c.n}")
        assert all(s <= SC.UNDECIDED_CAP for s in share.values()), share
        assert v.decided[c.named].all(), f"named cases undecided: {np.unique(c.label[c.named & ~v.decided]).tolist()}"
    v = verdicts[(1, 1)]
    # the seeds give the draws they were chosen for
    for label, r0 in c.edge_r0.items():
        assert (g.r0[c.label == label].astype(F) == r0).all(), label
    last_pickable = np.nonzero(pick > 0)[0][-1]
    assert (g.k[c.label == "r0 = 1"] == last_pickable).all() and c.edge_r0["r0 = 1"] == 1.0 and c.edge_r0["r0 = 1 - ulp"] == SC.BELOW1 and (g.k[c.label == "r0 = 0"] == 0).all()
    for k in (0, MC.SCAN_BLOCK - 1, MC.SCAN_BLOCK):
        at, below = c.edge_r0[f"r0 = cdf[{k}]"], c.edge_r0[f"r0 = cdf[{k}] - ulp"]             # the two draws nearest to cdf[k] that a seed can give
        assert below < cdf[k] <= at and float(at) - float(below) <= max(2.0 ** -32, float(np.spacing(cdf[k]))), k
        assert (g.k[c.label == f"r0 = cdf[{k}]"] > k).all() and (g.k[c.label == f"r0 = cdf[{k}] - ulp"] == k).all()
    kt = c.k_of["tiny"][0]
    assert (g.k[c.label == "r0 = cdf[pick = 0]"] == kt + 1).all() and (g.k[c.label == "r0 = cdf[pick = 0] - ulp"] == kt - 1).all()
    assert (pick[g.k] > 0).all() or c.singular.any()
    for name, r in (("r1", g.r1), ("r2", g.r2)):
        assert (r[c.label == f"{name} = 0"] == 0).all() and (r[c.label == f"{name} = below 1"].astype(F) == SC.BELOW1).all()
    assert (g.k > MC.SCAN_BLOCK).sum() > 100 and (g.k < MC.SCAN_BLOCK).sum() > 100, "picks on both sides of the seam"
    # the arrangements do what they were built for
    arr = c.group == "arrangements"
    assert not v.nom["lit"][arr & (c.label == "back")].any() and (v.nom["cosLight"][arr & (c.label == "back")] == 0).all()
    assert g.occluded[arr & (c.label == "behind")].mean() > 0.3, "the front lamp hides part of the one behind"
    half = arr & (c.label == "half")
    assert 0.2 < g.occluded[half].mean() < 0.8
    veiled = arr & (c.label == "veiled")
    assert v.nom["lit"][veiled].all() and v.decided[veiled].all(), "a plate past 0.995 |L| does not occlude, nor does the lamp"
    hz = c.group == "horizon"
    assert (v.nom["lit"] & ~v.nom["above"] & v.decided)[hz].sum() >= 20, "lit lights below the receiver's horizon"
    assert (v.nom["lit"] & v.decided)[c.group == "back face"].sum() >= 20
    assert (v.nom["lit"] & (v.nom["weight"] < 0.9) & v.decided).sum() > 100, "the MIS weight matters"
    assert v.silent[c.singular].all() and not v.nom["lit"][c.singular].any()
    for t in SC.NONSINGULAR:
        assert (v.nom["lit"] & v.decided & (S.type[c.mat] == t)).sum() >= 40, f"BSDF type {t}"


def test_draws_shift_with_the_lights_before(S, sampled):
    """with the environment map and the quad on, the mesh draws are numbers 4 to 6 of the stream"""
    c, g, _ = sampled
    g3 = SC.SampledGeometry(S, c, S.table, first=3)
    s = c.seed.copy()
    for _ in range(3):
        _, s = bc.rand01(s)
    r, _ = bc.rand01(s)
    assert np.array_equal(g3.r0, r) and not np.array_equal(g3.r0, g.r0)
    assert np.array_equal(SC.advance(c.seed, 3).astype(np.uint64), s)


def test_cases_stay_decided_behind_other_lights_and_without_a_prior(S, sampled):
    """the three-lights test holds dEi to float64 on its own (prior Ei 0, so the tolerance scales with dEi) from draws 4 to 6"""
    import copy
    c, _, _ = sampled
    c0 = copy.copy(c)
    c0.Ei = np.zeros_like(c.Ei)
    g3 = SC.SampledGeometry(S, c, S.table, first=3)
    for mode in SC.MODES[:2]:
        v = SC.sampled_verdict(S, c0, S.table, g3, mode)
        share = SC.undecided_share(v, c.group)
        print(f"sampled after three draws, no prior, mode {mode}: undecided {share}")
        assert all(s <= SC.UNDECIDED_CAP for s in share.values()), share
        assert (v.decided & ~v.silent).sum() > 500


def test_polygon_irradiance_against_quadrature():
    rng = np.random.RandomState(2)
    x = np.stack([rng.uniform(-1.0, 1.0, 100), np.zeros(100), rng.uniform(-1.0, 1.0, 100)], 1)
    n = np.array([0.0, 1.0, 0.0])
    a, b = SC.polygon_irradiance(x, n, SC.LF_LAMP), SC.quadrature_irradiance(x, n, SC.LF_LAMP)
    err = np.abs(a - b) / b
    print(f"edge sum against quadrature at 100 floor points: largest relative difference {err.max():.2e}; E from {a.min():.3f} to {a.max():.3f}")
    assert err.max() <= 1e-6
    # a lamp filling the upper half space gives pi
    big = np.array([[-1e7, 1.0, -1e7], [0.0, 1.0, 2e7], [1e7, 1.0, -1e7]])
    assert abs(SC.polygon_irradiance(np.zeros((1, 3)), n, big)[0] - np.pi) < 1e-5


def test_sub_pixel_grid_has_converged():
    """s = 4 against s = 8: no tile mean moves by more than 1e-5 of itself; the GPU test asserts that this is below a tenth of every tile's
    standard error"""
    d = SC.lamp_floor_scene()
    p = SC.lamp_floor_params(d, (1, 1))
    t4, t8 = SC.tile_means(SC.lamp_floor_truth(p, 4)), SC.tile_means(SC.lamp_floor_truth(p, 8))
    rel = np.abs(t4 - t8) / t8
    print(f"sub-pixel grid 4 against 8: largest relative move of a tile mean {rel.max():.2e}; tile means {t8.min():.4f} .. {t8.max():.4f}")
    assert rel.max() <= SC.LF_SUBPIXEL_REL
