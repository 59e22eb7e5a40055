"""Scenes and rays that PROVABLY drive the traversal stacks past their LDS levels, and the host-side witness that says so.

Every traversal kernel keeps LDS_LEVELS (csrc/flx_trace.h) / WIDE_LDS_LEVELS (csrc/flx_trace4.h) stack entries per lane in LDS and moves deeper
ones to a global spill buffer.  A tree's depth bounds the stack; it does not make any ray reach that depth: traverse<> pushes only when BOTH
children pass the slab test, and a camera ray through a deep chain pierces a handful of leaf boxes.  Here the geometry makes every level push:

  deck of cards     triangle k of nt is (0,0,z_k) (2,0,z_k) (0,2,z_k), z_k = k * dz; hand-built right-leaning chain, inner node 2k = {leaf k, rest}.
                    A ray going DOWN through the deck finds "rest" (it reaches up to the top card) nearer than leaf k at every level and both
                    boxes hit: nt - 1 pushes.  Through the solid half (x, y) ~ (0.5, 0.5) it ends on the top card nt - 1; through the hole half
                    ~ (1.5, 1.5) it is inside every box and outside every triangle: it pushes everything, then pops everything.  Going UP, the
                    leaf is the nearer child: the binary stack and the 4-wide closest-hit stack stay shallow (the 4-wide any-hit orders still
                    climb: they do not go near-first).
  decks of decks    several decks stacked along z with a gap, joined by a right-leaning top chain: a hole ray from above climbs and empties once
                    per deck, so ONE ray pages out and back in several times, with 1, 2, 3, 3 entries pending below the decks.

The witness is computed on the host from the same nodes and rays -- no kernel reports its stack depth:
  binary_witness    traverse<>'s push / pop rule restated in numpy (fp32 slab test, Moller-Trumbore, tbest shrinking): per ray the peak sp and
                    the number of climbs past LDS_LEVELS
  wide_witness      tests/wide_analysis.cpp (fh_wide_visits_stack): the 4-wide traversal with the device's arithmetic; per ray the peak entry
                    count and the page-outs / page-ins WStack's ring rule implies, for the three visit orders
LDS_LEVELS and WIDE_LDS_LEVELS are read out of the two headers: a change of either moves the thresholds with it.
Used by tests/test_stack_spill.py (CPU) and tests/test_gpu_stack_spill.py."""
import ctypes as C
import os
import re
import numpy as np
import traversal_cases as tc
from fluctus_amd import wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"closest": 0, "any_last_slot": 1, "any_far_near": 2}        # tests/wide_analysis.cpp: mode
DEEP = ("deep_solid", "deep_hole")
SHALLOW = ("shallow_solid", "shallow_hole", "root_miss")
FAMILIES = DEEP + SHALLOW
DECKS = [30, 29, 31, 20]
SLANT = (0.003, 0.002)


def _define(header, name):
    src = open(os.path.join(ROOT, "fluctus_amd", "csrc", header)).read()
    m = re.findall(r"^\s*#\s*define\s+" + name + r"\s+(\d+)\b", src, re.M)
    assert len(m) == 1, f"{header}: expected exactly one '#define {name} <number>', found {len(m)}"
    return int(m[0])


LDS_LEVELS = _define("flx_trace.h", "LDS_LEVELS")
WIDE_LDS_LEVELS = _define("flx_trace4.h", "WIDE_LDS_LEVELS")
WIDE_NO_PAGE = WIDE_LDS_LEVELS - 4           # WStack::reserve pages out when MORE than this many entries sit above `base`


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
def deck_points(sizes, dz=0.125, gap=1.0, offset=(0.0, 0.0, 0.0), shift_every=0, shift_x=0.0):
    """(T, 3, 3) card positions of decks of `sizes` cards stacked along z (deck 0 lowest), dz apart inside a deck, `gap` between decks;
    every shift_every-th card (0: none) moved by shift_x along x."""
    P, z = [], 0.0
    for s in sizes:
        for k in range(s):
            P.append([(0.0, 0.0, z), (2.0, 0.0, z), (0.0, 2.0, z)])
            z += dz
        z += gap - dz
    P = np.array(P, np.float64) + np.asarray(offset, np.float64)
    if shift_every:
        P[::shift_every, :, 0] += shift_x
    return P


def chain_tree(sizes):
    """The topology as nested pairs: a deck is the right-leaning chain (card, (card, (... card))), the decks hang on a right-leaning top chain."""
    decks, t = [], 0
    for s in sizes:
        node = t + s - 1
        for k in range(t + s - 2, t - 1, -1):
            node = (k, node)
        decks.append(node); t += s
    top = decks[-1]
    for dk in decks[-2::-1]:
        top = (dk, top)
    return top


def chain_nodes(P, tree):
    """wire.NODE array in the builders' DFS order (left child at i + 1, right child at iStartOrRight), one triangle per leaf, exact fp32 boxes."""
    P32 = np.asarray(P, np.float32)
    nt = P32.shape[0]
    nodes = np.zeros(2 * nt - 1, wire.NODE)
    count = [0]

    def emit(t, parent):                                  # iterative on the right spine: the chains are a hundred levels deep
        first = None
        while True:
            i = count[0]; count[0] += 1
            first = i if first is None else first
            nodes[i]["parent"] = parent
            if isinstance(t, tuple):
                nodes[i]["nPrims"] = 0
                emit(t[0], i)
                nodes[i]["iStartOrRight"] = count[0]
                parent, t = i, t[1]
            else:
                nodes[i]["nPrims"] = 1; nodes[i]["iStartOrRight"] = t
                lo, hi = P32[t].min(0), P32[t].max(0)
                for j, a in enumerate("xyz"):
                    nodes[i]["bmin"][a] = lo[j]; nodes[i]["bmax"][a] = hi[j]
                return first
    emit(tree, -1)
    assert count[0] == nodes.size
    for i in range(nodes.size - 1, -1, -1):               # children come after their parent: one backward pass unions the boxes
        if nodes[i]["nPrims"] == 0:
            for ch in (i + 1, int(nodes[i]["iStartOrRight"])):
                for a in "xyz":
                    lo, hi = nodes[ch]["bmin"][a], nodes[ch]["bmax"][a]
                    if ch == i + 1:
                        nodes[i]["bmin"][a], nodes[i]["bmax"][a] = lo, hi
                    else:
                        nodes[i]["bmin"][a] = min(nodes[i]["bmin"][a], lo); nodes[i]["bmax"][a] = max(nodes[i]["bmax"][a], hi)
    return nodes


def deck_scene(sizes, **kw):
    """SceneData of the decks with the hand-built chain over them."""
    sizes = [sizes] if isinstance(sizes, int) else list(sizes)
    P = deck_points(sizes, **kw)
    d = tc.make_scene(P)
    d.nodes = chain_nodes(P, chain_tree(sizes))
    d.indices = np.arange(P.shape[0], dtype=np.uint32)
    set_radius(d)
    d.sizes = sizes
    return d


def set_radius(d):
    r = d.nodes[0]
    d.world_radius = float(0.5 * np.linalg.norm([float(r["bmax"][a]) - float(r["bmin"][a]) for a in "xyz"]))


def shallow_scene():
    """Two cards under a one-level tree: nothing spills (the re-sizing case starts from it)."""
    return deck_scene(2)


SCENES = {"deck41": lambda: deck_scene(41), "deck100": lambda: deck_scene(100), "decks": lambda: deck_scene(DECKS)}


# ---------------------------------------------------------------------------------------------------------------------------------
# rays
def family_rays(P, fam, n, seed=0):
    """n rays of one family aimed at the cards in P as they stand (so a moved or refitted deck gets re-aimed rays): (orig, dir, tmax) fp32.
    The rays cross the deck's mid height ~0.5 inside the region every card shares -- solid: inside every triangle; hole: inside every
    card's box, outside every triangle -- with a small jitter, so neither ties nor grazing hits."""
    P = np.asarray(P, np.float64)
    rng = np.random.RandomState(seed + 17 * FAMILIES.index(fam))
    z0, z1 = P[:, :, 2].min(), P[:, :, 2].max()
    x0, y0 = P[:, 0, 0].max(), P[:, 0, 1].max()               # the right-angle corners: solid rays stay 0.5 behind the farthest one
    x1, y1 = P[:, 1, 0].min(), P[:, 2, 1].min()               # the far corners: hole rays stay 0.5 inside the nearest one
    j = rng.uniform(0.0, 0.03, (n, 2))
    if fam.endswith("solid"):
        xy = np.array([x0 + 0.5, y0 + 0.5]) + j
    elif fam.endswith("hole"):
        xy = np.array([x1 - 0.5, y1 - 0.5]) - j
    else:
        xy = np.array([x1 + 8.0, y1 + 8.0]) + 100.0 * j       # beside the root box
    down = not fam.startswith("shallow")
    dz = -1.0 if down else 1.0
    dirs = np.tile(np.array([SLANT[0], SLANT[1], dz]), (n, 1))
    zs = (z1 + 1.0) if down else (z0 - 1.0)
    zm = 0.5 * (z0 + z1)
    orig = np.concatenate([xy - np.array(SLANT) * abs(zm - zs), np.full((n, 1), zs)], 1)
    tmax = np.full(n, 2.0 * (z1 - z0 + 2.0))
    return orig.astype(np.float32), dirs.astype(np.float32), tmax.astype(np.float32)


def mixed_queue(P, n, seed=0):
    """n rays laid out for the kernels' 64-ray blocks: lanes of a block cycle through deep, shallow and root-missing rays, every fourth block is
    all deep (alternating solid / hole), so the lanes of one wave sit in different paging states and a persistent wave refills a lane that has
    just paged.  Returns orig, dir, tmax and the family index per ray."""
    i = np.arange(n)
    fam = i % 64 % len(FAMILIES)
    alldeep = (i // 64) % 4 == 3
    fam = np.where(alldeep, i % 2, fam)
    orig, dirs, tmax = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    for f, name in enumerate(FAMILIES):
        m = fam == f
        orig[m], dirs[m], tmax[m] = family_rays(P, name, int(m.sum()), seed)
    return orig, dirs, tmax, fam


def expected_hits(P, fam):
    """What the geometry says: the top card for deep_solid, the bottom card for shallow_solid, nothing otherwise; (closest, blocked)."""
    z = np.asarray(P)[:, 0, 2]
    top, bottom = int(np.argmax(z)), int(np.argmin(z))
    closest = np.full(fam.shape, -1, np.int64)
    closest[fam == FAMILIES.index("deep_solid")] = top
    closest[fam == FAMILIES.index("shallow_solid")] = bottom
    return closest, closest >= 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the witness
def _slab32(lo, hi, o, dinv, tprev):
    with np.errstate(all="ignore"):
        a, b = (lo - o) * dinv, (hi - o) * dinv
        tmin, tmax = np.minimum(a, b).max(1), np.maximum(a, b).min(1)
    return ~(tmax < 0) & ~(tmin > tmax) & (tmin < tprev), tmin


def _mt32(o, d, p0, p1, p2):
    """csrc/flx_trace.h: moller_trumbore, fp32"""
    f = np.float32
    with np.errstate(all="ignore"):
        s1, s2 = p1 - p0, p2 - p0
        pv = np.cross(d, s2).astype(f)
        det = (s1 * pv).sum(1, dtype=f)
        inv = f(1.0) / det
        tv = o - p0
        u = (tv * pv).sum(1, dtype=f) * inv
        qv = np.cross(tv, s1).astype(f)
        v = (d * qv).sum(1, dtype=f) * inv
        t = (s2 * qv).sum(1, dtype=f) * inv
        ok = ~(np.abs(det) < f(1e-12)) & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & ~(t < 0)
    return ok, t


def binary_witness(d, orig, dirs, tmax, any_hit):
    """traverse<ANY_HIT> (csrc/flx_trace.h) on d.nodes, all rays at once: both children hit -> push the farther, go to the nearer; one hit ->
    go there; none -> pop; a leaf tests its triangles in index order against the shrinking tbest (any hit: the first one ends the ray), then
    pops.  Returns dict(peak=deepest sp, climbs=pushes that left the LDS levels (sp LDS_LEVELS -> LDS_LEVELS + 1), tri=closest triangle or
    first occluder, -1 none)."""
    nd = d.nodes
    lo = np.stack([nd["bmin"][a] for a in "xyz"], 1).astype(np.float32); hi = np.stack([nd["bmax"][a] for a in "xyz"], 1).astype(np.float32)
    right, nprims = nd["iStartOrRight"].astype(np.int64), nd["nPrims"].astype(np.int64)
    assert nd.size > 1 and nprims[0] == 0
    P = tc.tri_points(d).astype(np.float32)
    idx = d.indices.astype(np.int64)
    o, dd = np.asarray(orig, np.float32), np.asarray(dirs, np.float32)
    n = o.shape[0]
    with np.errstate(all="ignore"):
        dinv = np.float32(1.0) / dd
    tbest = np.asarray(tmax, np.float32).copy() if any_hit else np.full(n, tc.FLT_MAX, np.float32)
    cur, sp, peak, climbs, tri = (np.zeros(n, np.int64) for _ in range(5))
    tri -= 1
    stack = np.zeros((n, nd.size), np.int64)
    alive = np.ones(n, bool)

    def pop(a):
        e = sp[a] == 0
        alive[a[e]] = False
        a = a[~e]
        sp[a] -= 1
        cur[a] = stack[a, sp[a]]

    while alive.any():
        a = np.nonzero(alive)[0]
        inner = nprims[cur[a]] == 0
        ai = a[inner]
        if ai.size:
            l, r = cur[ai] + 1, right[cur[ai]]
            lh, ln = _slab32(lo[l], hi[l], o[ai], dinv[ai], tbest[ai])
            rh, rn = _slab32(lo[r], hi[r], o[ai], dinv[ai], tbest[ai])
            both, go_r = lh & rh, rn < ln
            b = ai[both]
            stack[b, sp[b]] = np.where(go_r, l, r)[both]
            climbs[b] += sp[b] == LDS_LEVELS
            sp[b] += 1
            peak[b] = np.maximum(peak[b], sp[b])
            cur[b] = np.where(go_r, r, l)[both]
            one = lh ^ rh
            cur[ai[one]] = np.where(lh, l, r)[one]
            pop(ai[~lh & ~rh])
        al = a[~inner]
        if al.size:
            done = np.zeros(al.size, bool)
            for k in range(int(nprims[cur[al]].max())):
                m = (k < nprims[cur[al]]) & ~done
                am = al[m]
                t_id = idx[right[cur[am]] + k]
                ok, t = _mt32(o[am], dd[am], P[t_id, 0], P[t_id, 1], P[t_id, 2])
                h = ok & (t > 0) & (t < tbest[am])
                tri[am[h]] = t_id[h]
                if any_hit:
                    done[np.nonzero(m)[0][h]] = True
                else:
                    tbest[am[h]] = t[h]
            alive[al[done]] = False
            pop(al[~done])
    return dict(peak=peak, climbs=climbs, tri=tri)


_lib = None


def wide_lib():
    """tests/wide_analysis.cpp, built by conftest.build_wide_analysis.  A build failure is an error here: without the emulation nothing says that
    the 4-wide kernels paged."""
    global _lib
    if _lib is None:
        import conftest
        _lib = C.CDLL(conftest.build_wide_analysis())
        _lib.fh_analysis_last_error.restype = C.c_char_p
    return _lib


def wide_witness(d, orig, dirs, tmax, mode, budget=0):
    """The 4-wide traversal of csrc/flx_trace4.h emulated on the tree flx_wide.h builds from d.nodes.  mode: MODES.  Closest hit ignores tmax
    (the kernels start from FLT_MAX).  Returns dict(peak, page_outs, page_ins, susp_sp, susp_base (where a node-visit budget ran out in front
    of an inner node; -1: never), tri, node_visits)."""
    L = wide_lib()
    mode = MODES[mode] if isinstance(mode, str) else mode
    t = np.full(orig.shape[0], tc.FLT_MAX, np.float32) if mode == 0 else tmax
    rays = tc.emulation_rays(orig, dirs, t)
    n = rays.shape[0]
    out = np.zeros(8, np.float64); tri = np.zeros(n, np.int32); nv = np.zeros(n, np.uint32); stk = np.zeros((n, 6), np.int32)
    nodes = np.ascontiguousarray(d.nodes)
    rc = L.fh_wide_visits_stack(nodes.ctypes.data_as(C.c_void_p), C.c_uint64(nodes.size), d.tris.ctypes.data_as(C.c_void_p), C.c_uint64(d.tris.size),
                                d.indices.ctypes.data_as(C.c_void_p), C.c_uint64(d.indices.size), rays.ctypes.data_as(C.c_void_p), C.c_uint64(n),
                                C.c_int(mode), C.c_int(WIDE_LDS_LEVELS), C.c_int(budget), out.ctypes.data_as(C.c_void_p), tri.ctypes.data_as(C.c_void_p),
                                nv.ctypes.data_as(C.c_void_p), stk.ctypes.data_as(C.c_void_p))
    assert rc == 0, L.fh_analysis_last_error()
    return dict(peak=stk[:, 0], page_outs=stk[:, 1], page_ins=stk[:, 2], susp_sp=stk[:, 3], susp_base=stk[:, 4], tri=tri, node_visits=nv)


def witness(d, orig, dirs, tmax):
    """Everything the tests assert on: {"binary_closest", "binary_any", "closest", "any_last_slot", "any_far_near"} -> per-ray figures."""
    w = {"binary_closest": binary_witness(d, orig, dirs, tmax, False), "binary_any": binary_witness(d, orig, dirs, tmax, True)}
    for m in MODES:
        w[m] = wide_witness(d, orig, dirs, tmax, m)
    return w


# Which families must be deep under which traversal.  Going down, "rest" is the nearer child at every level: the near-first orders (binary,
# 4-wide closest hit) push every level, and so does last-slot-first (the inner child sits in the last slot of every wide node of a chain).
# Far -> near descends into the FARTHEST child: going down that is the leaf (3 entries pending, never more), going up it is "rest" -- so that
# order pages on the rays that are shallow for everybody else, and last-slot-first pages in both directions.
DEEP_IN = {"binary_closest": DEEP, "binary_any": DEEP, "closest": DEEP, "any_last_slot": DEEP + SHALLOW[:2], "any_far_near": SHALLOW[:2]}


def check_thresholds(w, fam, what, min_cycles=1):
    """The conditions of the spill tests, per family and traversal (a failure, never a skip):
      deep (DEEP_IN)   every ray peaks above the LDS levels: binary peak > LDS_LEVELS with at least one climb, 4-wide more than
                       WIDE_LDS_LEVELS - 4 entries and at least one page-out; hole rays also come all the way back: at least min_cycles
                       cycles, 4-wide page-ins == page-outs
      everything else  stays at or below the thresholds: no spill, no paging
    Returns the table rows (family, kernel, rays, peak min, max, page-outs / climbs min, max, page-ins min, max)."""
    rows = []
    for f, name in enumerate(FAMILIES):
        m = fam == f
        if not m.any():
            continue
        for k, v in w.items():
            binary = k.startswith("binary")
            peak = v["peak"][m]
            outs = (v["climbs"] if binary else v["page_outs"])[m]
            ins = outs if binary else v["page_ins"][m]
            rows.append((name, k, int(m.sum()), int(peak.min()), int(peak.max()), int(outs.min()), int(outs.max()), int(ins.min()), int(ins.max())))
            tag = f"{what}/{name}/{k}"
            limit = LDS_LEVELS if binary else WIDE_NO_PAGE
            if name in DEEP_IN[k]:
                assert (peak > limit).all(), f"{tag}: a ray peaks at {int(peak.min())}: it never leaves the LDS levels"
                assert (outs >= 1).all(), f"{tag}: a ray without a spill / page-out"
                if name.endswith("hole"):
                    assert (outs >= min_cycles).all(), f"{tag}: {int(outs.min())} spill cycles, expected at least {min_cycles}"
                    assert np.array_equal(ins, outs), f"{tag}: a hole ray empties its stack: every page-out pages back in"
            else:
                assert (peak <= limit).all(), f"{tag}: a shallow ray peaks at {int(peak.max())}"
                assert (outs == 0).all() and (ins == 0).all(), f"{tag}: a shallow ray spills"
    return rows


def format_rows(what, rows):
    head = f"{what}: family / kernel / rays / peak depth / page-outs (binary: climbs past LDS_LEVELS) / page-ins"
    return "\n".join([head] + [f"  {r[0]:14s} {r[1]:15s} {r[2]:6d}  peak {r[3]:3d}..{r[4]:<3d}  out {r[5]:2d}..{r[6]:<2d}  in {r[7]:2d}..{r[8]:<2d}" for r in rows])
