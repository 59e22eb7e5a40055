"""numpy float64 restatement of flx_tree_cost (csrc/flx_tree_cost.h), in two forms.

(a) device_sums(bnodes, trirecs, wnodes, wleaf): from the arrays of HipContext.tree_read (0, 1, 3, 4), by the rules of the header: the records a
    traversal can reach from the root, each half / used slot a child box, A(box) = 2 (dx dy + dy dz + dz dx).
(b) host_sums(nodes): for the BINARY tree only and independently of the device layout, from a host flx_node array: A(root); S_node = A(root) + the
    areas of the inner nodes below the root; S_leaf = the leaf areas; S_tri = leaf area x nPrims.  A one-leaf scene is outside (b): the device's
    synthetic root tests the only leaf's box in BOTH halves and both count, so its S_leaf and S_tri are twice what the node array says.

Every term is positive and carries a few fp64 roundings, and the sums are taken with math.fsum (correctly rounded), so (a) and (b) are good to
a few ulps: any reduction order of the device's agrees with them to about n 2^-53 relative (tests/test_gpu_tree_cost.py: 1e-9).
"""
import math
import numpy as np

LEAF_BIT = 0x80000000
OFF_MASK = 0x7FFFFFFF


def area(mn, mx):
    """(n, 3) fp32 corners -> (n,) float64 areas"""
    d = np.asarray(mx, np.float64) - np.asarray(mn, np.float64)
    return 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])


def cost_value(sums4):
    """the header's helper: (S_node + S_tri) / A_root, NaN unless A_root is positive and finite"""
    a, s_node, _, s_tri = sums4
    if not (a > 0.0) or math.isinf(a):
        return float("nan")
    return (s_node + s_tri) / a


def reachable_binary(bn):
    """record numbers a traversal reaches from record 0, the root first (what RefitTables::blevel lists)"""
    out, level = [], np.array([0], np.int64)
    while level.size:
        out.append(level)
        refs = bn[level][:, 12:14].reshape(-1)
        level = np.unique(refs[(refs & LEAF_BIT) == 0]).astype(np.int64)
        assert not np.isin(level, np.concatenate(out)).any(), "a record reachable twice"
    return np.concatenate(out)


def binary_sums(bn, tr):
    bn, tr = np.asarray(bn, np.uint32).reshape(-1, 16), np.asarray(tr, np.uint32).reshape(-1, 12)
    recs = reachable_binary(bn)
    f = bn[recs][:, :12].view(np.float32).reshape(-1, 2, 2, 3)              # record, half, {min, max}, axis
    refs = bn[recs][:, 12:14]
    a = area(f[:, :, 0], f[:, :, 1])                                        # (records, 2)
    leaf = (refs & LEAF_BIT) != 0
    counts = np.where(leaf, tr[np.where(leaf, refs & OFF_MASK, 0), 7], 0).astype(np.float64)
    root = f[0]
    a_root = float(area(np.minimum(root[0, 0], root[1, 0])[None], np.maximum(root[0, 1], root[1, 1])[None])[0])
    return (a_root, math.fsum(a[~leaf]) + a_root, math.fsum(a[leaf]), math.fsum((a * counts)[leaf]))


def _header_area_count(wl, off):
    return area(wl[off, :3].view(np.float32), wl[off + 1, :3].view(np.float32)), wl[off, 3].astype(np.float64)


def wide_sums(wn, wl):
    wn, wl = np.asarray(wn, np.uint32).reshape(-1, 16), np.asarray(wl, np.uint32).reshape(-1, 4)
    if wn.shape[0] == 1 and not wn.any():                                    # no wide node (a real one has power-of-two scales): the root is the leaf block
        a, n = _header_area_count(wl, np.array([5]))                        # ... behind the dummy leaf's five float4
        return (float(a[0]), 0.0, float(a[0]), float(a[0] * n[0]))
    out, level = [], np.array([0], np.int64)
    while level.size:
        out.append(level)
        refs = wn[level][:, 6:10].reshape(-1)
        level = np.unique(refs[(refs & LEAF_BIT) == 0]).astype(np.int64)
    nodes = wn[np.concatenate(out)]
    s = nodes[:, 3:6].view(np.float32).astype(np.float64)                   # (nodes, axis)
    refs = nodes[:, 6:10]
    k = np.arange(4, dtype=np.uint32) * 8
    qlo = ((nodes[:, 10:13, None] >> k) & 255).astype(np.float64)            # (nodes, axis, slot)
    qhi = ((nodes[:, 13:16, None] >> k) & 255).astype(np.float64)
    used = refs != LEAF_BIT
    ext = (qhi - qlo) * s[:, :, None]                                       # the decoded box [o + qlo s, o + qhi s]: its extent is exact in fp64
    a = 2.0 * (ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 2] * ext[:, 0])   # (nodes, slot)
    leaf = used & ((refs & LEAF_BIT) != 0)
    inner = used & ~leaf
    ha, hn = _header_area_count(wl, (refs & OFF_MASK)[leaf])
    r_used = used[0]
    rext = (qhi[0][:, r_used].max(1) - qlo[0][:, r_used].min(1)) * s[0]
    a_root = float(2.0 * (rext[0] * rext[1] + rext[1] * rext[2] + rext[2] * rext[0]))
    return (a_root, math.fsum(a[inner]) + a_root, math.fsum(a[leaf]), math.fsum(ha * hn))


def device_sums(bnodes, trirecs, wnodes, wleaf):
    """(a): ((A_root, S_node, S_leaf, S_tri) of the binary tree, the same of the 4-wide tree)"""
    return binary_sums(bnodes, trirecs), wide_sums(wnodes, wleaf)


def host_sums(nodes):
    """(b): the binary tree's four sums from a host flx_node array (at least one inner node)"""
    mn = np.stack([nodes["bmin"][k] for k in "xyz"], -1)
    mx = np.stack([nodes["bmax"][k] for k in "xyz"], -1)
    a = area(mn, mx)
    n = nodes["nPrims"].astype(np.float64)
    leaf = nodes["nPrims"] > 0
    assert not leaf[0], "a one-leaf scene has no inner node: the device sums its synthetic root (see the module docstring)"
    return (float(a[0]), math.fsum(a[~leaf]), math.fsum(a[leaf]), math.fsum((a * n)[leaf]))
