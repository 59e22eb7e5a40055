"""ctypes binding of libfluctus_host.so (C++ scene / BVH / env-map preparation)."""
import ctypes as C
import os
import numpy as np
from .wire import TRIANGLE, NODE, MATERIAL, TEXDESC

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        try:                              # see device._preload_torch_runtime: the C++ HipContext dlopens libfluctus_hip.so later
            import torch  # noqa: F401
        except Exception:
            pass
        path = os.path.join(_HERE, "libfluctus_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing -- run `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = C.CDLL(path)
        _lib.fh_last_error.restype = C.c_char_p
    return _lib


def _chk(rc):
    if rc != 0:
        raise RuntimeError("libfluctus_host: " + lib().fh_last_error().decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class SceneData:
    """Triangles/materials/textures in wire format + BVH arrays."""

    def __init__(self):
        self.tris = self.materials = self.texdesc = self.texdata = None
        self.nodes = self.indices = None
        self.world_radius = 1.0
        self.type_bits = 0
        self.world_up = (0.0, 1.0, 0.0)
        self.bvh_metrics = None
        self.object_of_triangle = None      # per triangle: index into object_names, 0xFFFFFFFF = none (OBJ `o` / `g` statements)
        self.object_names = []


def _scene_to_data(h):
    L = lib()
    nt, nm, nx, tb, bits = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
    _chk(L.fh_scene_counts(h, C.byref(nt), C.byref(nm), C.byref(nx), C.byref(tb), C.byref(bits)))
    d = SceneData()
    d.tris = np.zeros(nt.value, TRIANGLE)
    d.materials = np.zeros(nm.value, MATERIAL)
    d.texdesc = np.zeros(nx.value, TEXDESC)
    d.texdata = np.zeros(tb.value, np.uint8)
    _chk(L.fh_scene_get(h, _p(d.tris), _p(d.materials), _p(d.texdesc), _p(d.texdata)))
    d.type_bits = bits.value
    up = np.zeros(3, np.float32)
    L.fh_scene_world_up(h, up.ctypes.data_as(C.c_void_p))
    d.world_up = tuple(float(x) for x in up)
    # Scene::objectOfTriangle / objectNames: the OBJ loader's objects (NO_OBJECT = 0xFFFFFFFF: none)
    d.object_of_triangle = np.full(nt.value, 0xFFFFFFFF, np.uint32)
    nobj, need = C.c_uint32(), C.c_uint64()
    _chk(L.fh_scene_objects(h, _p(d.object_of_triangle), C.byref(nobj), None, C.c_uint64(0), C.byref(need)))
    buf = C.create_string_buffer(int(need.value))
    _chk(L.fh_scene_objects(h, None, None, buf, C.c_uint64(need.value), None))
    d.object_names = buf.value.decode().split("\n")[:-1] if nobj.value else []
    return d


def load_scene(path):
    L = lib()
    h = C.c_void_p()
    _chk(L.fh_scene_create(C.byref(h)))
    try:
        _chk(L.fh_scene_load(h, path.encode()))
        return _scene_to_data(h)
    finally:
        L.fh_scene_destroy(h)


def generate_scene(kind, target_tris, seed):
    L = lib()
    h = C.c_void_p()
    _chk(L.fh_scene_create(C.byref(h)))
    try:
        _chk(L.fh_scene_generate(h, kind.encode(), C.c_uint32(target_tris), C.c_uint32(seed)))
        return _scene_to_data(h)
    finally:
        L.fh_scene_destroy(h)


def load_png(path):
    """RGBA8 texture, lower-left origin (row 0 = bottom scanline), as the reference's DevIL setup delivers it."""
    L = lib()
    w, h = C.c_uint32(), C.c_uint32()
    _chk(L.fh_png_load(path.encode(), C.byref(w), C.byref(h), None))
    out = np.zeros((h.value, w.value, 4), np.uint8)
    _chk(L.fh_png_load(path.encode(), C.byref(w), C.byref(h), out.ctypes.data_as(C.c_void_p)))
    return out


load_texture = load_png      # PNG or JPEG, decided by the file signature


def decode_jpeg(data):
    """JPEG bytes -> (h, w, 3) uint8, top-left origin: the bytes libjpeg's default decode path produces."""
    L = lib()
    buf = np.frombuffer(bytes(data), np.uint8)
    w, h = C.c_uint32(), C.c_uint32()
    _chk(L.fh_jpeg_decode(buf.ctypes.data_as(C.c_void_p), C.c_uint64(buf.size), C.byref(w), C.byref(h), None, C.c_uint64(0)))
    out = np.zeros((h.value, w.value, 3), np.uint8)
    _chk(L.fh_jpeg_decode(buf.ctypes.data_as(C.c_void_p), C.c_uint64(buf.size), C.byref(w), C.byref(h), out.ctypes.data_as(C.c_void_p), C.c_uint64(out.size)))
    return out


BVH_MODES = {"sbvh": 0, "sah": 1, "binned": 2}


def build_bvh(d, mode="sbvh", threads=0, job_size=0):
    """threads: 0 = all usable cores (the SBVH builder is parallel; the tree does not depend on the thread count), 1 = serial."""
    L = lib()
    h = C.c_void_p()
    _chk(L.fh_bvh_build_ex(_p(d.tris), C.c_uint64(d.tris.size), BVH_MODES[mode], int(threads), C.c_uint64(job_size), C.byref(h)))
    try:
        nn, ni = C.c_uint64(), C.c_uint64()
        met = (C.c_uint32 * 4)()
        _chk(L.fh_bvh_counts(h, C.byref(nn), C.byref(ni), met))
        d.nodes = np.zeros(nn.value, NODE)
        d.indices = np.zeros(ni.value, np.uint32)
        wr = C.c_float()
        _chk(L.fh_bvh_get(h, _p(d.nodes), _p(d.indices), C.byref(wr)))
        d.world_radius = wr.value
        d.bvh_metrics = dict(depth=met[0], splits=met[1], duplicates=met[2], spatial_splits=met[3])
    finally:
        L.fh_bvh_destroy(h)
    return d


def wide_tree_check(d):
    """Build the traversal kernels' 4-wide quantised tree (csrc/flx_wide.h -- what flx_upload_scene builds) on the CPU and check its
    invariants: conservative quantised boxes, every binary leaf exactly once with its box / count / triangle order, every wide node
    reachable once, unused slots inverted.  Raises on a violation; returns the tree's figures."""
    out = (C.c_uint64 * 8)()
    areas = (C.c_double * 2)()
    _chk(lib().fh_wide_tree_areas(_p(d.nodes), C.c_uint64(d.nodes.size), _p(d.tris), C.c_uint64(d.tris.size),
                                  _p(d.indices), C.c_uint64(d.indices.size), out, areas))
    return dict(area_exact=areas[0], area_quantised=areas[1], wide_nodes=out[0], leaf_float4s=out[1], max_stack=out[2], nested=bool(out[3]), leaves=out[4],
                slots_used={2: out[5], 3: out[6], 4: out[7]})


def refit_bvh(d):
    """BVH::refit: new boxes for d.nodes from d.tris over the SAME topology and index list (leaf = union of the full bounds of its triangles,
    inner = union of its two children), in place; d.world_radius follows the new root box.  The CPU restatement of the device refit
    (HipContext.update_triangles), bit for bit."""
    wr = C.c_float()
    _chk(lib().fh_bvh_refit(_p(d.nodes), C.c_uint64(d.nodes.size), _p(d.indices), C.c_uint64(d.indices.size), _p(d.tris), C.c_uint64(d.tris.size), C.byref(wr)))
    d.world_radius = wr.value
    return d


def refit_bvh_subset(d, indices):
    """BVH::refitSubset: d.tris is the full array with the moved triangles already in place, indices lists them (strictly ascending).  A leaf
    holding a listed triangle becomes the union of the full bounds of its triangles, an inner node with a changed child the union of its two
    children, every other node of d.nodes keeps its bytes; in place, d.world_radius follows the root box.  The CPU restatement of
    HipContext.update_triangles_subset, bit for bit.  Raises, and leaves d.nodes untouched, on a malformed tree or list."""
    wr = C.c_float()
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    _chk(lib().fh_bvh_refit_subset(_p(d.nodes), C.c_uint64(d.nodes.size), _p(d.indices), C.c_uint64(d.indices.size), _p(d.tris), C.c_uint64(d.tris.size),
                                   _p(idx), C.c_uint64(idx.size), C.byref(wr)))
    d.world_radius = wr.value
    return d


def pose_triangles(rest_tris, xform):
    """csrc/flx_pose.h on the CPU -- what HipContext.objects_pose computes on the device, bit for bit: the wire triangles rest_tris posed by
    the 3 x 4 row-major affine transform xform = [M | t] (positions through [M | t], normals through the cofactor matrix of M, turned round
    when det M < 0, and renormalised; texcoords, matId and the spare words copied).  Returns a new array."""
    t = np.ascontiguousarray(rest_tris, TRIANGLE).reshape(-1)
    x = np.ascontiguousarray(xform, np.float32).reshape(-1)
    if x.size != 12:
        raise ValueError("pose_triangles: a 3 x 4 matrix")
    out = np.zeros(t.size, TRIANGLE)
    _chk(lib().fh_pose_triangles(_p(t), _p(out), C.c_uint64(t.size), _p(x)))
    return out


def _tris_mats(d):
    from .wire import TRIANGLE as T, MATERIAL as M
    return np.ascontiguousarray(d.tris, T).reshape(-1), np.ascontiguousarray(d.materials, M).reshape(-1)


def mesh_light_table(d):
    """csrc/flx_mesh_light.h on the CPU -- what HipContext.mesh_lights_read returns for the same triangles and materials, byte for byte:
    (tris uint32 ascending, cdf float32, pick float32, total float64) of the emissive triangles of d; four empty / zero results when d has no
    light (no emissive triangle with a positive weight)."""
    t, m = _tris_mats(d)
    n, total = C.c_uint32(), C.c_double()
    _chk(lib().fh_mesh_light_table(_p(t), C.c_uint64(t.size), _p(m), C.c_uint64(m.size), C.byref(n), None, None, None, C.byref(total)))
    tri, cdf, pick = np.zeros(n.value, np.uint32), np.zeros(n.value, np.float32), np.zeros(n.value, np.float32)
    _chk(lib().fh_mesh_light_table(_p(t), C.c_uint64(t.size), _p(m), C.c_uint64(m.size), C.byref(n), _p(tri), _p(cdf), _p(pick), C.byref(total)))
    return tri, cdf, pick, float(total.value)


def mesh_light_pick(cdf, pick, r):
    """ml_pick of csrc/flx_mesh_light.h over a table: the light picked for every r (float32)"""
    cdf, pick = np.ascontiguousarray(cdf, np.float32), np.ascontiguousarray(pick, np.float32)
    r = np.ascontiguousarray(r, np.float32).reshape(-1)
    out = np.zeros(r.size, np.uint32)
    _chk(lib().fh_mesh_light_pick(_p(cdf), _p(pick), C.c_uint32(cdf.size), _p(r), C.c_uint64(r.size), _p(out)))
    return out


def mesh_light_find(tris, query):
    """ml_find of csrc/flx_mesh_light.h: the position of every queried triangle in the ascending list, 0xFFFFFFFF = not a light"""
    lst, q = np.ascontiguousarray(tris, np.uint32), np.ascontiguousarray(query, np.uint32).reshape(-1)
    out = np.zeros(q.size, np.uint32)
    _chk(lib().fh_mesh_light_find(_p(lst), C.c_uint32(lst.size), _p(q), C.c_uint64(q.size), _p(out)))
    return out


def mesh_light_sample(d, r3):
    """What HipContext.mesh_lights_sample computes on the device, on the CPU: r3 (n, 3) float32 triples (pick, r1, r2) ->
    (light (n,) uint32, out8 (n, 8) float32 = P.xyz, pdfA, n_g.xyz, area, bary (n, 3) float32 the coefficients of P)"""
    t, m = _tris_mats(d)
    r = np.ascontiguousarray(r3, np.float32).reshape(-1, 3)
    light, out8, bary = np.zeros(r.shape[0], np.uint32), np.zeros((r.shape[0], 8), np.float32), np.zeros((r.shape[0], 3), np.float32)
    _chk(lib().fh_mesh_light_sample(_p(t), C.c_uint64(t.size), _p(m), C.c_uint64(m.size), _p(r), C.c_uint64(r.shape[0]), _p(light), _p(out8), _p(bary)))
    return light, out8, bary


def _bvh_arrays(h):
    """(nodes, indices, world radius) of a BVH handle"""
    L = lib()
    nn, ni = C.c_uint64(), C.c_uint64()
    _chk(L.fh_bvh_counts(h, C.byref(nn), C.byref(ni), None))
    nodes, idx = np.zeros(nn.value, NODE), np.zeros(ni.value, np.uint32)
    wr = C.c_float()
    _chk(L.fh_bvh_get(h, _p(nodes), _p(idx), C.byref(wr)))
    return nodes, idx, wr.value


class RebuildJob:
    """RebuildJob (host/rebuild_job.hpp): one BVH build on a worker thread over a snapshot of the triangles; GPU-free.
    start(tris, mode) / ready() / wait() / take() -> (nodes, indices, snapshot triangles); close() joins."""

    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p()
        _chk(self.L.fh_rebuild_job_create(C.byref(self.h)))

    def close(self):
        if self.h:
            self.L.fh_rebuild_job_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def start(self, tris, mode="sbvh", threads=0):
        t = np.ascontiguousarray(getattr(tris, "tris", tris), TRIANGLE).reshape(-1)
        _chk(self.L.fh_rebuild_job_start(self.h, _p(t), C.c_uint64(t.size), BVH_MODES[mode], int(threads)))
        self._n = t.size

    def ready(self):
        return bool(self.L.fh_rebuild_job_ready(self.h))

    def wait(self):
        _chk(self.L.fh_rebuild_job_wait(self.h))

    def hold(self, on):
        """test hook: while held, a finished build stays unpublished (ready() is False); wait() releases it"""
        _chk(self.L.fh_rebuild_job_hold(self.h, int(bool(on))))

    def take(self):
        b, n = C.c_void_p(), C.c_uint64()
        snap = np.zeros(getattr(self, "_n", 0), TRIANGLE)
        _chk(self.L.fh_rebuild_job_take(self.h, C.byref(b), _p(snap), C.c_uint64(snap.size), C.byref(n)))
        try:
            nodes, idx, _ = _bvh_arrays(b)
        finally:
            self.L.fh_bvh_destroy(b)
        return nodes, idx, snap[:n.value]


def tree_cost_binary(bnodes, blevel, trirecs):
    """The binary tree's (A_root, S_node, S_leaf, S_tri) on the CPU with the very functions flx_tree_cost's kernel runs (csrc/flx_tree_cost.h):
    bnodes / trirecs as HipContext.tree_read(0) / (1) return them, blevel the reachable record numbers, the root's first."""
    bn, tr = np.ascontiguousarray(bnodes, np.uint32), np.ascontiguousarray(trirecs, np.uint32)
    lst = np.ascontiguousarray(blevel, np.uint32)
    out = np.zeros(4, np.float64)
    _chk(lib().fh_tree_cost_binary(_p(bn), _p(lst), C.c_uint64(lst.size), _p(tr), C.c_uint64(tr.size // 12), _p(out)))
    return tuple(float(v) for v in out)


def tree_cost_value(sums4):
    """flxTreeCostValue of include/fluctus_hip.h, compiled into the host library"""
    L = lib()
    L.fh_tree_cost_value.restype = C.c_double
    s = np.ascontiguousarray(sums4, np.float64)
    assert s.size == 4
    return float(L.fh_tree_cost_value(_p(s)))


def wide_quantise(cmin, cmax, device_arithmetic=False):
    """The grid of one 4-wide node from its (ns, 3) child boxes: (o, s, qlo, qhi), three values each (qlo / qhi: byte k = child k).
    device_arithmetic False: build_wide's quantiser (csrc/flx_wide.h); True: the refit's fp64 restatement (csrc/flx_refit.h)."""
    cmin, cmax = np.ascontiguousarray(cmin, np.float32), np.ascontiguousarray(cmax, np.float32)
    out = np.zeros(12, np.uint32)
    _chk(lib().fh_wide_quantise(int(bool(device_arithmetic)), _p(cmin), _p(cmax), int(cmin.shape[0]), _p(out)))
    return out[0:3].view(np.float32).copy(), out[3:6].view(np.float32).copy(), out[6:9].copy(), out[9:12].copy()


def wide_tables_check(d):
    """build_wide's parent, depth and leaf tables (what a refit schedules from) checked against the child refs; (wide nodes, leaf blocks)"""
    out = (C.c_uint64 * 2)()
    _chk(lib().fh_wide_tables_check(_p(d.nodes), C.c_uint64(d.nodes.size), _p(d.tris), C.c_uint64(d.tris.size), _p(d.indices), C.c_uint64(d.indices.size), out))
    return int(out[0]), int(out[1])


def bvh_export(d, path, mode="sbvh"):
    """Build and write the hierarchy cache file (the reference's on-disk format, host/bvh.hpp)."""
    L = lib()
    h = C.c_void_p()
    _chk(L.fh_bvh_build(_p(d.tris), C.c_uint64(d.tris.size), BVH_MODES[mode], C.byref(h)))
    try:
        _chk(L.fh_bvh_export(h, path.encode()))
    finally:
        L.fh_bvh_destroy(h)


def bvh_import(path):
    """(nodes, indices) read back from a hierarchy cache file."""
    L = lib()
    h = C.c_void_p()
    _chk(L.fh_bvh_import(path.encode(), C.byref(h)))
    try:
        nn, ni = C.c_uint64(), C.c_uint64()
        met = (C.c_uint32 * 4)()
        _chk(L.fh_bvh_counts(h, C.byref(nn), C.byref(ni), met))
        nodes, idx = np.zeros(nn.value, NODE), np.zeros(ni.value, np.uint32)
        wr = C.c_float()
        _chk(L.fh_bvh_get(h, _p(nodes), _p(idx), C.byref(wr)))
        bvh_import.world_radius = wr.value           # of the last import (root box), same arithmetic as a fresh build
        return nodes, idx
    finally:
        L.fh_bvh_destroy(h)


def bvh_export_arrays(d, path):
    """Write d.nodes / d.indices as a hierarchy cache file without rebuilding (same bytes as BVH::exportTo)."""
    rec = np.zeros(d.nodes.size, np.dtype([("box", "<f4", 6), ("istart", "<u4"), ("parent", "<i4"), ("nprims", "u1")]))
    for k, ax in enumerate("xyz"):
        rec["box"][:, k] = d.nodes["bmin"][ax]
        rec["box"][:, 3 + k] = d.nodes["bmax"][ax]
    rec["istart"], rec["parent"], rec["nprims"] = d.nodes["iStartOrRight"], d.nodes["parent"], d.nodes["nPrims"]
    with open(path, "wb") as f:
        f.write(np.uint32(d.indices.size).tobytes()); f.write(np.ascontiguousarray(d.indices, "<u4").tobytes())
        f.write(np.uint32(d.nodes.size).tobytes()); f.write(rec.tobytes())


def xxh64(data, seed=0):
    L = lib()
    L.fh_xxh64.restype = C.c_uint64
    buf = np.frombuffer(bytes(data), np.uint8)
    return int(L.fh_xxh64(buf.ctypes.data_as(C.c_void_p) if buf.size else None, C.c_uint64(buf.size), C.c_uint64(seed)))


class EnvMap:
    def __init__(self, w, h, rgb, prob, alias, pdf):
        self.w, self.h, self.rgb, self.prob, self.alias, self.pdf = w, h, rgb, prob, alias, pdf


def _env_to_py(h):
    L = lib()
    w, hh = C.c_int(), C.c_int()
    L.fh_envmap_dims(h, C.byref(w), C.byref(hh))
    n = w.value * hh.value
    rgb = np.zeros(n * 3, np.float32)
    prob = np.zeros(n, np.float32)
    alias = np.zeros(n, np.int32)
    pdf = np.zeros(n, np.float32)
    _chk(L.fh_envmap_get(h, _p(rgb), _p(prob), _p(alias), _p(pdf)))
    return EnvMap(w.value, hh.value, rgb, prob, alias, pdf)


def load_envmap(path):
    L = lib()
    h = C.c_void_p()
    _chk(L.fh_envmap_load(path.encode(), C.byref(h)))
    try:
        return _env_to_py(h)
    finally:
        L.fh_envmap_destroy(h)


def envmap_from_rgb(w, h, rgb):
    L = lib()
    hd = C.c_void_p()
    rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1)
    _chk(L.fh_envmap_from_memory(w, h, _p(rgb), C.byref(hd)))
    try:
        return _env_to_py(hd)
    finally:
        L.fh_envmap_destroy(hd)


def synthetic_sky(w=512, h=256, seed=7):
    """Deterministic HDR sky (gradient + a few bright lobes): the env map that travels to the GPU
    box, where /root/reference (assets/env_maps/night.hdr) does not exist."""
    v = (np.arange(h, dtype=np.float32) + 0.5) / h
    u = (np.arange(w, dtype=np.float32) + 0.5) / w
    uu, vv = np.meshgrid(u, v)
    up = np.clip(1.0 - 2.0 * vv, 0.0, 1.0)
    img = np.stack([0.25 + 0.35 * up, 0.35 + 0.45 * up, 0.55 + 0.75 * up], -1).astype(np.float32)
    img[vv > 0.5] *= 0.25
    rng = np.random.RandomState(seed)
    for _ in range(4):
        cu, cv, s, a = rng.uniform(0, 1), rng.uniform(0.1, 0.4), rng.uniform(0.01, 0.04), rng.uniform(20, 200)
        du = np.minimum(np.abs(uu - cu), 1.0 - np.abs(uu - cu))
        img += (a * np.exp(-((du ** 2) + (vv - cv) ** 2) / (2 * s * s)))[..., None].astype(np.float32) * \
            np.array([1.0, 0.9, 0.7], np.float32)
    return envmap_from_rgb(w, h, img.astype(np.float32))
