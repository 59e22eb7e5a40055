"""ctypes binding of libfluctus_hip.so (include/fluctus_hip.h).

HipContext mirrors the reference's CLContext method for method (reference: src/clcontext.hpp:31-79):
uploadSceneData -> upload_scene, createEnvMap -> upload_envmap, updateParams -> set_params,
enqueueWf*Kernel -> wf_*, enqueueClearWfQueues -> clear_queues, enqueueGetCounters -> get_counters,
finishQueue -> finish, updatePixelIndex/resetPixelIndex -> pixel_index_update/reset.
There is NO CPU fallback: without the library or without a GPU every call raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

# every symbol include/fluctus_hip.h declares (checked by tests/test_abi.py against the header)
SYMBOLS = ["flx_create", "flx_destroy", "flx_last_error", "flx_upload_scene", "flx_upload_envmap", "flx_set_params",
           "flx_wf_reset", "flx_wf_raygen", "flx_wf_extend", "flx_wf_shadow", "flx_wf_logic", "flx_wf_materials",
           "flx_clear_queues", "flx_get_counters_async", "flx_finish", "flx_pixel_index_update", "flx_pixel_index_reset",
           "flx_end_iteration_async", "flx_counter_totals", "flx_num_tasks", "flx_postprocess", "flx_read_pixels", "flx_set_partition", "flx_local_pixels",
           "flx_copy_pixels_to_device", "flx_stream", "flx_group_unique_id", "flx_group_init", "flx_group_init_local", "flx_gather", "flx_gather_local", "flx_group_destroy", "flx_group_info", "flx_profile_enable", "flx_profile_get", "flx_profile_reset",
           "flx_trace_stats_enable", "flx_trace_stats_get", "flx_trace_stats_get_ex", "flx_trace_stats_get_all", "flx_scene_info", "flx_trace_stats_reset", "flx_state_export", "flx_state_import", "flx_math_probe", "flx_env_sample_table",
           "flx_queue_read", "flx_queue_write", "flx_set_counters", "flx_set_option", "flx_get_option", "flx_mk_reset", "flx_mk_raygen", "flx_mk_next_vertex",
           "flx_mk_sample_bsdf", "flx_mk_splat", "flx_mk_splat_preview", "flx_mk_stats_async", "flx_mk_stats_reset", "flx_write_pixels", "flx_denoise",
           "flx_denoise_variance_guided", "flx_gbuffer", "flx_history_capture", "flx_reproject", "flx_gbuffer_read", "flx_gbuffer_write",
           "flx_mk_adaptive_update", "flx_mk_adaptive_clear", "flx_mk_active_read", "flx_mk_active_write",
           "flx_update_triangles", "flx_update_triangles_subset", "flx_tree_read", "flx_tree_cost",
           "flx_objects_define", "flx_objects_pose", "flx_objects_read", "flx_gbuffer_objects_read", "flx_gbuffer_objects_write",
           "flx_gbuffer_bary_read", "flx_gbuffer_bary_write", "flx_deform_read",
           "flx_history_mark", "flx_history_rectify", "flx_history_mark_read",
           "flx_mesh_lights_read", "flx_mesh_lights_sample"]

KERNELS = {"reset": 0, "raygen": 1, "extend": 2, "shadow": 3, "logic": 4, "materials": 5, "postprocess": 6, "trace_span": 7, "logic_fused": 8}
K_DENOISE = 9           # FLX_K_DENOISE: timed with profile level 1, read with HipContext.denoise_profile (not part of profile_get)
K_GBUFFER, K_REPROJECT = 10, 11      # FLX_K_GBUFFER / FLX_K_REPROJECT: profile level 1, read with HipContext.kernel_profile
K_REFIT = 12                         # FLX_K_REFIT: the kernels of update_triangles, likewise
K_TREE_COST = 13                     # FLX_K_TREE_COST: the kernels of tree_cost, likewise
K_SNAPSHOT, K_MOVED_FLAGS = 14, 15   # FLX_K_SNAPSHOT / FLX_K_MOVED_FLAGS: option "deform_history"'s snapshot and flag passes, likewise
K_RECTIFY = 16                       # FLX_K_RECTIFY: the two kernels of history_rectify, likewise
NO_OBJECT = 0xFFFFFFFF            # FLX_NO_OBJECT: a triangle that belongs to no object (objects_define)


def tree_cost_value(sums4):
    """flxTreeCostValue (include/fluctus_hip.h): (S_node + S_tri) / A_root of four sums of tree_cost -- the two-constant surface-area heuristic
    with both constants 1; NaN when A_root is not a positive finite number ("no decision")"""
    a, s_node, _, s_tri = (float(v) for v in sums4)
    if not (a > 0.0) or a == float("inf"):
        return float("nan")
    return (s_node + s_tri) / a


class DenoiseParams(C.Structure):
    """flx_denoise_params (include/fluctus_hip.h)"""
    _fields_ = [("iterations", C.c_int), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("blend", C.c_float)]


# the library's defaults (FLX_DN_DEFAULT_*, csrc/flx_denoise.h)
DENOISE_DEFAULTS = dict(iterations=5, sigma_color=2.0, sigma_normal=0.3, sigma_albedo=0.1, blend=0.0)


class DenoiseVgParams(C.Structure):
    """flx_denoise_vg_params (include/fluctus_hip.h)"""
    _fields_ = [("iterations", C.c_int), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("blend", C.c_float)]


# the library's defaults (FLX_VG_DEFAULT_*, csrc/flx_denoise_vg.h)
DENOISE_VG_DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.3, sigma_albedo=0.1, blend=0.0)


class ReprojectParams(C.Structure):
    """flx_reproject_params (include/fluctus_hip.h)"""
    _fields_ = [("max_history", C.c_float), ("plane_tolerance_px", C.c_float), ("normal_cos", C.c_float), ("min_weight", C.c_float)]


# the library's defaults (FLX_RP_DEFAULT_*, csrc/flx_reproject.h)
REPROJECT_DEFAULTS = dict(max_history=32.0, plane_tolerance_px=2.0, normal_cos=0.9, min_weight=0.01)


class RectifyParams(C.Structure):
    """flx_rectify_params (include/fluctus_hip.h)"""
    _fields_ = [("radius", C.c_int), ("gamma", C.c_float), ("sensitivity", C.c_float), ("lum_floor", C.c_float), ("min_pixels", C.c_int),
                ("plane_tolerance_px", C.c_float), ("normal_cos", C.c_float)]


# the library's defaults (FLX_RC_DEFAULT_*, csrc/flx_rectify.h)
RECTIFY_DEFAULTS = dict(radius=3, gamma=3.0, sensitivity=2.0, lum_floor=0.01, min_pixels=8, plane_tolerance_px=2.0, normal_cos=0.9)


class AdaptiveParams(C.Structure):
    """flx_adaptive_params (include/fluctus_hip.h)"""
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("lum_floor", C.c_float), ("dilate", C.c_uint32)]


# the library's defaults (FLX_AD_DEFAULT_*, csrc/flx_adaptive.h)
ADAPTIVE_DEFAULTS = dict(threshold=0.05, min_samples=4, max_samples=32, lum_floor=0.01, dilate=1)


def _preload_torch_runtime():
    """PyTorch-ROCm bundles its own libamdhip64 / HSA runtime.  If libfluctus_hip.so (linked against /opt/rocm) is loaded
    first and torch later, the process ends up with two HSA runtimes and the first one no longer sees the GPU
    (scripts/order_probe.sh).  Importing torch first makes both share one runtime; without torch nothing is needed."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib_path():
    # FLX_HIP_LIB selects an A/B build of the same library (scripts/build_variants.py); default = the shipped one
    return os.environ.get("FLX_HIP_LIB") or os.path.join(_HERE, "libfluctus_hip.so")


def lib():
    global _lib
    if _lib is None:
        _preload_torch_runtime()
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing -- the HIP extension is required (no fallback); run __graft_entry__.build()")
        L = C.CDLL(path)
        for s in SYMBOLS:
            getattr(L, s)              # raises AttributeError if the library does not export it
        L.flx_last_error.restype = C.c_char_p
        L.flx_last_error.argtypes = [C.c_void_p]
        L.flx_num_tasks.restype = C.c_uint32
        L.flx_local_pixels.restype = C.c_uint32
        L.flx_stream.restype = C.c_void_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class HipContext:
    name = "mi355x"

    def __init__(self, num_tasks, device_index=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.num_tasks = int(num_tasks)
        rc = self.L.flx_create(int(device_index), C.c_uint32(num_tasks), C.byref(self.h))
        if rc != 0:
            raise RuntimeError("flx_create failed: " + self.L.flx_last_error(None).decode())
        self.params = None
        self._cnt = []

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError("libfluctus_hip: " + self.L.flx_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.L.flx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, d):
        self._chk(self.L.flx_upload_scene(self.h, _p(d.tris), C.c_size_t(d.tris.size), _p(d.indices), C.c_size_t(d.indices.size),
                                          _p(d.nodes), C.c_size_t(d.nodes.size), _p(d.materials), C.c_size_t(d.materials.size),
                                          _p(d.texdesc), C.c_size_t(d.texdesc.size), _p(d.texdata), C.c_size_t(d.texdata.size)))

    def update_triangles(self, tris, on_device=False):
        """flx_update_triangles: move the uploaded scene's triangles and refit both traversal trees on the device (topology kept).  tris: a
        SceneData or a wire.TRIANGLE array of the uploaded length; with on_device=True a torch tensor on this device holding the same bytes
        (160 per triangle).  One small blocking read, then asynchronous."""
        if on_device:
            n, rem = divmod(tris.numel() * tris.element_size(), 160)
            assert rem == 0 and tris.is_contiguous(), "a contiguous tensor of 160-byte wire triangles"
            self._chk(self.L.flx_update_triangles(self.h, C.c_void_p(tris.data_ptr()), C.c_size_t(n), 1))
            return
        from . import wire
        t = np.ascontiguousarray(getattr(tris, "tris", tris), wire.TRIANGLE).reshape(-1)
        self._chk(self.L.flx_update_triangles(self.h, _p(t), C.c_size_t(t.size), 0))

    def update_triangles_subset(self, tris, indices, on_device=False):
        """flx_update_triangles_subset: tris[k] replaces triangle indices[k] of the uploaded scene (indices strictly ascending, uint32); only the
        records holding those triangles and the boxes above them are rewritten, everything else keeps its bytes.  tris: a wire.TRIANGLE array
        of len(indices); with on_device=True both are torch tensors on this device (160 bytes per triangle; int32 or uint32 indices).  One
        small blocking read, then asynchronous."""
        if on_device:
            n, rem = divmod(tris.numel() * tris.element_size(), 160)
            assert rem == 0 and tris.is_contiguous() and indices.is_contiguous(), "contiguous tensors of 160-byte wire triangles and 4-byte indices"
            assert indices.element_size() == 4 and indices.numel() == n, "one 4-byte index per triangle"
            self._chk(self.L.flx_update_triangles_subset(self.h, C.c_void_p(tris.data_ptr() if n else None), C.c_void_p(indices.data_ptr() if n else None), C.c_size_t(n), 1))
            return
        from . import wire
        t = np.ascontiguousarray(tris, wire.TRIANGLE).reshape(-1)
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        if t.size != i.size:
            raise ValueError("update_triangles_subset: as many triangles as indices")
        self._chk(self.L.flx_update_triangles_subset(self.h, _p(t), _p(i), C.c_size_t(i.size), 0))

    def objects_define(self, rest_tris, object_of_triangle, nobjects):
        """flx_objects_define (blocking): objects over the uploaded triangles.  rest_tris: a SceneData or a wire.TRIANGLE array of the uploaded
        length, the REST pose; object_of_triangle[i] < nobjects is triangle i's object, NO_OBJECT a triangle that never moves.  Replaces an
        earlier definition; nobjects = 0 drops it (and so does upload_scene).  Changes no byte of any tree."""
        from . import wire
        if not nobjects:
            self._chk(self.L.flx_objects_define(self.h, None, C.c_size_t(0), None, C.c_uint32(0)))
            return
        t = np.ascontiguousarray(getattr(rest_tris, "tris", rest_tris), wire.TRIANGLE).reshape(-1)
        o = np.ascontiguousarray(object_of_triangle, np.uint32).reshape(-1)
        if t.size != o.size:
            raise ValueError("objects_define: one object id per triangle")
        self._chk(self.L.flx_objects_define(self.h, _p(t), C.c_size_t(t.size), _p(o), C.c_uint32(int(nobjects))))

    def objects_pose(self, ids, xforms):
        """flx_objects_pose: xforms[k] (3 x 4, row-major [M | t]) is the ABSOLUTE rest -> world transform of object ids[k] (strictly ascending);
        objects not listed keep their pose.  The triangles are posed on the device from the rest pose kept there (host.pose_triangles is the
        same arithmetic on the CPU) and handed to the subset refit as a device source: update_triangles_subset's boundary, one small blocking
        read, then asynchronous."""
        i = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        x = np.ascontiguousarray(xforms, np.float32).reshape(-1)
        if x.size != 12 * i.size:
            raise ValueError("objects_pose: one 3 x 4 matrix per listed object")
        self._chk(self.L.flx_objects_pose(self.h, _p(i), _p(x), C.c_uint32(i.size)))

    def objects_read(self):
        """test hook (blocking): (counts, members) -- the triangles of each defined object, and the device's ascending list of every object's
        triangles"""
        n = C.c_uint32()
        self._chk(self.L.flx_objects_read(self.h, None, C.byref(n), None))
        counts = np.zeros(n.value, np.uint32)
        self._chk(self.L.flx_objects_read(self.h, _p(counts), C.byref(n), None))
        members = np.zeros(int(counts.sum()), np.uint32)
        self._chk(self.L.flx_objects_read(self.h, _p(counts), C.byref(n), _p(members)))
        return counts, members

    # emissive triangles as lights: set_option("mesh_lights", 1) (include/fluctus_hip.h) for the microkernel integrator, and
    # set_option("mesh_lights_wavefront", 1) on top of it (either order) for the wavefront one: wf_logic then runs the MESH
    # instance of the plain logic pass and the chain is the unfused one whatever "fuse" says.  Inert without "mesh_lights" or without lamps.
    def mesh_lights_read(self):
        """flx_mesh_lights_read (blocking): (tris uint32 ascending, cdf float32, pick float32, total float64) -- the table of emissive triangles
        as it stands on the device; host.mesh_light_table gives the same bytes on the CPU.  All empty when the scene has no light."""
        n, total = C.c_uint32(), C.c_double()
        self._chk(self.L.flx_mesh_lights_read(self.h, C.byref(n), None, None, None, C.byref(total)))
        tri, cdf, pick = np.zeros(n.value, np.uint32), np.zeros(n.value, np.float32), np.zeros(n.value, np.float32)
        self._chk(self.L.flx_mesh_lights_read(self.h, C.byref(n), _p(tri), _p(cdf), _p(pick), C.byref(total)))
        return tri, cdf, pick, float(total.value)

    def mesh_lights_sample(self, r3):
        """test hook (blocking): ml_pick + ml_sample_triangle on the device for (n, 3) float32 triples (pick, r1, r2) ->
        (light (n,) uint32, out8 (n, 8) float32 = P.xyz, pdfA, n_g.xyz, area)"""
        r = np.ascontiguousarray(r3, np.float32).reshape(-1, 3)
        light, out8 = np.zeros(r.shape[0], np.uint32), np.zeros((r.shape[0], 8), np.float32)
        self._chk(self.L.flx_mesh_lights_sample(self.h, _p(r), C.c_uint32(r.shape[0]), _p(light), _p(out8)))
        return light, out8

    TREE_ARRAYS = {0: ("bnodes", 64), 1: ("trirecs", 48), 2: ("shade", 64), 3: ("wnodes", 64), 4: ("wleaf", 16)}

    def tree_read(self, which):
        """test hook: device array `which` of the uploaded scene (0 BNode records, 1 TriRec, 2 ShadeRec, 3 WNode, 4 wide leaf data) as a
        (records, words) uint32 array"""
        need = C.c_size_t()
        self._chk(self.L.flx_tree_read(self.h, int(which), None, C.c_size_t(0), C.byref(need)))
        out = np.zeros(need.value // 4, np.uint32)
        self._chk(self.L.flx_tree_read(self.h, int(which), _p(out), C.c_size_t(out.nbytes), C.byref(need)))
        return out.reshape(-1, self.TREE_ARRAYS[int(which)][1] // 4)

    def tree_cost(self):
        """flx_tree_cost (one small blocking read): the surface-area cost sums of both device trees as they stand now, after a fresh upload or
        any number of update_triangles -- ((A_root, S_node, S_leaf, S_tri) of the binary tree, the same of the 4-wide tree), float64.
        tree_cost_value turns four sums into one figure."""
        out = np.zeros(8, np.float64)
        self._chk(self.L.flx_tree_cost(self.h, _p(out)))
        return tuple(float(v) for v in out[:4]), tuple(float(v) for v in out[4:])

    def upload_envmap(self, e):
        self._chk(self.L.flx_upload_envmap(self.h, _p(e.rgb), e.w, e.h, _p(e.prob), _p(e.alias), _p(e.pdf)))

    def set_params(self, p):
        self.params = p.copy()
        self._chk(self.L.flx_set_params(self.h, _p(np.ascontiguousarray(self.params).reshape(1))))

    def set_partition(self, rank, nranks):
        self._chk(self.L.flx_set_partition(self.h, C.c_uint32(rank), C.c_uint32(nranks)))

    def local_pixels(self):
        return int(self.L.flx_local_pixels(self.h))

    def wf_reset(self): self._chk(self.L.flx_wf_reset(self.h))
    def wf_raygen(self): self._chk(self.L.flx_wf_raygen(self.h))
    def wf_extend(self): self._chk(self.L.flx_wf_extend(self.h))
    def wf_shadow(self): self._chk(self.L.flx_wf_shadow(self.h))
    def wf_logic(self, first=False): self._chk(self.L.flx_wf_logic(self.h, int(bool(first))))
    def wf_materials(self): self._chk(self.L.flx_wf_materials(self.h))
    def postprocess(self): self._chk(self.L.flx_postprocess(self.h))
    def clear_queues(self): self._chk(self.L.flx_clear_queues(self.h))
    # microkernel integrator
    def mk_reset(self): self._chk(self.L.flx_mk_reset(self.h))
    def mk_raygen(self): self._chk(self.L.flx_mk_raygen(self.h))
    def mk_next_vertex(self): self._chk(self.L.flx_mk_next_vertex(self.h))
    def mk_sample_bsdf(self): self._chk(self.L.flx_mk_sample_bsdf(self.h))
    def mk_splat(self): self._chk(self.L.flx_mk_splat(self.h))
    def mk_splat_preview(self): self._chk(self.L.flx_mk_splat_preview(self.h))

    def mk_adaptive_update(self, **params):
        """flx_mk_adaptive_update (blocking; option "moments"): threshold, min_samples, max_samples, lum_floor, dilate -- any left out takes its
        default (ADAPTIVE_DEFAULTS).  Classifies the pixels, installs the ascending list of active ones for the following mk_raygen ... mk_splat
        and returns its length."""
        unknown = set(params) - set(ADAPTIVE_DEFAULTS)
        if unknown:
            raise TypeError(f"mk_adaptive_update: unknown parameters {sorted(unknown)}")
        v = dict(ADAPTIVE_DEFAULTS, **params)
        ap = AdaptiveParams(float(v["threshold"]), int(v["min_samples"]), int(v["max_samples"]), float(v["lum_floor"]), int(v["dilate"]))
        n = C.c_uint32()
        self._chk(self.L.flx_mk_adaptive_update(self.h, C.byref(ap) if params else None, C.byref(n)))
        return int(n.value)

    def mk_adaptive_clear(self): self._chk(self.L.flx_mk_adaptive_clear(self.h))

    def mk_active_read(self):
        """test hook: (list, flags) -- the installed ascending list of active pixels (uint32) and the flag byte of every pixel as the last update
        left it (bit 0 own, 1 active, 2 done, 3 converged)"""
        npix = int(self.params["width"]) * int(self.params["height"])
        lst, flags, n = np.zeros(npix, np.uint32), np.zeros(npix, np.uint8), C.c_uint32()
        self._chk(self.L.flx_mk_active_read(self.h, _p(lst), C.byref(n), _p(flags)))
        return lst[:n.value].copy(), flags

    def mk_active_write(self, lst):
        """test hook: install an arbitrary list of active pixels (strictly ascending, every entry < width * height)"""
        lst = np.ascontiguousarray(lst, np.uint32).reshape(-1)
        self._chk(self.L.flx_mk_active_write(self.h, _p(lst), C.c_uint32(lst.size)))

    def mk_stats(self, reset=False):
        out = np.zeros(4, np.uint32)
        self._chk(self.L.flx_mk_stats_async(self.h, _p(out)))
        if reset:
            self._chk(self.L.flx_mk_stats_reset(self.h))
        self.finish()
        return out

    def get_counters(self):
        """Asynchronous: the returned array is filled by the next finish()."""
        out = np.zeros(8, np.uint32)
        self._cnt.append(out)           # keep alive until finish
        self._chk(self.L.flx_get_counters_async(self.h, _p(out)))
        return out

    def finish(self):
        self._chk(self.L.flx_finish(self.h))
        self._cnt.clear()

    def set_counters(self, c):
        c = np.ascontiguousarray(c, np.uint32)
        self._chk(self.L.flx_set_counters(self.h, _p(c)))

    def pixel_index_update(self, npix, nnew): self._chk(self.L.flx_pixel_index_update(self.h, C.c_uint32(npix), C.c_uint32(nnew)))
    def pixel_index_reset(self): self._chk(self.L.flx_pixel_index_reset(self.h))

    def end_iteration_async(self): self._chk(self.L.flx_end_iteration_async(self.h))

    def counter_totals(self, reset=False):
        out = np.zeros(8, np.uint64)
        self._chk(self.L.flx_counter_totals(self.h, _p(out), int(reset)))
        return out

    def read_pixels(self, which=0):
        out = np.zeros((self.local_pixels(), 4), np.float32)
        self._chk(self.L.flx_read_pixels(self.h, which, _p(out)))
        return out

    def write_pixels(self, which, arr):
        """which = 0 raw accumulation, 4 / 5 albedo / normal accumulators, 7 luminance moments (option "moments"): (local pixels, 4) float32,
        blocking"""
        arr = np.ascontiguousarray(arr, np.float32).reshape(-1, 4)
        assert arr.shape[0] == self.local_pixels(), (arr.shape, self.local_pixels())
        self._chk(self.L.flx_write_pixels(self.h, int(which), _p(arr)))

    def denoise(self, **params):
        """flx_denoise (asynchronous): iterations, sigma_color, sigma_normal, sigma_albedo, blend; missing ones take the defaults.
        No keyword at all passes NULL (the library's defaults).  Result: read_pixels(6) and the preview read_pixels(1)."""
        unknown = set(params) - set(DENOISE_DEFAULTS)
        if unknown:
            raise TypeError(f"denoise: unknown parameters {sorted(unknown)}")
        if not params:
            self._chk(self.L.flx_denoise(self.h, None))
            return
        P = dict(DENOISE_DEFAULTS, **params)
        dp = DenoiseParams(int(P["iterations"]), float(P["sigma_color"]), float(P["sigma_normal"]), float(P["sigma_albedo"]), float(P["blend"]))
        self._chk(self.L.flx_denoise(self.h, C.byref(dp)))

    def denoise_variance_guided(self, **params):
        """flx_denoise_variance_guided (asynchronous; options "denoiser" and "moments"): iterations, sigma_luminance, sigma_normal, sigma_albedo,
        blend; missing ones take the defaults, no keyword at all passes NULL.  Result: read_pixels(6) and the preview read_pixels(1)."""
        unknown = set(params) - set(DENOISE_VG_DEFAULTS)
        if unknown:
            raise TypeError(f"denoise_variance_guided: unknown parameters {sorted(unknown)}")
        if not params:
            self._chk(self.L.flx_denoise_variance_guided(self.h, None))
            return
        P = dict(DENOISE_VG_DEFAULTS, **params)
        dp = DenoiseVgParams(int(P["iterations"]), float(P["sigma_luminance"]), float(P["sigma_normal"]), float(P["sigma_albedo"]), float(P["blend"]))
        self._chk(self.L.flx_denoise_variance_guided(self.h, C.byref(dp)))

    # temporal reprojection (include/fluctus_hip.h)
    def gbuffer(self):
        """flx_gbuffer (asynchronous): the primary-visibility G-buffer of the current camera into the current slot"""
        self._chk(self.L.flx_gbuffer(self.h))

    def history_capture(self):
        """flx_history_capture: copies of which = 0 (and 7); the current G-buffer slot becomes the previous one"""
        self._chk(self.L.flx_history_capture(self.h))

    def reproject(self, **params):
        """flx_reproject (asynchronous): max_history, plane_tolerance_px, normal_cos, min_weight; missing ones take the defaults, no keyword at
        all passes NULL.  Overwrites which = 0 (and 7) with the captured history resampled into the current view."""
        unknown = set(params) - set(REPROJECT_DEFAULTS)
        if unknown:
            raise TypeError(f"reproject: unknown parameters {sorted(unknown)}")
        if not params:
            self._chk(self.L.flx_reproject(self.h, None))
            return
        P = dict(REPROJECT_DEFAULTS, **params)
        rp = ReprojectParams(float(P["max_history"]), float(P["plane_tolerance_px"]), float(P["normal_cos"]), float(P["min_weight"]))
        self._chk(self.L.flx_reproject(self.h, C.byref(rp)))

    # history rectification (include/fluctus_hip.h)
    def history_mark(self):
        """flx_history_mark (asynchronous): copies of which = 0 (and 7) as the mark the next history_rectify compares the new samples with"""
        self._chk(self.L.flx_history_mark(self.h))

    def history_rectify(self, **params):
        """flx_history_rectify (asynchronous): radius, gamma, sensitivity, lum_floor, min_pixels, plane_tolerance_px, normal_cos; missing ones take
        the defaults, no keyword at all passes NULL.  Takes the share of the marked history the samples since the mark contradict out of
        which = 0 (and 7) and out of the mark."""
        unknown = set(params) - set(RECTIFY_DEFAULTS)
        if unknown:
            raise TypeError(f"history_rectify: unknown parameters {sorted(unknown)}")
        if not params:
            self._chk(self.L.flx_history_rectify(self.h, None))
            return
        P = dict(RECTIFY_DEFAULTS, **params)
        rp = RectifyParams(int(P["radius"]), float(P["gamma"]), float(P["sensitivity"]), float(P["lum_floor"]), int(P["min_pixels"]),
                           float(P["plane_tolerance_px"]), float(P["normal_cos"]))
        self._chk(self.L.flx_history_rectify(self.h, C.byref(rp)))

    def history_mark_read(self, moments=False):
        """test hook (blocking) -> (mark (pixels, 4), mark moments (pixels, 4) or None, lambda (pixels,)) of the last history_rectify since the
        mark (zeros before one)"""
        n = self.local_pixels()
        mark, lam = np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
        mom = np.zeros((n, 4), np.float32) if moments else None
        self._chk(self.L.flx_history_mark_read(self.h, _p(mark), _p(mom), _p(lam)))
        return mark, mom, lam

    def gbuffer_read(self, slot=0):
        """test hook -> ((pixels, 8) float32: G0 = (P, hit index bits), G1 = (Ng, t); the slot's camera as a wire.CAMERA record)"""
        from . import wire
        out = np.zeros((self.local_pixels(), 8), np.float32)
        cam = np.zeros(1, wire.CAMERA)
        self._chk(self.L.flx_gbuffer_read(self.h, int(slot), _p(out), _p(cam)))
        return out, cam.reshape(())

    def gbuffer_write(self, slot, g, camera):
        """test hook: (pixels, 8) float32 and a wire.CAMERA record into slot 0 (current) or 1 (previous)"""
        from . import wire
        g = np.ascontiguousarray(g, np.float32).reshape(-1, 8)
        assert g.shape[0] == self.local_pixels(), (g.shape, self.local_pixels())
        cam = np.frombuffer(np.asarray(camera).tobytes(), wire.CAMERA).copy()      # any 80-byte flx_camera record
        assert cam.size == 1
        self._chk(self.L.flx_gbuffer_write(self.h, int(slot), _p(g), _p(cam)))

    # ... across a pose of objects: set_option("motion_history", 1) (include/fluctus_hip.h)
    def gbuffer_objects_read(self, slot=0):
        """test hook: (pixels,) uint32, the object id of every pixel of the slot's G-buffer (NO_OBJECT: a miss, the area light, no object)"""
        out = np.empty(self.local_pixels(), np.uint32)
        self._chk(self.L.flx_gbuffer_objects_read(self.h, int(slot), _p(out)))
        return out

    def gbuffer_objects_write(self, slot, objects):
        """test hook: one uint32 per pixel into the object plane of slot 0 (current) or 1 (previous); after gbuffer_write, which fills it with NO_OBJECT"""
        o = np.ascontiguousarray(objects, np.uint32).reshape(-1)
        assert o.size == self.local_pixels(), (o.size, self.local_pixels())
        self._chk(self.L.flx_gbuffer_objects_write(self.h, int(slot), _p(o)))

    # ... across a per-triangle move: set_option("deform_history", 1) (include/fluctus_hip.h)
    def gbuffer_bary_read(self, slot=0):
        """test hook: (pixels, 2) float32, the barycentrics (u, v) of every pixel of the slot's G-buffer ((-1, -1): a miss, the area light)"""
        out = np.empty((self.local_pixels(), 2), np.float32)
        self._chk(self.L.flx_gbuffer_bary_read(self.h, int(slot), _p(out)))
        return out

    def gbuffer_bary_write(self, slot, bary):
        """test hook: two float32 per pixel into the barycentric plane of slot 0 (current) or 1 (previous); after gbuffer_write, which fills it with (-1, -1)"""
        b = np.ascontiguousarray(bary, np.float32).reshape(-1, 2)
        assert b.shape[0] == self.local_pixels(), (b.shape, self.local_pixels())
        self._chk(self.L.flx_gbuffer_bary_write(self.h, int(slot), _p(b)))

    def deform_read(self, ntris):
        """test hook (blocking) -> ((ntris, 3, 3) float32: every triangle's positions as the first move after the last capture found them,
        (ntris,) bool: its positions now differ from them bitwise).  ntris: the uploaded scene's triangle count.  Fails without a snapshot."""
        pos, moved = np.empty((int(ntris), 3, 3), np.float32), np.empty(int(ntris), np.uint8)
        self._chk(self.L.flx_deform_read(self.h, _p(pos), _p(moved)))
        return pos, moved.astype(bool)

    def kernel_profile(self, kernel):
        """(milliseconds, launches) of one FLX_K_* id accumulated while profiling (level 1) since the last profile_reset; after finish()"""
        ms, n = C.c_double(), C.c_uint64()
        self._chk(self.L.flx_profile_get(self.h, int(kernel), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def denoise_profile(self):
        """(milliseconds, launches) of flx_denoise accumulated while profiling (level 1) since the last profile_reset; after finish()"""
        ms, n = C.c_double(), C.c_uint64()
        self._chk(self.L.flx_profile_get(self.h, K_DENOISE, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # multi-GPU group (RCCL); see include/fluctus_hip.h
    def group_init(self, rank, nranks, unique_id):
        """One process per GPU: ncclCommInitRank + the pixel partition.  unique_id: the 128 bytes of group_unique_id() made on rank 0."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.L.flx_group_init(self.h, C.c_uint32(rank), C.c_uint32(nranks), buf))

    def group_info(self):
        """(ncclCommCount, ncclCommUserRank) as the communicator itself reports them."""
        out = (C.c_uint32 * 2)()
        self._chk(self.L.flx_group_info(self.h, out))
        return int(out[0]), int(out[1])

    def gather(self, root=0):
        """Collective over the group: returns the full (width*height, 4) accumulation image on `root`, None elsewhere."""
        npix = int(self.params["width"]) * int(self.params["height"])
        out = np.zeros((npix, 4), np.float32)
        self._chk(self.L.flx_gather(self.h, C.c_uint32(root), _p(out)))
        return out

    def copy_pixels_to_device(self, ptr):
        self._chk(self.L.flx_copy_pixels_to_device(self.h, C.c_void_p(ptr)))

    def state_export(self):
        out = np.zeros((64, self.num_tasks), np.float32)
        self._chk(self.L.flx_state_export(self.h, _p(out)))
        return out

    def env_sample_table(self, w, h):
        """(w * h, 8) float32: the per-texel light-sample table built at upload_envmap (test hook)."""
        out = np.zeros((int(w) * int(h), 8), np.float32)
        self._chk(self.L.flx_env_sample_table(self.h, _p(out)))
        return out

    def math_probe(self, fn, a, b):
        """include/flx_math.h function `fn` over operand arrays on the device; bit patterns (test hook)."""
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        out = np.zeros(a.size, np.uint32)
        self._chk(self.L.flx_math_probe(self.h, int(fn), _p(a), _p(b), C.c_uint32(a.size), _p(out)))
        return out

    def state_import(self, st):
        st = np.ascontiguousarray(st, np.float32)
        assert st.shape == (64, self.num_tasks)
        self._chk(self.L.flx_state_import(self.h, _p(st)))

    def queue_read(self, q):
        out = np.zeros(self.num_tasks, np.uint32)
        self._chk(self.L.flx_queue_read(self.h, q, _p(out)))
        return out

    def queue_write(self, q, arr):
        arr = np.ascontiguousarray(arr, np.uint32)
        self._chk(self.L.flx_queue_write(self.h, q, _p(arr), C.c_uint32(arr.size)))

    # measurement
    def profile_enable(self, on=True): self._chk(self.L.flx_profile_enable(self.h, int(on)))
    def profile_reset(self): self._chk(self.L.flx_profile_reset(self.h))

    def profile_get(self):
        out = {}
        for name, k in KERNELS.items():
            ms, n = C.c_double(), C.c_uint64()
            self._chk(self.L.flx_profile_get(self.h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def trace_stats_enable(self, on=True): self._chk(self.L.flx_trace_stats_enable(self.h, int(on)))
    def reset_stats(self): self._chk(self.L.flx_trace_stats_reset(self.h))

    def stats(self):
        out = np.zeros(7, np.uint64)
        self._chk(self.L.flx_trace_stats_get(self.h, _p(out)))
        return dict(ext_rays=int(out[0]), ext_inner=int(out[1]), ext_tri=int(out[2]), ext_hits=int(out[3]),
                    shadow_inner=int(out[4]), shadow_tri=int(out[5]), shadow_rays=int(out[6]))

    def leaf_stats(self):
        """Leaf visits of the extension / shadow traversal (wide kernels only)."""
        out = np.zeros(24, np.uint64)
        self._chk(self.L.flx_trace_stats_get_all(self.h, _p(out)))
        return dict(ext_leaf=int(out[16]), shadow_leaf=int(out[17]))

    def scene_info(self):
        out = np.zeros(8, np.uint32)
        self._chk(self.L.flx_scene_info(self.h, _p(out)))
        k = ("wide_nodes", "wide_leaf_f4", "wide_stack_bound", "nested", "binary_depth", "spill_levels", "binary_records", "max_leaf")
        return {n: int(v) for n, v in zip(k, out)}

    def wave_stats(self):
        """Wave-level trip counts of the traversal loops (see flx_trace_stats_get_ex)."""
        out = np.zeros(16, np.uint64)
        self._chk(self.L.flx_trace_stats_get_ex(self.h, _p(out)))
        k = ("outer", "inner", "leaf", "tri")
        return dict(ext={n: int(out[8 + i]) for i, n in enumerate(k)}, shadow={n: int(out[12 + i]) for i, n in enumerate(k)}, ext_max_inner_sum=int(out[7]))

    def set_option(self, name, value): self._chk(self.L.flx_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int()
        self._chk(self.L.flx_get_option(self.h, name.encode(), C.byref(v)))
        return v.value


def group_unique_id():
    """ncclGetUniqueId (rank 0 of a multi-process job); ship the bytes to the other ranks and pass them to HipContext.group_init."""
    buf = (C.c_char * 128)()
    if lib().flx_group_unique_id(buf) != 0:
        raise RuntimeError("flx_group_unique_id failed: " + lib().flx_last_error(None).decode())
    return bytes(buf)


def _handles(ctxs):
    return (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])


def group_init_local(ctxs):
    """Single process: contexts 0..n-1 become ranks 0..n-1 of one group (RCCL communicator if on distinct devices)."""
    if lib().flx_group_init_local(_handles(ctxs), C.c_uint32(len(ctxs))) != 0:
        raise RuntimeError("flx_group_init_local: " + lib().flx_last_error(ctxs[0].h).decode())


def gather_local(ctxs, root=0):
    p = ctxs[root].params
    out = np.zeros((int(p["width"]) * int(p["height"]), 4), np.float32)
    if lib().flx_gather_local(_handles(ctxs), C.c_uint32(len(ctxs)), C.c_uint32(root), _p(out)) != 0:
        raise RuntimeError("flx_gather_local: " + lib().flx_last_error(ctxs[root].h).decode())
    return out
