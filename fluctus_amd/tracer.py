"""ctypes binding of the C++ headless Tracer (fluctus_amd/host/tracer.cpp) in libfluctus_host.so."""
import ctypes as C
import numpy as np
from . import host
from .wire import RENDER_PARAMS


class Tracer:
    def __init__(self, width, height, device=0, num_tasks=1 << 20):
        """device: one HIP device index, or a list of them (one process driving several GPUs: devices[0] is the root; the same
        index may repeat -- a 1-GPU stand-in for N ranks)."""
        self.L = host.lib()
        self.h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            devs = (C.c_int * len(device))(*[int(d) for d in device])
            host._chk(self.L.fh_tracer_create_multi(int(width), int(height), devs, len(device), C.c_uint32(num_tasks), C.byref(self.h)))
        else:
            host._chk(self.L.fh_tracer_create(int(width), int(height), int(device), C.c_uint32(num_tasks), C.byref(self.h)))

    @property
    def num_ranks(self):
        return int(self.L.fh_tracer_num_ranks(self.h))

    def read_accumulation(self):
        """Full-resolution accumulation image (rgb sum, sample count), gathered from all ranks."""
        p = self.params
        out = np.zeros((int(p["width"]) * int(p["height"]), 4), np.float32)
        host._chk(self.L.fh_tracer_read_accumulation(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.size)))
        return out

    def close(self):
        if self.h:
            self.L.fh_tracer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init(self, width, height, scene):
        host._chk(self.L.fh_tracer_init(self.h, int(width), int(height), scene.encode()))

    def triangles(self):
        """the scene's wire triangles (a copy)"""
        from .wire import TRIANGLE
        n = C.c_uint64()
        host._chk(self.L.fh_tracer_get_triangles(self.h, None, C.c_uint64(0), C.byref(n)))
        t = np.zeros(n.value, TRIANGLE)
        host._chk(self.L.fh_tracer_get_triangles(self.h, t.ctypes.data_as(C.c_void_p), C.c_uint64(t.size), C.byref(n)))
        return t

    def update_geometry(self, tris):
        """Tracer::updateGeometry: the scene's triangles move (same count, same materials); the host tree and the device trees are refitted, the
        accumulation restarts"""
        from .wire import TRIANGLE
        t = np.ascontiguousarray(tris, TRIANGLE).reshape(-1)
        host._chk(self.L.fh_tracer_update_geometry(self.h, t.ctypes.data_as(C.c_void_p), C.c_uint64(t.size)))

    def update_geometry_subset(self, tris, indices):
        """Tracer::updateGeometry(indices, tris): tris[k] replaces triangle indices[k] of the scene (indices strictly ascending); only the boxes
        above the listed triangles are refitted, on the host tree and on every rank.  The rebuild policy applies as in
        update_geometry."""
        from .wire import TRIANGLE
        t = np.ascontiguousarray(tris, TRIANGLE).reshape(-1)
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        if t.size != i.size:
            raise ValueError("update_geometry_subset: as many triangles as indices")
        host._chk(self.L.fh_tracer_update_geometry_subset(self.h, t.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p), C.c_uint64(i.size)))

    def define_objects(self, object_of_triangle=None, nobjects=None):
        """Tracer::defineObjects: object_of_triangle[i] < nobjects is the object of triangle i, device.NO_OBJECT a triangle that
        never moves; the rest pose is the scene's triangles at this moment.  Without arguments: the objects the OBJ loader found (`o`
        statements, `g` where a file has none).  nobjects = 0 drops the definition.  Returns the number of objects."""
        if object_of_triangle is None:
            n = C.c_uint32()
            host._chk(self.L.fh_tracer_define_scene_objects(self.h, C.byref(n)))
            return int(n.value)
        o = np.ascontiguousarray(object_of_triangle, np.uint32).reshape(-1)
        host._chk(self.L.fh_tracer_define_objects(self.h, host._p(o), C.c_uint64(o.size), C.c_uint32(int(nobjects))))
        return int(nobjects)

    def pose_objects(self, ids, xforms):
        """Tracer::poseObjects: xforms[k] (3 x 4, row-major [M | t]) is the ABSOLUTE rest -> world transform of object ids[k] (strictly
        ascending); objects not listed keep their pose.  Every rank poses the triangles on the device and refits only the boxes above them;
        the host tree and the scene's triangles follow with the same arithmetic.  The rebuild policy applies as in update_geometry."""
        i = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        x = np.ascontiguousarray(xforms, np.float32).reshape(-1)
        if x.size != 12 * i.size:
            raise ValueError("pose_objects: one 3 x 4 matrix per listed object")
        host._chk(self.L.fh_tracer_pose_objects(self.h, host._p(i), host._p(x), C.c_uint32(i.size)))

    REBUILD_MODES = {"off": 0, "blocking": 1, "background": 2}

    def set_rebuild_policy(self, mode, threshold=None):
        """Tracer::setRebuildPolicy: "off" (the default: update_geometry only refits), "blocking" or "background".  Otherwise
        every update_geometry reads the 4-wide tree's surface-area cost after its refit; when cost now / cost right after the last topology
        upload exceeds `threshold` (required, > 1; no default -- DESIGN.md tabulates what a value means) the SBVH is rebuilt for the new
        triangles: inside the call ("blocking"), or on a worker thread while frames go on with refits ("background"; the finished tree is
        uploaded and refitted to the current triangles at the start of the next update_geometry or update)."""
        if mode not in self.REBUILD_MODES:
            raise ValueError(f"set_rebuild_policy: mode must be one of {sorted(self.REBUILD_MODES)}, not {mode!r}")
        if threshold is None:
            if mode != "off":
                raise ValueError("set_rebuild_policy: a threshold is required (there is no default)")
            threshold = 0.0
        host._chk(self.L.fh_tracer_set_rebuild_policy(self.h, self.REBUILD_MODES[mode], C.c_double(float(threshold))))

    def _rebuild_state(self):
        n, pend, ratio = C.c_uint32(), C.c_int(), C.c_double()
        host._chk(self.L.fh_tracer_rebuild_state(self.h, C.byref(n), C.byref(pend), C.byref(ratio)))
        return int(n.value), bool(pend.value), float(ratio.value)

    @property
    def rebuild_count(self):
        """topologies the rebuild policy has uploaded"""
        return self._rebuild_state()[0]

    @property
    def rebuild_pending(self):
        """a background rebuild was started and its tree is not uploaded yet"""
        return self._rebuild_state()[1]

    @property
    def last_cost_ratio(self):
        """cost ratio of the last update_geometry under a policy (1.0 after a blocking rebuild; NaN: none yet)"""
        return self._rebuild_state()[2]

    def wait_for_rebuild(self):
        """joins the background worker; swaps nothing (the next update_geometry / update does)"""
        host._chk(self.L.fh_tracer_wait_for_rebuild(self.h))

    def get_option(self, name, rank=0):
        """test hook: a rank's HipContext.get_option(name)"""
        v = C.c_int()
        host._chk(self.L.fh_tracer_get_option(self.h, C.c_uint32(rank), name.encode(), C.byref(v)))
        return v.value

    def hold_rebuild(self, on):
        """TEST HOOK ONLY (a host has no use for it): while held, a finished background build stays unpublished (rebuild_pending, nothing
        swapped), so a test decides between which two calls a job completes; wait_for_rebuild and close release it"""
        host._chk(self.L.fh_tracer_hold_rebuild(self.h, int(bool(on))))

    def tree_cost(self):
        """the root rank's HipContext.tree_cost: ((A_root, S_node, S_leaf, S_tri) of the binary tree, the same of the 4-wide tree)"""
        out = np.zeros(8, np.float64)
        host._chk(self.L.fh_tracer_tree_cost(self.h, out.ctypes.data_as(C.c_void_p)))
        return tuple(float(v) for v in out[:4]), tuple(float(v) for v in out[4:])

    def tree_read(self, which, rank=0):
        """test hook: a rank's HipContext.tree_read(which) as a (records, words) uint32 array"""
        from .device import HipContext
        need = C.c_uint64()
        host._chk(self.L.fh_tracer_tree_read(self.h, C.c_uint32(rank), int(which), None, C.c_uint64(0), C.byref(need)))
        out = np.zeros(need.value // 4, np.uint32)
        host._chk(self.L.fh_tracer_tree_read(self.h, C.c_uint32(rank), int(which), out.ctypes.data_as(C.c_void_p), C.c_uint64(out.nbytes), C.byref(need)))
        return out.reshape(-1, HipContext.TREE_ARRAYS[int(which)][1] // 4)

    def set_envmap(self, path):
        host._chk(self.L.fh_tracer_set_envmap(self.h, path.encode()))

    @property
    def params(self):
        p = np.zeros(1, RENDER_PARAMS)
        host._chk(self.L.fh_tracer_params(self.h, p.ctypes.data_as(C.c_void_p), None))
        return p.reshape(())

    @params.setter
    def params(self, p):
        a = np.ascontiguousarray(p).reshape(1)
        host._chk(self.L.fh_tracer_params(self.h, None, a.ctypes.data_as(C.c_void_p)))

    def update(self):
        cnt = np.zeros(8, np.uint32)
        host._chk(self.L.fh_tracer_update(self.h, cnt.ctypes.data_as(C.c_void_p)))
        return cnt

    def render_single(self, spp, denoise=False):
        """Tracer::renderSingle (src/tracer.cpp:95-187): exactly spp samples per pixel on the microkernel integrator;
        denoise=True also fills the denoiser feature buffers (read_pixels(2) albedo, read_pixels(3) normals)."""
        host._chk(self.L.fh_tracer_render_single(self.h, int(spp), int(bool(denoise))))

    def render_adaptive(self, min_spp, max_spp, threshold, denoise=False):
        """Tracer::renderAdaptive: render_single to a noise threshold -- min_spp samples everywhere, then only the pixels whose
        relative standard error of the mean luminance is above `threshold` (and their 3 x 3 neighbours) go on, to at most max_spp.  Returns the
        samples taken; read_pixels(0)[:, 3] is the count of every pixel."""
        n = C.c_uint64()
        host._chk(self.L.fh_tracer_render_adaptive(self.h, int(min_spp), int(max_spp), C.c_float(float(threshold)), int(bool(denoise)), C.byref(n)))
        return int(n.value)

    def set_denoiser(self, on):
        host._chk(self.L.fh_tracer_set_denoiser(self.h, int(bool(on))))

    def set_denoiser_strength(self, s):
        """The reference's denoiser strength (blend = 1 - s).  0 (the default) only fills the feature buffers; > 0 makes update() denoise
        the preview at iterations 10, 20, ... and render_single(spp, denoise=True) denoise its final frame (read_pixels(6), read_pixels(1)).
        Single-GPU."""
        host._chk(self.L.fh_tracer_set_denoiser_strength(self.h, C.c_float(float(s))))

    def set_denoiser_mode(self, mode):
        """Tracer::setDenoiserMode: "guided" (the default, flx_denoise) or "variance" (flx_denoise_variance_guided; while the denoiser is on
        the splats also accumulate the luminance moments, read_pixels(7)).  The denoising schedule is the same in both modes."""
        modes = {"guided": 0, "variance": 1}
        if mode not in modes:
            raise ValueError(f"set_denoiser_mode: mode must be one of {sorted(modes)}, not {mode!r}")
        host._chk(self.L.fh_tracer_set_denoiser_mode(self.h, modes[mode]))

    def set_temporal_reprojection(self, on):
        """Tracer::setTemporalReprojection (default off): a camera move on the wavefront integrator keeps the accumulated image by
        reprojecting it into the new view instead of restarting from nothing.  Single-GPU."""
        host._chk(self.L.fh_tracer_set_temporal_reprojection(self.h, int(bool(on))))

    @property
    def temporal_reprojection(self):
        return bool(self.L.fh_tracer_get_temporal_reprojection(self.h))

    def set_motion_reprojection(self, on):
        """Tracer::setMotionReprojection (default off; needs set_temporal_reprojection(True)): pose_objects on the wavefront integrator keeps the
        accumulated image -- a posed object's pixels look their history up where the object was.  Single-GPU."""
        host._chk(self.L.fh_tracer_set_motion_reprojection(self.h, int(bool(on))))

    @property
    def motion_reprojection(self):
        return bool(self.L.fh_tracer_get_motion_reprojection(self.h))

    def set_deform_reprojection(self, on):
        """Tracer::setDeformReprojection (default off; needs set_temporal_reprojection(True), refuses while motion reprojection is on):
        update_geometry in both forms and pose_objects on the wavefront integrator keep the accumulated image -- a moved triangle's pixels look
        their history up where that point of the triangle was.  Single-GPU."""
        host._chk(self.L.fh_tracer_set_deform_reprojection(self.h, int(bool(on))))

    @property
    def deform_reprojection(self):
        return bool(self.L.fh_tracer_get_deform_reprojection(self.h))

    def set_max_history(self, n):
        """Tracer::setMaxHistory: the sample count a reprojected pixel may keep (flx_reproject's max_history, >= 1; default 32)"""
        host._chk(self.L.fh_tracer_set_max_history(self.h, C.c_float(float(n))))

    def set_history_rectification(self, on):
        """Tracer::setHistoryRectification (default off; needs set_temporal_reprojection(True)): a frame that reprojects ends on a mark, and once
        rectify_delay frames have been rendered since, the share of the marked history that the new samples contradict is taken out
        (DESIGN.md 4.3.7).  While on, a moved, resized or re-coloured area light keeps the accumulation the same way.  Single-GPU."""
        host._chk(self.L.fh_tracer_set_history_rectification(self.h, int(bool(on))))

    @property
    def history_rectification(self):
        return bool(self.L.fh_tracer_get_history_rectification(self.h))

    def set_rectify_delay(self, frames):
        """Tracer::setRectifyDelay: frames between the G-buffer of a reprojecting frame and the rectify (>= 1; 0: the default, 2 maxBounces + 2)"""
        host._chk(self.L.fh_tracer_set_rectify_delay(self.h, int(frames)))

    @property
    def rectify_delay(self):
        return int(self.L.fh_tracer_get_rectify_delay(self.h))

    def rectify_info(self, measure=True):
        """-> (the share of the marked sample count the last rectify of update() kept, NaN before one measured; how many rectifies update() has
        run).  measure: from now on every rectify reads the mark before and after (two blocking reads)."""
        share, count = C.c_double(float("nan")), C.c_uint32(0)
        host._chk(self.L.fh_tracer_rectify_info(self.h, int(bool(measure)), C.byref(share), C.byref(count)))
        return share.value, count.value

    def set_option(self, name, value):
        """HipContext::setOption -> flx_set_option (e.g. "extend_tree", 2 for the reference's bit-exact visit order)."""
        host._chk(self.L.fh_tracer_set_option(self.h, name.encode(), int(value)))

    def set_mesh_lights(self, on):
        """Tracer::setMeshLights (default off): the scene's emissive triangles light the microkernel integrator.  While on,
        update() renders with that integrator and toggle_renderer() to the wavefront loop raises.  Single-GPU."""
        host._chk(self.L.fh_tracer_set_mesh_lights(self.h, int(bool(on))))

    def set_mesh_lights_wavefront(self, on):
        """Tracer::setMeshLightsWavefront (default off): the wavefront integrator sees the lamps too, so toggle_renderer() to the
        wavefront loop no longer raises and update() renders them there (the unfused chain: logic, then the separate material kernels).  Raises
        unless set_mesh_lights(True) came first, and on a multi-rank Tracer; set_mesh_lights(False) clears it."""
        host._chk(self.L.fh_tracer_set_mesh_lights_wavefront(self.h, int(bool(on))))

    @property
    def mesh_lights_wavefront(self):
        return bool(self.L.fh_tracer_get_mesh_lights_wavefront(self.h))

    def mesh_light_count(self):
        """Tracer::meshLightCount: the emissive triangles listed as lights on the device (raises while mesh lights are off)"""
        n = C.c_uint32()
        host._chk(self.L.fh_tracer_mesh_light_count(self.h, C.byref(n)))
        return int(n.value)

    def toggle_renderer(self):
        host._chk(self.L.fh_tracer_toggle_renderer(self.h))

    @property
    def uses_wavefront(self):
        return bool(self.L.fh_tracer_uses_wavefront(self.h))

    def stats(self):
        """RenderStats accumulated on the host: primary, extension, shadow rays, samples."""
        out = np.zeros(4, np.uint64)
        host._chk(self.L.fh_tracer_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_cache_dirs(self, hierarchies="", states=""):
        """Directories of the reference-format caches: hierarchy_<hash>.bin (BVH) and state_<hash>.dat (camera/light/sampling state)."""
        self.L.fh_tracer_set_cache_dirs(self.h, hierarchies.encode(), states.encode())

    def save_state(self):
        return self.L.fh_tracer_save_state(self.h) == 0

    def load_state(self):
        return self.L.fh_tracer_load_state(self.h) == 0

    @property
    def scene_hash(self):
        buf = C.create_string_buffer(64)
        host._chk(self.L.fh_tracer_scene_hash(self.h, buf, C.c_uint64(64)))
        return buf.value.decode()

    def run_benchmark(self, seconds=1.0, iterations=0):
        buf = C.create_string_buffer(1 << 20)
        host._chk(self.L.fh_tracer_run_benchmark(self.h, C.c_double(seconds), int(iterations), buf, C.c_uint64(len(buf))))
        return buf.value.decode()

    def read_pixels(self, which=0):
        p = self.params
        out = np.zeros((int(p["width"]) * int(p["height"]), 4), np.float32)
        host._chk(self.L.fh_tracer_read_pixels(self.h, which, out.ctypes.data_as(C.c_void_p), C.c_uint64(out.size)))
        return out

    def save_image(self, path):
        host._chk(self.L.fh_tracer_save_image(self.h, path.encode()))
