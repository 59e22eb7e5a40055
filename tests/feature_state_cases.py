"""Which call invalidates what: event sequences over the context's image-feature state and the flags each must end in.
One table, two executors: tests/test_feature_state.py runs it through csrc/flx_feature_state.h on the CPU (tests/feature_state_cpu.cpp),
tests/test_gpu_feature_state.py through the C ABI on the device.

Every sequence starts from a context with a scene uploaded, a W0 x H0 image, no objects and every option off.  Events:
    ("opt", name, v)         flx_set_option: "motion_history", "moments", "denoiser"
    ("define", n)            flx_objects_define: the scene's first n spheres as objects 0 .. n-1 (n = 0 drops the definition)
    ("pose", {id: pose})     flx_objects_pose; pose "I" (identity) or "T" (a translation)
    ("gbuffer",)  ("capture",)  ("gb_write", slot)  ("obj_write", slot)
    ("upload",)  ("upload_refused",) (null triangles)  ("update",)  ("subset", k) (the first k triangles; 0: an empty list)
    ("resize", W, H)  ("partition",) (flx_set_partition(0, 1))
    ("mk_reset",)  ("adaptive_clear",)  ("adaptive_update",)  ("active_write", n)  ("denoise",)
    ("refused", event, message)   the call must be refused with that message (an argument check on the host) and change nothing but
                                  what the table says a refused call changes
expect = (T0, T1, O0, O1, H, L): slot 0 / 1 holds a G-buffer, slot 0 / 1 holds an object plane, a history is captured, a list of active
pixels is installed.  Optional keys: D (which = 6 holds a denoised image), moved (with H = 1 and the G-buffers in place, flx_reproject
finds a posed object: what known / knownCap and the two poses amount to), and -- on the CPU only, the C ABI does not show them -- Hm
(the captured history has moments) and known / knownCap (one character per object)."""
W0, H0 = 16, 12
MH, MH_OFF, MOMENTS = ("opt", "motion_history", 1), ("opt", "motion_history", 0), ("opt", "moments", 1)
GB, CAP, DEF2, LIST = ("gbuffer",), ("capture",), ("define", 2), ("active_write", 3)


def case(name, events, expect, **more):
    return dict(name=name, events=list(events), expect=tuple(expect), **more)


CASES = [
    case("gbuffer", [GB], (1, 0, 0, 0, 0, 0)),
    case("gbuffer_mh_objects", [MH, DEF2, GB], (1, 0, 1, 0, 0, 0), known="00", knownCap="00"),
    case("gbuffer_mh_no_objects", [MH, GB], (1, 0, 0, 0, 0, 0)),
    case("capture", [GB, CAP], (0, 1, 0, 0, 1, 0), Hm=0, moved=0),
    case("capture_twice_with_moments", [MOMENTS, GB, CAP, GB, CAP], (0, 1, 0, 0, 1, 0), Hm=1, moved=0),
    case("capture_refused_without_gbuffer", [("refused", CAP, "no G-buffer has been traced for the current slot")], (0, 0, 0, 0, 0, 0)),
    case("capture_keeps_the_list", [LIST, GB, CAP], (0, 1, 0, 0, 1, 1)),
    # flx_objects_pose after a capture: kept with the option on and the previous slot's plane valid, dropped otherwise
    case("capture_pose_mh_plane", [MH, DEF2, ("pose", {0: "I"}), GB, CAP, ("pose", {0: "T"})], (0, 1, 0, 1, 1, 0),
         known="10", knownCap="10", moved=1),
    case("capture_pose_mh_same_bytes", [MH, DEF2, ("pose", {0: "T", 1: "I"}), GB, CAP, ("pose", {0: "T"})], (0, 1, 0, 1, 1, 0),
         known="11", knownCap="11", moved=0),
    case("capture_pose_mh_first_pose_drops_list", [MH, DEF2, LIST, GB, CAP, ("pose", {1: "T"})], (0, 1, 0, 1, 1, 0),
         known="01", knownCap="00", moved=1),
    case("capture_pose_mh_no_plane", [MH, DEF2, GB, CAP, MH_OFF, MH, ("pose", {0: "T"})], (0, 0, 0, 0, 0, 0), known="10", knownCap="00"),
    case("capture_pose_mh_off", [DEF2, ("pose", {0: "I"}), GB, CAP, ("pose", {0: "T"})], (0, 0, 0, 0, 0, 0), known="10", knownCap="10"),
    case("capture_pose_empty_list_mh_off", [DEF2, GB, CAP, GB, ("pose", {})], (0, 0, 0, 0, 0, 0), known="00", knownCap="00"),
    case("pose_refused_without_objects", [GB, CAP, GB, LIST, ("refused", ("pose", {0: "T"}), "no objects are defined")], (1, 1, 0, 0, 1, 1)),
    case("pose_capture_update", [MH, DEF2, ("pose", {0: "I", 1: "T"}), GB, CAP, ("update",)], (0, 0, 0, 0, 0, 0),
         known="00", knownCap="11"),
    case("pose_capture_subset", [MH, DEF2, ("pose", {0: "I"}), LIST, GB, CAP, GB, ("subset", 4)], (0, 0, 0, 0, 0, 0),
         known="00", knownCap="10"),
    case("subset_empty_list", [LIST, GB, CAP, GB, ("subset", 0)], (0, 0, 0, 0, 0, 0), Hm=0),
    case("moments_flag_survives_a_drop", [MOMENTS, GB, CAP, ("update",)], (0, 0, 0, 0, 0, 0), Hm=1),
    # a new definition and a new scene: the planes always go, the history only with the option on
    case("define_after_capture_mh", [MH, DEF2, ("pose", {0: "I"}), GB, CAP, DEF2], (0, 0, 0, 0, 0, 0), known="00", knownCap="00"),
    case("define_after_capture_mh_off", [DEF2, ("pose", {0: "I"}), GB, CAP, GB, DEF2], (1, 1, 0, 0, 1, 0),
         known="00", knownCap="00", moved=0),
    case("define_none_after_capture_mh", [MH, DEF2, GB, CAP, ("define", 0)], (0, 0, 0, 0, 0, 0), known="", knownCap=""),
    case("define_none_after_capture_mh_off", [DEF2, GB, CAP, ("define", 0)], (0, 1, 0, 0, 1, 0), known="", knownCap="", moved=0),
    case("upload_after_capture_mh", [MH, DEF2, LIST, GB, CAP, GB, ("upload",)], (0, 0, 0, 0, 0, 0), known="", knownCap=""),
    case("upload_after_capture_mh_off", [DEF2, ("pose", {0: "T"}), LIST, GB, CAP, GB, ("upload",)], (1, 1, 0, 0, 1, 0),
         known="", knownCap="", moved=0),
    case("upload_refused_drops_the_list", [LIST, GB, ("refused", ("upload_refused",), "empty scene")], (1, 0, 0, 0, 0, 0)),
    # the option and the hooks
    case("mh_off_between_gbuffer_and_capture", [MH, DEF2, GB, MH_OFF, CAP], (0, 1, 0, 0, 1, 0), moved=0),
    case("mh_off_and_on_again", [MH, DEF2, GB, CAP, GB, MH_OFF, MH], (1, 1, 0, 0, 1, 0)),
    case("write_slot_1_without_capture", [("gb_write", 1)], (0, 1, 0, 0, 0, 0)),
    case("write_slots_mh", [MH, ("gb_write", 0), ("gb_write", 1)], (1, 1, 1, 1, 0, 0)),
    case("write_slot_mh_off_then_on", [("gb_write", 0), MH, ("refused", ("obj_write", 1), "no G-buffer of the current size"),
                                       ("obj_write", 0)], (1, 0, 1, 0, 0, 0)),
    case("obj_write_refused_mh_off", [GB, ("refused", ("obj_write", 0), "motion_history")], (1, 0, 0, 0, 0, 0)),
    case("plane_travels_with_the_capture", [MH, GB, ("obj_write", 0), CAP, GB], (1, 1, 0, 1, 1, 0)),
    # the list of active pixels and the framebuffers
    case("resize", [LIST, ("opt", "denoiser", 1), ("denoise",), GB, CAP, GB, ("resize", 8, 6)], (0, 0, 0, 0, 0, 0), D=0),
    case("resize_same_pixel_count", [LIST, ("opt", "denoiser", 1), ("denoise",), GB, CAP, GB, ("resize", H0, W0)], (1, 1, 0, 0, 1, 0), D=1),
    case("same_size_again", [LIST, GB, ("resize", W0, H0)], (1, 0, 0, 0, 0, 1)),
    case("partition", [LIST, GB, ("partition",)], (1, 0, 0, 0, 0, 0)),
    case("moments_off", [MOMENTS, ("adaptive_update",), ("opt", "moments", 0)], (0, 0, 0, 0, 0, 0)),
    case("moments_on", [LIST, MOMENTS], (0, 0, 0, 0, 0, 1)),
    case("adaptive_update_refused_without_moments", [("refused", ("adaptive_update",), "needs the luminance moments")], (0, 0, 0, 0, 0, 0)),
    case("adaptive_update", [MOMENTS, GB, ("adaptive_update",)], (1, 0, 0, 0, 0, 1)),
    case("mk_reset", [LIST, GB, ("mk_reset",)], (1, 0, 0, 0, 0, 0)),
    case("adaptive_clear", [LIST, ("adaptive_clear",)], (0, 0, 0, 0, 0, 0)),
    case("update_drops_the_list", [LIST, ("update",)], (0, 0, 0, 0, 0, 0)),
]
assert len({c["name"] for c in CASES}) == len(CASES)


def script(cases=CASES):
    """the table as tests/feature_state_cpu.cpp reads it: `case NAME`, one event per line, `end`"""
    def line(e):
        if e[0] == "refused":
            return "refused " + line(e[1])
        if e[0] == "pose":
            return " ".join(["pose"] + [f"{o}:{p}" for o, p in sorted(e[1].items())])
        return " ".join(str(x) for x in e)
    out = []
    for c in cases:
        out += [f"case {c['name']} {W0} {H0}"] + [line(e) for e in c["events"]] + ["end"]
    return "\n".join(out) + "\n"
