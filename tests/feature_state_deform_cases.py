"""Which call invalidates what under option "deform_history" (DESIGN.md 4.3.5, 4.3.6): event sequences over the temporal state and the flags each
must end in.  One table, two executors: tests/test_feature_state_deform.py runs it through csrc/flx_feature_state.h on the CPU
(tests/feature_state_deform_cpu.cpp), tests/test_gpu_reproject_deform.py through the C ABI on the device.  tests/feature_state_cases.py keeps
checking, untouched, that the members that were there before do what they did.

Every sequence starts from a context with a scene uploaded, a W0 x H0 image, no objects and every option off.  Events:
    ("opt", name, v)         flx_set_option: "deform_history", "motion_history"
    ("define", n)            flx_objects_define: the scene's first n spheres as objects 0 .. n-1
    ("pose",)                flx_objects_pose of object 0 by a translation
    ("gbuffer",)  ("capture",)  ("gb_write", slot)  ("bary_write", slot)  ("reproject",)
    ("upload",)  ("update",)  ("subset", k) (the first k triangles)  ("update_nan",) (flx_update_triangles with a NaN vertex: always refused)
    ("resize", W, H)
    ("refused", event, message)   the call must be refused with that message and change nothing
expect = (T0, T1, B0, B1, H, S): slot 0 / 1 holds a G-buffer, slot 0 / 1 holds a barycentric plane, a history is captured, a snapshot of the
positions at that capture exists (flx_reproject follows the moves).  Optional key, CPU only: snapshots, how many times a move had to copy the
positions aside."""
W0, H0 = 16, 12
DH, DH_OFF, MH = ("opt", "deform_history", 1), ("opt", "deform_history", 0), ("opt", "motion_history", 1)
GB, CAP, UPD, RP = ("gbuffer",), ("capture",), ("update",), ("reproject",)


def case(name, events, expect, **more):
    return dict(name=name, events=list(events), expect=tuple(expect), **more)


CASES = [
    case("gbuffer_writes_the_plane", [DH, GB], (1, 0, 1, 0, 0, 0)),
    case("gbuffer_option_off", [GB], (1, 0, 0, 0, 0, 0)),
    case("capture_carries_the_plane", [DH, GB, CAP], (0, 1, 0, 1, 1, 0), snapshots=0),
    # a move under the option, with a history and the previous slot's plane: snapshot, only the current slot goes
    case("move_keeps_the_history", [DH, GB, CAP, UPD], (0, 1, 0, 1, 1, 1), snapshots=1),
    case("move_with_a_current_slot", [DH, GB, CAP, GB, ("subset", 4)], (0, 1, 0, 1, 1, 1), snapshots=1),
    case("two_moves_after_one_capture", [DH, GB, CAP, UPD, ("subset", 4)], (0, 1, 0, 1, 1, 1), snapshots=1),
    case("pose_is_a_move", [DH, ("define", 2), GB, CAP, ("pose",)], (0, 1, 0, 1, 1, 1), snapshots=1),
    case("move_gbuffer_reproject", [DH, GB, CAP, UPD, GB, RP], (1, 1, 1, 1, 1, 1), snapshots=1),
    case("reproject_refused_without_current_gbuffer", [DH, GB, CAP, UPD, ("refused", RP, "no G-buffer has been traced for the current camera")],
         (0, 1, 0, 1, 1, 1)),
    case("capture_clears_the_snapshot", [DH, GB, CAP, UPD, GB, CAP], (0, 1, 0, 1, 1, 0), snapshots=1),
    case("each_capture_its_own_snapshot", [DH, GB, CAP, UPD, UPD, GB, CAP, UPD], (0, 1, 0, 1, 1, 1), snapshots=2),
    case("refused_move", [DH, GB, CAP, GB, ("refused", ("update_nan",), "NaN or infinite")], (1, 1, 1, 1, 1, 0), snapshots=0),
    case("refused_move_after_a_move", [DH, GB, CAP, UPD, GB, ("refused", ("update_nan",), "NaN or infinite")], (1, 1, 1, 1, 1, 1), snapshots=1),
    # any other move does what it does without the option
    case("move_option_off", [GB, CAP, GB, UPD], (0, 0, 0, 0, 0, 0), snapshots=0),
    case("move_without_a_previous_plane", [GB, CAP, DH, GB, UPD], (0, 0, 0, 0, 0, 0), snapshots=0),
    case("move_without_a_history", [DH, GB, UPD], (0, 0, 0, 0, 0, 0), snapshots=0),
    case("pose_option_off", [("define", 2), GB, CAP, ("pose",)], (0, 0, 0, 0, 0, 0), snapshots=0),
    # the two options
    case("motion_refused_under_deform", [DH, ("refused", MH, "deform_history"), GB], (1, 0, 1, 0, 0, 0)),
    case("deform_refused_under_motion", [MH, ("refused", DH, "motion_history"), GB], (1, 0, 0, 0, 0, 0)),
    case("off_with_a_snapshot_drops_the_history", [DH, GB, CAP, UPD, GB, DH_OFF], (0, 0, 0, 0, 0, 0)),
    case("off_without_a_snapshot_keeps_it", [DH, GB, CAP, GB, DH_OFF], (1, 1, 0, 0, 1, 0)),
    case("off_and_on_again_then_a_move", [DH, GB, CAP, DH_OFF, DH, UPD], (0, 0, 0, 0, 0, 0), snapshots=0),
    # a new scene, a new definition, a new size
    case("upload_drops_the_history", [DH, GB, CAP, GB, ("upload",)], (0, 0, 0, 0, 0, 0)),
    case("upload_after_a_move", [DH, GB, CAP, UPD, ("upload",)], (0, 0, 0, 0, 0, 0)),
    case("upload_option_off_keeps_it", [GB, CAP, GB, ("upload",)], (1, 1, 0, 0, 1, 0)),
    case("define_keeps_it", [DH, GB, CAP, GB, ("define", 2)], (1, 1, 1, 1, 1, 0)),
    case("resize_after_a_move", [DH, GB, CAP, UPD, ("resize", 8, 6)], (0, 0, 0, 0, 0, 0)),
    # the hooks
    case("write_slots", [DH, ("gb_write", 0), ("gb_write", 1)], (1, 1, 1, 1, 0, 0)),
    case("write_slot_option_off_then_on", [("gb_write", 0), DH, ("refused", ("bary_write", 1), "no G-buffer of the current size"), ("bary_write", 0)],
         (1, 0, 1, 0, 0, 0)),
    case("bary_write_refused_option_off", [GB, ("refused", ("bary_write", 0), "deform_history")], (1, 0, 0, 0, 0, 0)),
    case("plane_travels_with_the_capture", [DH, ("gb_write", 0), ("bary_write", 0), CAP, GB], (1, 1, 1, 1, 1, 0)),
]
assert len({c["name"] for c in CASES}) == len(CASES)


def script(cases=CASES):
    """the table as tests/feature_state_deform_cpu.cpp reads it: `case NAME W H`, one event per line, `end`"""
    def line(e):
        return "refused " + line(e[1]) if e[0] == "refused" else " ".join(str(x) for x in e)
    out = []
    for c in cases:
        out += [f"case {c['name']} {W0} {H0}"] + [line(e) for e in c["events"]] + ["end"]
    return "\n".join(out) + "\n"
