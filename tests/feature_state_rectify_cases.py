"""Which call drops the mark of flx_history_mark: event sequences over the context's image-feature state and the flags
each must end in.  One table, two executors: tests/test_feature_state_rectify.py runs it through csrc/flx_feature_state.h on the CPU
(tests/feature_state_rectify_cpu.cpp), tests/test_gpu_feature_state_rectify.py through the C ABI on the device.

Every sequence starts from a context with a scene uploaded, a W0 x H0 image, no objects and every option off.  Events (the ones of
tests/feature_state_cases.py where the names agree):
    ("opt", name, v)         flx_set_option: "motion_history", "moments"
    ("define", n)  ("pose", {id: pose})  ("gbuffer",)  ("capture",)  ("gb_write", slot)
    ("upload",)  ("update",)  ("subset", k)  ("resize", W, H)  ("partition",)  ("mk_reset",)  ("wf_reset",)
    ("mark",)                flx_history_mark
    ("rectify",)             flx_history_rectify with the defaults;  ("rectify_bad",) with radius 0
    ("write_pixels",)        flx_write_pixels(which = 0)
    ("refused", event, message)   the call must be refused with that message and change nothing
expect = (T0, Mk, MkMom, Live): slot 0 holds a G-buffer, a mark exists, the mark has moments, flx_history_rectify would run."""
W0, H0 = 16, 12
MH, MOMENTS, MOMENTS_OFF = ("opt", "motion_history", 1), ("opt", "moments", 1), ("opt", "moments", 0)
GB, CAP, MARK, RECT, DEF2 = ("gbuffer",), ("capture",), ("mark",), ("rectify",), ("define", 2)


def case(name, events, expect):
    return dict(name=name, events=list(events), expect=tuple(expect))


CASES = [
    case("mark", [GB, MARK], (1, 1, 0, 1)),
    case("mark_with_moments", [MOMENTS, GB, MARK], (1, 1, 1, 1)),
    case("mark_refused_without_gbuffer", [("refused", MARK, "no G-buffer of the current size")], (0, 0, 0, 0)),
    case("mark_refused_after_capture", [GB, CAP, ("refused", MARK, "no G-buffer of the current size")], (0, 0, 0, 0)),
    case("rectify_refused_without_mark", [GB, ("refused", RECT, "no mark")], (1, 0, 0, 0)),
    case("rectify_keeps_the_mark", [GB, MARK, RECT, RECT], (1, 1, 0, 1)),
    case("rectify_refused_keeps_the_mark", [MOMENTS, GB, MARK, ("refused", ("rectify_bad",), "parameters must be")], (1, 1, 1, 1)),
    case("mark_twice_second_without_moments", [MOMENTS, GB, MARK, MOMENTS_OFF, MARK], (1, 1, 0, 1)),
    case("moments_off_keeps_the_marks_moments", [MOMENTS, GB, MARK, MOMENTS_OFF, RECT], (1, 1, 1, 1)),
    # what keeps the mark
    case("write_pixels_keeps", [GB, MARK, ("write_pixels",)], (1, 1, 0, 1)),
    case("gbuffer_again_keeps", [GB, MARK, GB], (1, 1, 0, 1)),
    case("gb_write_keeps", [GB, MARK, ("gb_write", 0), ("gb_write", 1)], (1, 1, 0, 1)),
    case("same_size_again_keeps", [GB, MARK, ("resize", W0, H0)], (1, 1, 0, 1)),
    case("sequence_of_the_header", [GB, CAP, GB, ("mk_reset",), MARK, RECT], (1, 1, 0, 1)),
    # what drops it
    case("mk_reset_drops", [GB, MARK, ("mk_reset",)], (1, 0, 0, 0)),
    case("wf_reset_drops", [MOMENTS, GB, MARK, ("wf_reset",), ("refused", RECT, "no mark")], (1, 0, 0, 0)),
    case("resize_same_pixel_count_drops", [GB, MARK, ("resize", H0, W0)], (1, 0, 0, 0)),
    case("resize_drops_everything", [GB, MARK, ("resize", 8, 6)], (0, 0, 0, 0)),
    case("partition_drops", [GB, MARK, ("partition",)], (1, 0, 0, 0)),
    case("capture_drops", [GB, MARK, CAP], (0, 0, 0, 0)),
    case("capture_then_gbuffer_stays_dropped", [GB, MARK, CAP, GB], (1, 0, 0, 0)),
    case("update_drops", [GB, MARK, ("update",)], (0, 0, 0, 0)),
    case("subset_drops", [GB, MARK, ("subset", 4)], (0, 0, 0, 0)),
    case("subset_empty_list_drops", [GB, MARK, ("subset", 0)], (0, 0, 0, 0)),
    case("pose_drops", [DEF2, GB, MARK, ("pose", {0: "T"})], (0, 0, 0, 0)),
    case("pose_that_keeps_the_history_drops_the_mark", [MH, DEF2, ("pose", {0: "I"}), GB, CAP, GB, MARK, ("pose", {0: "T"})], (0, 0, 0, 0)),
    case("upload_drops", [GB, MARK, ("upload",)], (1, 0, 0, 0)),
    case("dropped_then_marked_again", [MOMENTS, GB, MARK, ("mk_reset",), MOMENTS_OFF, MARK], (1, 1, 0, 1)),
]
assert len({c["name"] for c in CASES}) == len(CASES)


def script(cases=CASES):
    """the table as tests/feature_state_rectify_cpu.cpp reads it: `case NAME W H`, one event per line, `end`"""
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
