"""What each public Tracer call does to the history: event sequences over host/history_state.hpp and what every frame and
every move of triangles must then decide.  tests/test_tracer_history.py runs the table through the header on the CPU
(tests/tracer_history_cpu.cpp); the Tracer tests of tests/test_gpu_reproject*.py and tests/test_gpu_rectify.py see the same decisions on the device.

THE EXPECTED COLUMN WAS READ OFF Tracer's code as it stood BEFORE the state moved into the header (thirteen loose members, written in place by
init, the moves, the switches, update ...), statement by statement -- never produced by running the header.

Every sequence starts from a Tracer after its constructor: the wavefront integrator, every switch off, parameters pending, iteration 0, a 32 x 24
image, maxBounces 4 (so the default rectify delay is 10), the area light on.  Events, one per public call:
    ("frame", n)                     n x update()
    ("temporal" | "motion" | "deform" | "rectify", 0 | 1)      the four switches      ("delay", n)    setRectifyDelay
    ("params", "camera" | "exposure" | "light" | "bounces", n | "size", W, H)         getParams() changed + paramsChanged()
    ("update_geometry", how)  ("pose", how)      how "": accepted; "refused": the device throws; "reupload": a Blocking rebuild inside the call
    ("adopt_rebuild",)               a finished background rebuild is adopted
    ("define",)  ("envmap",)  ("toggle",)  ("mesh_lights",)  ("mesh_lights_wavefront",)  ("render_single", spp)  ("render_adaptive", spp)
    ("benchmark", n)  ("init",)      ("restart",) setDenoiser / setDenoiserMode: iteration = 0 and nothing else
    ("dropped",)                     not a call: HistoryState::dropped() with init()'s two other lines, what init is measured against
trace: one token per frame -- the device calls in order, c flx_history_capture, g flx_gbuffer, r flx_reproject, m flx_history_mark,
R flx_history_rectify, "." none, "mk" the microkernel branch, then @ and the frame number the denoiser's schedule sees -- and one per move:
"mv:" k the history is kept, c this call captured it, "." neither.
flags (optional): "have captured mark framesSinceGbuffer temporalFrames iteration pending switches delay history" at the end; switches are four
digits temporal motion deform rectify, delay is getRectifyDelay(), history is historyExists(params, integrator, posed = false)."""


def idle(a, b):
    """frames a .. b of the schedule in which nothing but the render happens"""
    return " ".join(f".@{k}" for k in range(a, b + 1))


def mk(a, b):
    return " ".join(f"mk@{k}" for k in range(a, b + 1))


T, M, D, RC = ("temporal", 1), ("motion", 1), ("deform", 1), ("rectify", 1)
F3, F = ("frame", 3), ("frame", 1)
CAM, LIGHT, EXPOSURE = ("params", "camera"), ("params", "light"), ("params", "exposure")
GEOM, POSE = ("update_geometry", ""), ("pose", "")
PRE = "g@0 .@1 .@2"                  # temporal reprojection on, three frames: a G-buffer on the first and nothing since
MARKED = [T, RC, F3, CAM, F]         # ... rectification on, a camera move: the frame reprojected and ended on a mark
MARKED_TRACE = PRE + " cgrm@3"


def case(name, events, trace, flags=None):
    return dict(name=name, events=list(events), trace=trace, flags=flags)


CASES = [
    # 1. every switch off: no capture, no G-buffer, no reprojection; the denoiser counts iterations
    case("all_off", [F3, CAM, ("frame", 2)], ".@0 .@1 .@2 .@0 .@1", "0 0 0 5 2 2 0 0000 10 0"),
    # 2. temporal reprojection: the first frame traces only; a camera-only change captures, traces, reprojects, and the schedule goes on
    case("temporal_first_frames", [T, F3], PRE, "1 0 0 3 3 3 0 1000 10 1"),
    case("temporal_camera", [T, F3, CAM, F], PRE + " cgr@3", "1 0 0 1 4 1 0 1000 10 1"),
    case("temporal_exposure", [T, F3, EXPOSURE, F], PRE + " cgr@3", "1 0 0 1 4 1 0 1000 10 1"),
    case("temporal_camera_every_frame",[T, F, CAM, F, CAM, F], "g@0 cgr@1 cgr@2"),
    # 3. ... and maxBounces with it: nothing kept, the schedule restarts
    case("temporal_camera_and_bounces", [T, F3, CAM, ("params", "bounces", 5), F], PRE + " g@0", "1 0 0 1 1 1 0 1000 12 1"),
    # 4. the area light alone: as 3 without rectification, as 2 with it, plus the mark
    case("temporal_light", [T, F3, LIGHT, F], PRE + " g@0", "1 0 0 1 1 1 0 1000 10 1"),
    case("rectify_light", [T, RC, F3, LIGHT, F], PRE + " cgrm@3", "1 0 1 1 4 1 0 1001 10 1"),
    case("rectify_camera", MARKED, MARKED_TRACE, "1 0 1 1 4 1 0 1001 10 1"),
    case("rectify_does_not_excuse_the_bounces", [T, RC, F3, LIGHT, ("params", "bounces", 5), F], PRE + " g@0"),
    # 5. another size since the G-buffer: no history
    case("size_changed", [T, F3, ("params", "size", 40, 30), F], PRE + " g@0", "1 0 0 1 1 1 0 1000 10 1"),
    case("size_exchanged", [T, F3, ("params", "size", 24, 32), F], PRE + " g@0"),
    # 6. a frame on the microkernel integrator consumes the update without a G-buffer and counts only its iteration
    case("microkernel_frame", [T, F3, ("toggle",), CAM, F], PRE + " mk@0", "0 0 0 3 0 1 0 1000 10 0"),
    case("microkernel_frame_then_wavefront", [T, F3, ("toggle",), CAM, F, ("toggle",), F, CAM, F], PRE + " mk@0 .@0 g@0", "1 0 0 1 1 1 0 1000 10 1"),
    # 7. a move under its switch: kept, captured once per frame; the next frame does not capture again, traces and reprojects
    case("move_captures", [T, D, F3, GEOM], PRE + " mv:kc", "1 1 0 3 3 0 1 1010 10 0"),        # (history 0: worldRadius moved, and posed = false)
    case("two_moves_one_capture", [T, D, F3, GEOM, GEOM, F, CAM, F], PRE + " mv:kc mv:k gr@3 cgr@4", "1 0 0 1 5 1 0 1010 10 1"),
    case("moves_and_camera_in_one_frame", [T, D, F3, GEOM, ("update_geometry", ""), CAM, F], PRE + " mv:kc mv:k gr@3"),
    case("camera_then_move_in_one_frame", [T, D, F3, CAM, GEOM, F], PRE + " mv:kc gr@3"),
    case("pose_under_motion", [T, M, F3, POSE, F], PRE + " mv:kc gr@3", "1 0 0 1 4 1 0 1100 10 1"),
    case("pose_under_deform", [T, D, F3, POSE, GEOM, F], PRE + " mv:kc mv:k gr@3", "1 0 0 1 4 1 0 1010 10 1"),
    case("move_under_rectify_marks", [T, D, RC, F3, GEOM, F], PRE + " mv:kc grm@3", "1 0 1 1 4 1 0 1011 10 1"),
    # 8. ... with the topology re-uploaded inside the move: the history is gone
    case("move_reuploads", [T, D, F3, ("update_geometry", "reupload"), F], PRE + " mv:kc g@0", "1 0 0 1 1 1 0 1010 10 1"),
    case("pose_reuploads", [T, M, F3, ("pose", "reupload"), F], PRE + " mv:kc g@0"),
    # 9. a move refused after its capture: the next frame traces the handed-over slot again and reprojects, without a second capture
    case("move_refused_after_capture", [T, D, F3, ("update_geometry", "refused")], PRE + " mv:kc", "1 1 0 3 3 3 1 1010 10 1"),
    case("move_refused_then_frame", [T, D, F3, ("update_geometry", "refused"), F], PRE + " mv:kc gr@3", "1 0 0 1 4 1 0 1010 10 1"),
    case("second_move_refused", [T, D, F3, GEOM, ("update_geometry", "refused"), F], PRE + " mv:kc mv:k gr@3"),
    case("pose_refused_after_capture", [T, M, F3, ("pose", "refused"), F], PRE + " mv:kc gr@3"),
    case("move_refused_without_switch", [T, F3, ("update_geometry", "refused"), F], PRE + " mv:. .@3", "1 0 0 4 4 4 0 1000 10 1"),
    # 10. a move without its switch keeps nothing
    case("pose_without_switch", [T, F3, POSE, F], PRE + " mv:. g@0", "1 0 0 1 1 1 0 1000 10 1"),
    case("update_geometry_under_motion", [T, M, F3, GEOM, F], PRE + " mv:. g@0", "1 0 0 1 1 1 0 1100 10 1"),
    case("move_on_microkernel", [T, D, F3, ("toggle",), GEOM, F], PRE + " mv:. mk@0", "0 0 0 3 0 1 0 1010 10 0"),
    case("move_before_any_frame", [T, D, GEOM, F], "mv:. g@0"),
    # 11. calls that drop the history: the next frame traces only
    case("define_under_motion", [T, M, F3, ("define",), CAM, F], PRE + " g@0", "1 0 0 1 1 1 0 1100 10 1"),
    case("define_without_motion", [T, F3, ("define",), CAM, F], PRE + " cgr@3"),
    case("define_under_deform", [T, D, F3, ("define",), CAM, F], PRE + " cgr@3"),
    case("envmap", [T, F3, ("envmap",), F], PRE + " g@0"),
    case("toggle_twice", [T, F3, ("toggle",), ("toggle",), CAM, F], PRE + " g@0"),
    case("mesh_lights", [T, F3, ("mesh_lights",), CAM, F], PRE + " g@0"),
    case("mesh_lights_wavefront", [T, F3, ("mesh_lights_wavefront",), CAM, F], PRE + " g@0"),
    case("render_single", [T, F3, ("render_single", 4), ("toggle",), CAM, F], PRE + " g@0", "1 0 0 1 1 1 0 1000 10 1"),
    case("render_adaptive", [T, F3, ("render_adaptive", 4), ("toggle",), CAM, F], PRE + " g@0"),
    case("benchmark", [T, F3, ("benchmark", 5), CAM, F], PRE + " g@0"),
    case("adopt_rebuild", [T, D, F3, ("adopt_rebuild",), F], PRE + " g@0"),
    case("temporal_set_again", [T, F3, T, CAM, F], PRE + " g@0", "1 0 0 1 1 1 0 1000 10 1"),
    case("temporal_set_again_restarts_the_schedule", [T, F3, T, F], PRE + " .@0", "0 0 0 4 1 4 0 1000 10 0"),      # (nothing pending: no G-buffer)
    case("temporal_on_restarts_the_schedule", [F3, T, F], ".@0 .@1 .@2 .@0", "0 0 0 4 1 4 0 1000 10 0"),
    case("temporal_off", [T, F3, ("temporal", 0), CAM, F], PRE + " .@0", "0 0 0 4 1 1 0 0000 10 0"),
    case("temporal_off_takes_the_others", [T, D, RC, ("temporal", 0)], "", "0 0 0 0 0 0 1 0000 10 0"),
    case("temporal_off_takes_motion", [T, M, ("temporal", 0)], "", "0 0 0 0 0 0 1 0000 10 0"),
    case("motion_on", [T, F3, M, CAM, F], PRE + " g@0"),
    case("motion_off", [T, M, F3, ("motion", 0), CAM, F], PRE + " g@0"),
    case("deform_on", [T, F3, D, CAM, F], PRE + " g@0"),
    case("deform_off", [T, D, F3, ("deform", 0), CAM, F], PRE + " g@0"),
    # (setHistoryRectification alone of the four keeps the history: it only clears the pending mark)
    case("rectify_on", [T, F3, RC, CAM, F], PRE + " cgrm@3"),
    case("rectify_off", [T, RC, F3, ("rectify", 0), CAM, F], PRE + " cgr@3"),
    case("rectify_set_clears_the_mark", MARKED + [("rectify", 0), RC, ("frame", 10)], MARKED_TRACE + " " + idle(4, 13)),
    # (runBenchmark leaves iteration != 0, so no frame start clears the mark behind it: dropped() has to)
    case("benchmark_drops_the_mark", MARKED + [("benchmark", 5), ("frame", 10)], MARKED_TRACE + " " + idle(4, 13), "0 0 0 11 14 15 0 1001 10 0"),
    # 12. rectification: due once, at the end of the frame in which framesSinceGbuffer + 1 first reaches the delay
    case("rectify_default_delay", MARKED + [("frame", 10)], MARKED_TRACE + " " + idle(4, 11) + " R@12 .@13", "1 0 0 11 14 11 0 1001 10 1"),
    case("rectify_second_reprojection_restarts_the_count", MARKED + [F3, CAM, F, ("frame", 10)],
         MARKED_TRACE + " " + idle(4, 6) + " cgrm@7 " + idle(8, 15) + " R@16 .@17"),
    case("rectify_restart_clears_the_mark", MARKED + [("frame", 2), ("restart",), ("frame", 10)], MARKED_TRACE + " .@4 .@5 " + idle(0, 9)),
    case("rectify_other_change_clears_the_mark", MARKED + [("params", "bounces", 5), ("frame", 13)], MARKED_TRACE + " g@0 " + idle(1, 12)),
    case("rectify_delay_3", [T, RC, ("delay", 3), F3, CAM, F, F3], PRE + " cgrm@3 .@4 R@5 .@6", "1 0 0 4 7 4 0 1001 3 1"),
    case("rectify_delay_1", [T, RC, ("delay", 1), F3, CAM, F, ("frame", 2)], PRE + " cgrm@3 R@4 .@5"),
    case("rectify_delay_0_is_the_default", [T, RC, ("delay", 3), ("delay", 0), F3, CAM, F, ("frame", 10)],
         MARKED_TRACE + " " + idle(4, 11) + " R@12 .@13", "1 0 0 11 14 11 0 1001 10 1"),
]

# 13. init() in every state a sequence of calls reaches -- nothing since the constructor, frames rendered, a move that captured, a refused move
# (captured, nothing dropped), a pending mark, the other integrator -- against dropped(): a move right behind it keeps nothing, the next frame
# traces only and no rectify comes
INIT_STATES = [
    ("fresh", [], "", "mv:. " + idle(0, 11)),
    ("frames", [T, F3], PRE, "mv:. g@0 " + idle(1, 11)),
    ("captured", [T, D, F3, GEOM], PRE + " mv:kc", "mv:. g@0 " + idle(1, 11)),
    ("refused", [T, D, F3, ("update_geometry", "refused")], PRE + " mv:kc", "mv:. g@0 " + idle(1, 11)),
    ("marked", MARKED, MARKED_TRACE, "mv:. g@0 " + idle(1, 11)),
    ("microkernel", [T, F3, ("toggle",)], PRE, "mv:. " + mk(0, 11)),
]
for _state, _events, _before, _after in INIT_STATES:
    for _how in ("init", "dropped"):
        CASES.append(case(f"{_how}_{_state}", _events + [(_how,), GEOM, ("frame", 12)], (_before + " " + _after).strip()))
    CASES.append(case(f"init_{_state}_then_frame", _events + [("init",), ("frame", 2)],
                      (_before + " " + {"fresh": ".@0 .@1", "microkernel": "mk@0 mk@1"}.get(_state, "g@0 .@1")).strip()))
assert len({c["name"] for c in CASES}) == len(CASES)


def script(cases=CASES):
    """the table as tests/tracer_history_cpu.cpp reads it: `case NAME`, one event per line, `end`"""
    out = []
    for c in cases:
        out += [f"case {c['name']}"] + [" ".join(str(x) for x in e).strip() for e in c["events"]] + ["end"]
    return "\n".join(out) + "\n"
