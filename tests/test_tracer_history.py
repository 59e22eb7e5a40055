"""What each public Tracer call does to the history, without a GPU: tests/tracer_history_cases.py through host/history_state.hpp
(tests/tracer_history_cpu.cpp, a stand-alone program that includes only that header), once as an ordinary build and once under the address and
undefined-behaviour sanitizers.  The Tracer tests of tests/test_gpu_reproject*.py and tests/test_gpu_rectify.py see the same decisions on the device."""
import os
import subprocess
import pytest
import tracer_history_cases as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": (), "sanitized": ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")}


def build_cpu(outdir, *flags):
    """g++ -std=c++17 tests/tracer_history_cpu.cpp -> <outdir>/tracer_history_cpu.  A failed compile or a warning raises."""
    exe = os.path.join(str(outdir), "tracer_history_cpu")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", *flags, os.path.join(ROOT, "tests", "tracer_history_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and not r.stdout.strip(), "tracer_history_cpu.cpp does not compile cleanly:\n" + r.stdout
    return exe


@pytest.fixture(scope="module", params=sorted(BUILDS))
def results(request, tmp_path_factory):
    """every case of the table in one run of the program: {name: (trace, flags)}"""
    exe = build_cpu(tmp_path_factory.mktemp("tracer_history_" + request.param), *BUILDS[request.param])
    r = subprocess.run([exe], input=th.script(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    rows = [l.split(" | ") for l in r.stdout.splitlines()]
    names = [x[0].split()[0] for x in rows]
    assert names == [c["name"] for c in th.CASES]
    return {n: (" ".join(x[0].split()[1:]), x[1].strip()) for n, x in zip(names, rows)}


@pytest.mark.parametrize("case", th.CASES, ids=[c["name"] for c in th.CASES])
def test_sequence(results, case):
    trace, flags = results[case["name"]]
    assert trace == case["trace"], (trace, flags)
    if case["flags"] is not None:
        assert flags == case["flags"], (trace, flags)


def test_init_is_dropped_in_every_state(results):
    for state, *_ in th.INIT_STATES:
        assert results["init_" + state] == results["dropped_" + state], state


def test_table_covers_what_it_must():
    ev = [e for c in th.CASES for e in c["events"]]
    assert len(th.CASES) >= 60
    for kind in ("frame", "temporal", "motion", "deform", "rectify", "delay", "params", "update_geometry", "pose", "adopt_rebuild", "define", "envmap",
                 "toggle", "mesh_lights", "mesh_lights_wavefront", "render_single", "render_adaptive", "benchmark", "init", "dropped", "restart"):
        assert any(e[0] == kind for e in ev), kind
    for what in ("camera", "exposure", "light", "bounces", "size"):
        assert any(e[0] == "params" and e[1] == what for e in ev), what
    for move in ("update_geometry", "pose"):
        for how in ("", "refused", "reupload"):
            assert any(e == (move, how) for e in ev), (move, how)
    for switch in ("temporal", "motion", "deform", "rectify"):
        for on in (0, 1):
            assert any(e == (switch, on) for e in ev), (switch, on)
