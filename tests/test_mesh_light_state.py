"""MeshLightState's wavefront member (csrc/flx_feature_state.h) without a GPU: "mesh_lights_wavefront" is a wish of its own
-- set and cleared by its option alone, in either order with "mesh_lights", kept across uploads -- and litWavefront() holds exactly while the
table has lamps and both options are on.  tests/mesh_light_state_cpu.cpp is a stand-alone program that includes only that header, in the manner
of tests/test_feature_state.py."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (events, expected: on, wavefront, usable, lit, litWavefront)
CASES = [
    ("", (0, 0, 0, 0, 0)),
    ("wf_on", (0, 1, 0, 0, 0)),
    ("wf_on upload:3", (0, 1, 0, 0, 0)),                         # inert without "mesh_lights"
    ("on wf_on", (1, 1, 0, 0, 0)),                               # no scene yet
    ("on wf_on upload:3", (1, 1, 1, 1, 1)),
    ("wf_on on upload:3", (1, 1, 1, 1, 1)),                      # the order of the two options does not matter
    ("upload:3 wf_on on", (1, 1, 1, 1, 1)),
    ("upload:3 on wf_on", (1, 1, 1, 1, 1)),
    ("upload:3 on", (1, 0, 1, 1, 0)),                            # "mesh_lights" alone: as before this option existed
    ("on wf_on upload:0", (1, 1, 1, 0, 0)),                      # a scene without emitters
    ("on wf_on upload:3 upload:0", (1, 1, 1, 0, 0)),
    ("on wf_on upload:0 upload:5", (1, 1, 1, 1, 1)),             # both survive an upload
    ("on wf_on upload:3 moved", (1, 1, 1, 1, 1)),                # rebuilt by the call that moved the triangles
    ("on wf_on upload:3 off", (0, 1, 0, 0, 0)),                  # switching "mesh_lights" off leaves the wish standing ...
    ("on wf_on upload:3 off on", (1, 1, 1, 1, 1)),               # ... and it takes effect again
    ("on wf_on upload:3 wf_off", (1, 0, 1, 1, 0)),
    ("on wf_on upload:3 wf_off wf_on", (1, 1, 1, 1, 1)),
]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("mesh_light_state")), "mesh_light_state_cpu")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "mesh_light_state_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and not r.stdout.strip(), "mesh_light_state_cpu.cpp does not compile cleanly:\n" + r.stdout
    r = subprocess.run([exe], input="".join(ev + "\n" for ev, _ in CASES), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]
    assert len(rows) == len(CASES)
    return rows


@pytest.mark.parametrize("i", range(len(CASES)), ids=[ev or "fresh" for ev, _ in CASES])
def test_sequence(results, i):
    assert results[i] == CASES[i][1], CASES[i][0]
