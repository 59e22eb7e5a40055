"""Which call invalidates what under option "deform_history", without a GPU: tests/feature_state_deform_cases.py through
csrc/flx_feature_state.h (tests/feature_state_deform_cpu.cpp, a stand-alone program that includes only that header).
tests/test_gpu_reproject_deform.py runs the same table through the C ABI; tests/test_feature_state.py keeps running the table that was there
before, untouched, against the same header."""
import os
import subprocess
import pytest
import feature_state_deform_cases as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpu(outdir, *flags):
    """g++ -std=c++17 tests/feature_state_deform_cpu.cpp -> <outdir>/feature_state_deform_cpu.  A failed compile raises."""
    exe = os.path.join(str(outdir), "feature_state_deform_cpu")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", *flags, os.path.join(ROOT, "tests", "feature_state_deform_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and not r.stdout.strip(), "feature_state_deform_cpu.cpp does not compile cleanly:\n" + r.stdout
    return exe


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case of the table in one run of the program: {name: fields}"""
    exe = build_cpu(tmp_path_factory.mktemp("feature_state_deform"))
    r = subprocess.run([exe], input=fs.script(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in r.stdout.splitlines()]
    assert [x[0] for x in rows] == [c["name"] for c in fs.CASES]
    return {x[0]: [int(v) for v in x[1:]] for x in rows}


@pytest.mark.parametrize("case", fs.CASES, ids=[c["name"] for c in fs.CASES])
def test_sequence(results, case):
    f = results[case["name"]]
    assert tuple(f[:6]) == case["expect"], f
    if "snapshots" in case:
        assert f[6] == case["snapshots"], f


def test_table_covers_what_it_must():
    ev = [[e[1][0] if e[0] == "refused" else e[0] for e in c["events"]] for c in fs.CASES]
    names = {c["name"] for c in fs.CASES}
    for kind in ("opt", "define", "pose", "gbuffer", "capture", "gb_write", "bary_write", "reproject", "upload", "update", "subset", "update_nan", "resize"):
        assert any(kind in e for e in ev), kind
    # the sequences the option's definition names
    assert {"two_moves_after_one_capture", "refused_move", "motion_refused_under_deform", "deform_refused_under_motion",
            "off_with_a_snapshot_drops_the_history", "off_without_a_snapshot_keeps_it"} <= names
