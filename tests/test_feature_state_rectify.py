"""Which call drops the mark of flx_history_mark, without a GPU: tests/feature_state_rectify_cases.py through csrc/flx_feature_state.h
(tests/feature_state_rectify_cpu.cpp, a stand-alone program that includes only that header).  tests/test_gpu_feature_state_rectify.py runs the
same table through the C ABI."""
import os
import subprocess
import pytest
import feature_state_rectify_cases as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case of the table in one run of the program: {name: fields}"""
    exe = os.path.join(str(tmp_path_factory.mktemp("feature_state_rectify")), "feature_state_rectify_cpu")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "feature_state_rectify_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and not r.stdout.strip(), "feature_state_rectify_cpu.cpp does not compile cleanly:\n" + r.stdout
    r = subprocess.run([exe], input=fs.script(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in r.stdout.splitlines()]
    assert [x[0] for x in rows] == [c["name"] for c in fs.CASES]
    return {x[0]: tuple(int(v) for v in x[1:]) for x in rows}


@pytest.mark.parametrize("case", fs.CASES, ids=[c["name"] for c in fs.CASES])
def test_sequence(results, case):
    assert results[case["name"]] == case["expect"]


def test_table_covers_what_it_must():
    """every call the mark is dropped by, the one that must keep it, and the refusals"""
    ev = [[e[1][0] if e[0] == "refused" else e[0] for e in c["events"]] for c in fs.CASES]
    for kind in ("mark", "rectify", "rectify_bad", "wf_reset", "mk_reset", "resize", "partition", "capture", "update", "subset", "pose", "upload",
                 "write_pixels", "gbuffer", "gb_write"):
        assert any(kind in e for e in ev), kind
    dropped = [c for c in fs.CASES if "mark" in [e[0] for e in c["events"]] and c["expect"][1] == 0]
    assert len(dropped) >= 11
    assert all(c["expect"][1] >= c["expect"][2] and c["expect"][1] >= c["expect"][3] for c in fs.CASES)
