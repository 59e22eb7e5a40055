"""Which call invalidates what, without a GPU: tests/feature_state_cases.py through csrc/flx_feature_state.h (tests/feature_state_cpu.cpp, a
stand-alone program that includes only that header).  tests/test_gpu_feature_state.py runs the same table through the C ABI."""
import os
import subprocess
import pytest
import feature_state_cases as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpu(outdir, *flags):
    """g++ -std=c++17 tests/feature_state_cpu.cpp -> <outdir>/feature_state_cpu.  A failed compile raises."""
    exe = os.path.join(str(outdir), "feature_state_cpu")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", *flags, os.path.join(ROOT, "tests", "feature_state_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and not r.stdout.strip(), "feature_state_cpu.cpp does not compile cleanly:\n" + r.stdout
    return exe


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case of the table in one run of the program: {name: fields}"""
    exe = build_cpu(tmp_path_factory.mktemp("feature_state"))
    r = subprocess.run([exe], input=fs.script(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in r.stdout.splitlines()]
    assert [x[0] for x in rows] == [c["name"] for c in fs.CASES]
    return {x[0]: x[1:] for x in rows}


@pytest.mark.parametrize("case", fs.CASES, ids=[c["name"] for c in fs.CASES])
def test_sequence(results, case):
    f = results[case["name"]]
    flags, (Hm, D, moved), known, known_cap = tuple(int(v) for v in f[:6]), (int(v) for v in f[6:9]), f[9].strip("-"), f[10].strip("-")
    assert flags == case["expect"], f
    got = dict(Hm=Hm, D=D, moved=moved, known=known, knownCap=known_cap)
    for k in got:
        if k in case:
            assert got[k] == case[k], (k, f)
    if "moved" in case:
        assert flags[4] == 1                                 # only a captured history gives the GPU executor a way to see it


def test_table_covers_what_it_must():
    ev = [[e[1][0] if e[0] == "refused" else e[0] for e in c["events"]] for c in fs.CASES]
    assert len(fs.CASES) >= 20
    for kind in ("define", "pose", "gbuffer", "capture", "gb_write", "obj_write", "upload", "upload_refused", "update", "subset", "resize",
                 "partition", "mk_reset", "adaptive_clear", "adaptive_update", "active_write", "denoise"):
        assert any(kind in e for e in ev), kind
