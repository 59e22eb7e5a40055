"""csrc/flx_pose.h on the CPU (host.pose_triangles -- the very function the kernel of flx_objects_pose runs) and the OBJ loader's objects.

  restatement  bit for bit equal to tests/pose_cases.py's float32 numpy restatement on every case and transform
  accuracy     positions within 4 ulp of the float64 version.  WHERE THE BOUND COMES FROM: a position component is three products and three sums,
               each correctly rounded; every intermediate is at most S = sum |m_ij p_j| + |t_i| in magnitude, so the six roundings add up to at
               most 6 x ulp(S) / 2 = 3 ulp(S).  One ulp is therefore measured at S (the O(1) magnitude of the terms, not of a result that
               cancellation may have made small), and 4 leaves one for the rounding of S itself.
  identity     returns the rest bytes, given unit normals
  normals      unit length; on the side of the surface they were on (a point off the surface along the rest normal is carried to the posed
               normal's side), for the mirror too -- there the geometric normal of the posed positions, whose winding the mirror has turned,
               points the other way
  copied       .w words, pad, uv and matId bytes
  absolute     a pose is a function of the rest triangles and the transform alone: nothing a previous pose leaves behind enters it
  OBJ          `o` statements (`g` where a file has none) give every triangle an object; triangles and materials do not change by a byte
  sanitizers   tests/pose_cpu.cpp: the member compaction and the pose under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone
"""
import os
import shutil
import subprocess
import numpy as np
import pytest
import pose_cases as pc
import refit_cases as rc
import refit_subset_cases as sc
from fluctus_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_XF = [(n, b, t) for n, b in pc.CASES for t in pc.TRANSFORM_NAMES]


def _posed(name, builder, tname):
    d = pc.case(name, builder)
    X = pc.transforms(rc.SCENES[name])[tname]
    return d, X, host.pose_triangles(d.tris, X)


@pytest.mark.parametrize("name,builder,tname", CASE_XF)
def test_pose_equals_the_float32_restatement_bit_for_bit(name, builder, tname):
    d, X, got = _posed(name, builder, tname)
    want = pc.pose32(d.tris, X)
    for v in pc.VERTS:
        for f in "pn":
            for k in "xyz":
                bad = got[v][f][k].view(np.uint32) != want[v][f][k].view(np.uint32)
                assert not bad.any(), f"{v}.{f}.{k}: {int(bad.sum())} of {bad.size} differ, first {got[v][f][k][bad][:3]} vs {want[v][f][k][bad][:3]}"
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name,builder,tname", [c for c in CASE_XF if c[0].endswith("-o0")])
def test_positions_within_4_ulp_of_float64(name, builder, tname):
    d, X, got = _posed(name, builder, tname)
    P64, _, mag = pc.pose64(d.tris, X)
    assert mag.max() < 64.0, "the case is not of O(1) magnitude"
    P32 = np.stack([np.stack([got[v]["p"][k] for k in "xyz"], -1) for v in pc.VERTS], 1).astype(np.float64)
    ulp = np.spacing(mag.astype(np.float32)).astype(np.float64)
    err = np.abs(P32 - P64) / ulp
    print(f"{name}/{tname}: largest position error {err.max():.3f} ulp")
    assert err.max() <= 4.0


@pytest.mark.parametrize("name,builder", pc.CASES)
def test_identity_returns_the_rest_bytes(name, builder):
    d, _, got = _posed(name, builder, "identity")
    assert got.tobytes() == d.tris.tobytes()
    # a normal that is not unit length to the last bit is renormalised
    t = d.tris[:4].copy()
    t["v1"]["n"]["x"] *= np.float32(1.5); t["v1"]["n"]["y"] *= np.float32(1.5); t["v1"]["n"]["z"] *= np.float32(1.5)
    out = host.pose_triangles(t, pc.IDENTITY)
    n = np.stack([out["v1"]["n"][k] for k in "xyz"], -1).astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 2e-7 and out["v0"].tobytes() == t["v0"].tobytes()


@pytest.mark.parametrize("name,builder,tname", CASE_XF)
def test_normals_are_unit_and_stay_on_their_side(name, builder, tname):
    d, X, got = _posed(name, builder, tname)
    M = np.asarray(X, np.float64)[:, :3]
    _, U64, _ = pc.pose64(d.tris, X)
    N0 = np.stack([np.stack([d.tris[v]["n"][k] for k in "xyz"], -1) for v in pc.VERTS], 1).astype(np.float64)
    N = np.stack([np.stack([got[v]["n"][k] for k in "xyz"], -1) for v in pc.VERTS], 1).astype(np.float64)
    assert np.abs(np.linalg.norm(N, axis=-1) - 1.0).max() < 2e-7
    assert np.abs(N - U64).max() < 1e-5                      # (the cofactors of a shear or scale cancel: a few hundred ulps of 1 at the worst)
    side = ((N0 @ M.T) * N).sum(-1)                          # M n: where a point just off the surface along n goes
    assert (side > 0).all(), f"{int((side <= 0).sum())} normals ended on the other side of their surface"
    # the geometric normal of the posed positions, in the posed winding, against the posed FACE normals of the unshaded scene
    face = host.pose_triangles(sc.built(name, builder).tris, X)
    P = np.stack([np.stack([face[v]["p"][k] for k in "xyz"], -1) for v in pc.VERTS], 1).astype(np.float64)
    g = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ln = np.linalg.norm(g, axis=1)
    ok = ln > 1e-9 * ln.max()                                # (a sliver whose fp32 posed vertices are nearly collinear says nothing)
    nf = np.stack([face["v0"]["n"][k] for k in "xyz"], -1).astype(np.float64)
    cosine = (g[ok] / ln[ok, None] * nf[ok]).sum(1)
    want = -1.0 if np.linalg.det(M) < 0 else 1.0             # a mirror turns the winding, and the normal does not follow it
    assert np.abs(cosine - want).max() < 1e-2, f"{tname}: posed face normals vs the posed winding: {cosine.min():.4f} .. {cosine.max():.4f}"


@pytest.mark.parametrize("name,builder,tname", CASE_XF)
def test_spare_words_uvs_and_material_ids_are_copied(name, builder, tname):
    d, _, got = _posed(name, builder, tname)
    for v in pc.VERTS:
        assert got[v]["t"].tobytes() == d.tris[v]["t"].tobytes()
        for f in "pn":
            assert got[v][f]["w"].tobytes() == d.tris[v][f]["w"].tobytes()
    assert got["matId"].tobytes() == d.tris["matId"].tobytes() and got["_pad"].tobytes() == d.tris["_pad"].tobytes()
    assert d.tris["_pad"].any() and d.tris["v2"]["n"]["w"].view(np.uint32).all(), "the case carries no marks to lose"


def test_poses_are_absolute():
    name, builder = pc.CASES[0]
    d = pc.case(name, builder)
    xf = pc.transforms(rc.SCENES[name])
    rest = d.tris.copy()
    y_alone = host.pose_triangles(d.tris, xf["shear"])
    host.pose_triangles(d.tris, xf["rotation"])
    assert d.tris.tobytes() == rest.tobytes(), "posing changed the rest triangles"
    assert host.pose_triangles(d.tris, xf["shear"]).tobytes() == y_alone.tobytes()
    # ... whereas feeding a posed triangle back in is the CALLER composing transforms, with its rounding: X then X^-1 comes close, not back
    X = np.vstack([xf["rotation"].astype(np.float64), [0, 0, 0, 1]])
    back = host.pose_triangles(host.pose_triangles(d.tris, xf["rotation"]), np.linalg.inv(X)[:3])
    assert back.tobytes() != rest.tobytes()
    assert np.abs(back["v0"]["p"]["x"] - rest["v0"]["p"]["x"]).max() < 1e-4
    with pytest.raises(ValueError, match="3 x 4"):
        host.pose_triangles(d.tris, np.eye(4))


# ---------------------------------------------------------------------------------------------------------------------------------
OBJ = """mtllib two.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0 0 1
v 1 0 1
v 1 1 1
vn 0 0 1
f 1//1 2//1 3//1
{o1}
usemtl red
f 1//1 2//1 3//1 4//1
{g1}
f 5 6 7
{o2}
usemtl blue
f 1 2 6 5
f 2 3 7
{o1}
f 4 3 7
"""
MTL = "newmtl red\nKd 1 0 0\nnewmtl blue\nKd 0 0 1\n"


def _load(tmp_path, name, **lines):
    (tmp_path / "two.mtl").write_text(MTL)
    p = tmp_path / name
    p.write_text(OBJ.format(**lines))
    return host.load_scene(str(p))


def test_obj_objects_from_o_and_g_statements(tmp_path):
    NO = pc.NO_OBJECT
    plain = _load(tmp_path, "plain.obj", o1="", o2="", g1="")
    assert plain.tris.size == 8 and plain.object_names == [] and (plain.object_of_triangle == NO).all()
    # `o` wins where a file has both; a face in front of the first statement belongs to no object; a name met again continues its object
    a = _load(tmp_path, "o.obj", o1="o table top", o2="o chair", g1="g ignored")
    assert a.object_names == ["table", "chair"]
    assert a.object_of_triangle.tolist() == [NO, 0, 0, 0, 1, 1, 1, 0]
    # `g` where there is no `o`
    b = _load(tmp_path, "g.obj", o1="g first", o2="g second", g1="g third")
    assert b.object_names == ["first", "third", "second"]
    assert b.object_of_triangle.tolist() == [NO, 0, 0, 1, 2, 2, 2, 0]
    for d in (a, b):
        assert d.tris.tobytes() == plain.tris.tobytes() and d.materials.tobytes() == plain.materials.tobytes()
        assert d.texdesc.tobytes() == plain.texdesc.tobytes() and d.type_bits == plain.type_bits
    assert len(set(plain.tris["matId"].tolist())) == 3
    # a loader that knows no objects
    gen = host.generate_scene("kitchen", 500, 3)
    assert gen.object_names == [] and gen.object_of_triangle.size == gen.tris.size and (gen.object_of_triangle == NO).all()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_compaction_and_pose_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/pose_cpu.cpp: flx_pose.h's member count, compaction and pose over heap buffers of exactly the callers' sizes.  Exit status 0 and no
    sanitizer report."""
    exe = str(tmp_path / "pose_cpu")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "pose_cpu.cpp"), "-o", exe]
    assert shutil.which("g++"), "the suite builds its native code with g++"
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout
    assert r.stdout.startswith("ok ")
