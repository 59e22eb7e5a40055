#!/usr/bin/env python3
"""What emissive triangles as lights cost (option "mesh_lights").

    python scripts/bench_mesh_lights.py OUTDIR [--scene kitchen] [--lamps 4000] [--calls 20] [--passes 16] [--warmup 3]

The room is bench.py's stand-in scene (scene and SBVH from bench.build_workload) in which the `--lamps` triangles nearest the ceiling get an
emissive copy of their material and form ONE object.  In a child process under its own time limit, wall clock around the calls + flx_finish:
  rebuild_ms          the table alone: the option switched off and on over the uploaded scene (weights, prefix sums, normalisation on the stream)
  pose_on_ms / pose_off_ms    flx_objects_pose of the lamps (a scale about their centre, another factor per call) with the option on -- the call
                      ends in the rebuild -- and off: the parent commit's call, the yardstick, measured in the same run
  pass_on_ms / pass_off_ms    one microkernel sample pass (raygen, maxBounces + 1 x (next vertex, sample BSDF), splat) at the scene's bench
                      resolution with the option on -- the MESH instances: one more shadow ray per vertex, the table searched -- and off
Writes OUTDIR/bench_mesh_lights.json.  Nothing here is imported by the product or the tests; bench.py's measurement is not involved."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scale_about(centre, s):
    import numpy as np
    X = np.zeros((3, 4), np.float32)
    X[:, :3] = np.eye(3) * s
    X[:, 3] = (1.0 - s) * np.asarray(centre, np.float64)
    return X


def wall(g, calls, warmup):
    for c in calls[:warmup]:
        c()
    g.finish()
    t0 = time.perf_counter()
    for c in calls[warmup:]:
        c()
        g.finish()
    return (time.perf_counter() - t0) / (len(calls) - warmup) * 1e3


def child(a):
    import numpy as np
    import bench
    from fluctus_amd import driver, wire
    from fluctus_amd.device import HipContext, NO_OBJECT
    d, p, _ = bench.build_workload(None, None, a.scene)
    y = (d.tris["v0"]["p"]["y"] + d.tris["v1"]["p"]["y"] + d.tris["v2"]["p"]["y"]) / 3.0
    lamps = np.sort(np.argsort(-y, kind="stable")[:a.lamps]).astype(np.uint32)
    # an emissive copy of each lamp triangle's material
    uniq, inv = np.unique(d.tris["matId"][lamps], return_inverse=True)
    extra = d.materials[uniq].copy()
    for k in "xyz":
        extra["Ke"][k] = 10.0
    d.tris["matId"][lamps] = d.materials.size + inv
    d.materials = np.concatenate([d.materials, extra]).astype(wire.MATERIAL)
    P = np.stack([np.stack([d.tris[v]["p"][k][lamps] for k in "xyz"], 1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)
    centre = 0.5 * (P.min((0, 1)) + P.max((0, 1)))
    omap = np.full(d.tris.size, NO_OBJECT, np.uint32)
    omap[lamps] = 0
    p["useAreaLight"], p["useEnvMap"], p["useRoulette"] = 0, 0, 0
    W, H = int(p["width"]), int(p["height"])
    ids = np.zeros(1, np.uint32)
    n = a.warmup + a.calls
    xfs = [scale_about(centre, 1.0 + 0.01 * (k % 7)) for k in range(n)]
    out = {"scene": a.scene, "triangles": int(d.tris.size), "lamps": int(lamps.size), "width": W, "height": H, "calls": a.calls, "passes": a.passes}
    for on in (1, 0):
        g = HipContext(W * H)
        g.set_option("mesh_lights", on)
        g.upload_scene(d)
        g.objects_define(d.tris, omap, 1)
        g.set_params(p)
        tag = "on" if on else "off"
        if on:
            assert g.mesh_lights_read()[0].size == lamps.size
            out["rebuild_ms"] = wall(g, [lambda: (g.set_option("mesh_lights", 0), g.set_option("mesh_lights", 1)) for _ in range(n)], a.warmup)
        out[f"pose_{tag}_ms"] = wall(g, [lambda X=X: g.objects_pose(ids, X) for X in xfs], a.warmup)
        g.mk_reset()
        out[f"pass_{tag}_ms"] = wall(g, [lambda: driver.render_single_pass(g, p["maxBounces"]) for _ in range(a.warmup + a.passes)], a.warmup)
        out[f"shadow_rays_{tag}"] = int(g.mk_stats()[2])
        g.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--scene", default="kitchen")
    ap.add_argument("--lamps", type=int, default=4000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds for the child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(a.outdir, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--child", "--scene", a.scene, "--lamps", str(a.lamps), "--calls", str(a.calls),
           "--passes", str(a.passes), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
    if r.returncode != 0:
        sys.stdout.write(r.stdout)
        raise SystemExit(f"child exited with {r.returncode}")
    out = {"what": "ms, wall clock: emissive triangles as lights on bench.py's stand-in room (DESIGN.md 4.2.2)", "result": json.loads(r.stdout.strip().splitlines()[-1])}
    with open(os.path.join(a.outdir, "bench_mesh_lights.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
