#!/usr/bin/env python3
"""Cost of moving an object by its transform (flx_objects_pose) against handing the same triangles to flx_update_triangles_subset
(DESIGN.md 4.10.3).

    python scripts/bench_pose.py OUTDIR [--scenes kitchen courtyard-1440p] [--calls 20] [--warmup 3]

Per scene (bench.py's stand-ins: scene and SBVH from bench.build_workload), in a child process of its own under its own time limit: ONE object -- the
triangles whose centroid lies in a cube around the median centroid, sized to hold about an eighth of the triangles -- rotated about the cube's
centre by another angle in every call.  ms per call, wall clock around the call + flx_finish (the blocking validation read included), and the device
time of the kernels alone (flx_profile level 1, FLX_K_REFIT: for a pose the pose kernels and the refit passes together), for
  pose           flx_objects_pose: 48 bytes cross the bus, the triangles are made on the device
  host_source    flx_update_triangles_subset with a host source for the same triangles (posed beforehand: the CPU's pose is not in the figure)
  device_source  flx_update_triangles_subset with a device source for the same triangles
The last two are the parent commit's code, unchanged: the yardstick, measured in the same run.
Writes OUTDIR/bench_pose.json.  Nothing here is imported by the product or the tests; bench.py's measurement is not involved."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def rotation_about(centre, angle):
    import numpy as np
    c, s = np.cos(angle), np.sin(angle)
    M = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    X = np.zeros((3, 4), np.float32)
    X[:, :3] = M
    X[:, 3] = np.asarray(centre, np.float64) - M @ np.asarray(centre, np.float64)
    return X


def timed(g, calls_list, a):
    """calls_list: warmup + calls closures, one per call (every call its own angle)"""
    from fluctus_amd.device import K_REFIT
    for call in calls_list[:a.warmup]:
        call()
    g.finish()
    g.profile_reset(); g.profile_enable(1)
    t0 = time.perf_counter()
    for call in calls_list[a.warmup:]:
        call()
        g.finish()
    wall = (time.perf_counter() - t0) / a.calls * 1e3
    g.profile_enable(0)
    ms, _ = g.kernel_profile(K_REFIT)
    return {"ms_per_call_wall": wall, "ms_kernels_device": ms / a.calls}


def child(a):
    import torch
    import numpy as np
    import bench
    from bench_update_subset import box_subset
    from fluctus_amd import host
    from fluctus_amd.device import HipContext, NO_OBJECT
    d, _, _ = bench.build_workload(None, None, a.scene)
    idx, _ = box_subset(d, 0.125)
    P = np.stack([np.stack([d.tris[v]["p"][k][idx] for k in "xyz"], 1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)
    centre = 0.5 * (P.min((0, 1)) + P.max((0, 1)))
    omap = np.full(d.tris.size, NO_OBJECT, np.uint32)
    omap[idx] = 0
    n = a.warmup + a.calls
    xfs = [rotation_about(centre, 0.02 * (k + 1)) for k in range(n)]
    g = HipContext(1 << 20)
    g.upload_scene(d)
    g.objects_define(d.tris, omap, 1)
    out = {"scene": a.scene, "triangles": int(d.tris.size), "object_triangles": int(idx.size), "fraction": idx.size / d.tris.size, "calls": a.calls}
    ids = np.zeros(1, np.uint32)
    out["pose"] = timed(g, [lambda X=X: g.objects_pose(ids, X) for X in xfs], a)
    rest = np.ascontiguousarray(d.tris[idx])
    posed = [host.pose_triangles(rest, X) for X in xfs]
    g.upload_scene(d)
    out["host_source"] = timed(g, [lambda t=t: g.update_triangles_subset(t, idx) for t in posed], a)
    dev_idx = torch.from_numpy(idx.astype(np.int32)).cuda()
    dev = [torch.from_numpy(np.frombuffer(t.tobytes(), np.uint8).copy()).cuda() for t in posed[:a.warmup + 2]]   # (two buffers alternate: 8.9 M x 160 B each)
    g.upload_scene(d)
    out["device_source"] = timed(g, [lambda k=k: g.update_triangles_subset(dev[k % len(dev)], dev_idx, on_device=True) for k in range(n)], a)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--scenes", nargs="+", default=["kitchen", "courtyard-1440p"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds per scene's child process")
    ap.add_argument("--scene", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.scene:
        return child(a)
    out = {"what": "ms per call: one object of about an eighth of the triangles, a rotation per call (DESIGN.md 4.10.3)", "scenes": []}
    os.makedirs(a.outdir, exist_ok=True)
    for s in a.scenes:
        cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--scene", s, "--calls", str(a.calls), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            raise SystemExit(f"{s}: child exited with {r.returncode}")            # nothing more is started on the GPU
        out["scenes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        with open(os.path.join(a.outdir, "bench_pose.json"), "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
