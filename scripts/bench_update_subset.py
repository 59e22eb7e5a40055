#!/usr/bin/env python3
"""Cost of flx_update_triangles_subset against flx_update_triangles with the same resulting triangles, and what each leaves to traverse
(DESIGN.md 4.10.2).

    python scripts/bench_update_subset.py OUTDIR [--scenes kitchen conference courtyard-1440p] [--calls 20] [--warmup 3] [--iters 6]

Per scene (bench.py's stand-ins: scene, SBVH and camera from bench.build_workload), in a child process of its own under its own time limit, and per
subset -- the triangles whose centroid lies in a cube around the median centroid, sized to hold about 1 % and about 10 % of the triangles,
translated by 2 % of the scene's extent along x:
  update    ms per call for a host source (wall clock around the call + flx_finish: PCIe copy and the blocking validation read included) and for
            a device source (torch tensors), and the device time of the passes alone (flx_profile level 1, FLX_K_REFIT) -- for the subset call and,
            same box, same run, for flx_update_triangles given the whole resulting triangle array (the path of the parent commit)
  traverse  Mrays/s of flx_wf_extend / flx_wf_shadow (flx_profile level 2) over --iters benchmark iterations from the same camera and seeds on
            "upload, one subset update", on "upload, one full update" and on a tree rebuilt for the resulting triangles; flx_tree_cost's two figures
            for each
Writes OUTDIR/bench_update_subset.json.  Nothing here is imported by the product or the tests; bench.py's measurement is not involved."""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def box_subset(d, fraction):
    """(ascending indices of the triangles whose centroid lies in the cube around the median centroid that holds `fraction` of them, extent)"""
    import numpy as np
    P = np.stack([np.stack([d.tris[v]["p"][k] for k in "xyz"], 1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)
    c = P.mean(1)
    dist = np.abs(c - np.median(c, 0)).max(1)
    idx = np.nonzero(dist <= np.quantile(dist, fraction))[0].astype(np.uint32)
    return idx, float((P.max((0, 1)) - P.min((0, 1))).max())


def moved(d, idx, dx):
    """a copy of d (same tree) whose triangles idx are translated by dx along x"""
    import numpy as np
    m = copy.copy(d)
    m.tris, m.nodes = d.tris.copy(), d.nodes.copy()
    for v in ("v0", "v1", "v2"):
        x = m.tris[v]["p"]["x"]
        x[idx] = np.float32(x[idx] + np.float32(dx))
    return m


def timed(g, call, a):
    from fluctus_amd.device import K_REFIT
    for _ in range(a.warmup):
        call()
    g.finish()
    g.profile_reset(); g.profile_enable(1)
    t0 = time.perf_counter()
    for _ in range(a.calls):
        call()
        g.finish()
    wall = (time.perf_counter() - t0) / a.calls * 1e3
    g.profile_enable(0)
    ms, k = g.kernel_profile(K_REFIT)
    return {"ms_per_call_wall": wall, "ms_passes_device": ms / max(1, k), "calls": int(k)}


def child(a):
    import torch
    import numpy as np
    import bench
    import bench_refit
    from fluctus_amd import host
    from fluctus_amd.device import HipContext, tree_cost_value
    name = a.scene
    d, p, env = bench.build_workload(None, None, name)
    g = HipContext(1 << 20)
    g.upload_scene(d)
    info = g.scene_info()
    out = {"scene": name, "triangles": int(d.tris.size), "index_list": int(d.indices.size), "binary_records": info["binary_records"],
           "wide_nodes": info["wide_nodes"], "subsets": {}}

    def figures(scene):
        b, w = g.tree_cost()
        pm = p.copy(); pm["worldRadius"] = scene.world_radius
        r = bench_refit.traverse(g, scene, pm, env, a.iters)
        r["cost_binary"], r["cost_wide"] = tree_cost_value(b), tree_cost_value(w)
        return r

    out["uploaded_tree"] = figures(d)
    for label, fraction in (("1pct", 0.01), ("10pct", 0.10)):
        idx, ext = box_subset(d, fraction)
        m = moved(d, idx, 0.02 * ext)
        sub = np.ascontiguousarray(m.tris[idx])
        dev_all = torch.from_numpy(np.frombuffer(m.tris.tobytes(), np.uint8).copy()).cuda()
        dev_sub = torch.from_numpy(np.frombuffer(sub.tobytes(), np.uint8).copy()).cuda()
        dev_idx = torch.from_numpy(idx.astype(np.int32)).cuda()
        res = {"triangles_moved": int(idx.size), "fraction": idx.size / d.tris.size}
        # the subset call: "upload, one subset update" is what is traversed (repeating the call rewrites the same records)
        g.upload_scene(d); g.update_triangles_subset(sub, idx); g.finish()
        host.refit_bvh_subset(m, idx)                    # world_radius of the moved scene for the parameters
        res["subset"] = {"traverse": figures(m),
                         "host_source": timed(g, lambda: g.update_triangles_subset(sub, idx), a),
                         "device_source": timed(g, lambda: g.update_triangles_subset(dev_sub, dev_idx, on_device=True), a)}
        # the parent commit's path: the whole resulting array through flx_update_triangles
        g.upload_scene(d); g.update_triangles(m); g.finish()
        res["full"] = {"traverse": figures(m),
                       "host_source": timed(g, lambda: g.update_triangles(m), a),
                       "device_source": timed(g, lambda: g.update_triangles(dev_all, on_device=True), a)}
        # a tree rebuilt for the resulting triangles
        t0 = time.perf_counter()
        host.build_bvh(m, "sbvh")
        t1 = time.perf_counter()
        g.upload_scene(m); g.finish()
        t2 = time.perf_counter()
        res["rebuilt"] = {"traverse": figures(m), "rebuild_ms": {"build_bvh": (t1 - t0) * 1e3, "upload_scene": (t2 - t1) * 1e3}}
        out["subsets"][label] = res
        del dev_all, dev_sub, dev_idx
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--scenes", nargs="+", default=["kitchen", "conference", "courtyard-1440p"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--limit", type=int, default=420, help="seconds per scene's child process")
    ap.add_argument("--scene", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.scene:
        return child(a)
    out = {"schedule": "level-synchronous, stamps (DESIGN.md 4.10.2)", "scenes": []}
    os.makedirs(a.outdir, exist_ok=True)
    for s in a.scenes:
        cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--scene", s, "--calls", str(a.calls), "--warmup", str(a.warmup), "--iters", str(a.iters)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            raise SystemExit(f"{s}: child exited with {r.returncode}")            # nothing more is started on the GPU
        out["scenes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        with open(os.path.join(a.outdir, "bench_update_subset.json"), "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
